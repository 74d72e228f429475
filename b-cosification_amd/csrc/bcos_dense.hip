// bcos_dense.hip -- the two streaming kernels a densely connected (DenseNet) plan needs around the contraction kernels: the
// pre-activation BatchNormUncentered + ReLU a dense layer / transition / head applies to a channel SLICE of the block's concatenated
// feature buffer (torchvision _DenseLayer: norm1 -> relu1 -> conv1 over cat(features); reference standard_models.py:56-63,
// batchnorm_uncentered.py:46-60), and its input gradient accumulated into the same slice of the block's gradient buffer.
// Both walk rows of C floats inside rows of `pitch` floats with 16-byte accesses; a wavefront owns whole rows (C / 4 lanes per row
// where that divides 64, otherwise 64 lanes looping over the row), so the row maximum is a cross-lane reduction without atomics.
// Per-channel constants sit in registers (a lane keeps its channel quad for every row) or in LDS (looping form).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

// x * scale + shift is TWO roundings here, as in bcos_channel_affine_rows (bcos_train.hip), whose bits bcos_slice_affine_rows must
// reproduce; and the gate of the backward kernel is decided on exactly the value the forward kernel compared with zero.
#pragma clang fp contract(off)

namespace {

constexpr int MAX_LDS_C = 8192;            // scale + shift of the looping form: 2 x 32 KiB of dynamic LDS at most

// per-channel constants of one lane: registers when the lane's channel quad is the same for every row (LPR < 64), LDS otherwise
template <int LPR>
struct ChannelConsts {
    f32x4 sc, sh;
    const float* lds;
    int C;
    __device__ __forceinline__ void load(const float* __restrict__ scale, const float* __restrict__ shift, float* smem, int C_, int l) {
        C = C_;
        lds = smem;
        if constexpr (LPR == 64) {
            for (int c = threadIdx.x * 4; c < C; c += 256 * 4) {
                if (scale) *reinterpret_cast<f32x4*>(smem + c) = *reinterpret_cast<const f32x4*>(scale + c);
                if (shift) *reinterpret_cast<f32x4*>(smem + C + c) = *reinterpret_cast<const f32x4*>(shift + c);
            }
            __syncthreads();
        } else {
            if (scale) sc = *reinterpret_cast<const f32x4*>(scale + l * 4);
            if (shift) sh = *reinterpret_cast<const f32x4*>(shift + l * 4);
        }
    }
    __device__ __forceinline__ f32x4 scale_at(int c) const {
        if constexpr (LPR == 64) return *reinterpret_cast<const f32x4*>(lds + c);
        else return sc;
    }
    __device__ __forceinline__ f32x4 shift_at(int c) const {
        if constexpr (LPR == 64) return *reinterpret_cast<const f32x4*>(lds + C + c);
        else return sh;
    }
};

// the value whose sign is the ReLU's decision: ONE definition for the forward kernel and for the gate of the backward kernel
template <int LPR>
__device__ __forceinline__ f32x4 pre_activation(f32x4 v, const ChannelConsts<LPR>& k, bool has_scale, bool has_shift, int c) {
    if (has_scale) v = v * k.scale_at(c);
    if (has_shift) v = v + k.shift_at(c);
    return v;
}

template <int LPR>
__global__ __launch_bounds__(256) void slice_affine_rows_kernel(const float* __restrict__ x, int64_t x_pitch, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* __restrict__ mul,
                                                                float* __restrict__ y, int64_t y_pitch, unsigned* __restrict__ absmax,
                                                                int64_t rows, int C, int relu) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RPW = 64 / LPR;                        // rows per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR, l = lane % LPR;
    ChannelConsts<LPR> k;
    k.load(scale, shift, smem, C, l);
    const bool has_scale = scale != nullptr, has_shift = shift != nullptr;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {        // (wave-uniform trip count: the shuffles below see every lane)
        const int64_t row = r0 + sub;
        const bool live = row < rows;
        unsigned mx = 0u;
        if (live)
            for (int c = l * 4; c < C; c += LPR * 4) {
                f32x4 v = pre_activation<LPR>(*reinterpret_cast<const f32x4*>(x + row * x_pitch + c), k, has_scale, has_shift, c);
                if (relu) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
                }
                if (mul) v = v * __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mul + row * C + c));     // read exactly once
#pragma unroll
                for (int q = 0; q < 4; ++q) mx = max(mx, __float_as_uint(v[q]) & 0x7fffffffu);
                *reinterpret_cast<f32x4*>(y + row * y_pitch + c) = v;
            }
        if (absmax) {
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
            if (live && l == 0) absmax[row] = mx;
        }
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void slice_affine_bwd_acc_kernel(const float* __restrict__ d, const float* __restrict__ x, int64_t x_pitch,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   float* __restrict__ g, int64_t g_pitch, int64_t rows, int C, int relu,
                                                                   int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR, l = lane % LPR;
    ChannelConsts<LPR> k;
    k.load(scale, shift, smem, C, l);
    const bool has_scale = scale != nullptr, has_shift = shift != nullptr;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const int64_t row = r0 + sub;
        if (row >= rows) continue;
        for (int c = l * 4; c < C; c += LPR * 4) {
            f32x4 p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d + row * C + c));              // read exactly once
            if (has_scale) p = p * k.scale_at(c);
            if (relu) {
                const f32x4 v = pre_activation<LPR>(*reinterpret_cast<const f32x4*>(x + row * x_pitch + c), k, has_scale, has_shift, c);
#pragma unroll
                for (int q = 0; q < 4; ++q) p[q] = v[q] > 0.f ? p[q] : 0.f;
            }
            f32x4* dst = reinterpret_cast<f32x4*>(g + row * g_pitch + c);
            if (accumulate) p = *dst + p;
            *dst = p;
        }
    }
}

// ---- training mode: BatchNormUncentered2d with batch statistics over a channel slice (batchnorm_uncentered.py:36-44) -------------------
// Column reductions over a slice use ONE geometry whatever the slice: a workgroup owns a block of rows and a tile of CQ = 8 channel
// quads (32 channels, 128 contiguous bytes of a row); thread (tc, tr) = (threadIdx.x % 8, threadIdx.x / 8) owns quad tc of the tile and
// the rows r_lo + tr, r_lo + tr + 32, ... of the block, four rows in flight, added in row order; the 32 row lanes of a quad meet in LDS
// in lane order; a finish launch adds the workgroups' partials of a channel in workgroup order.  The row blocks follow from `rows`
// alone (col_plan), so everything that happens to a column -- and therefore every bit of its sums -- depends on `rows` and on the
// column's own values, not on C, the pitch, the slice offset or the other columns of the call.
constexpr int CQ = 8, RL = 32;

template <typename T>
__device__ __forceinline__ void lane_merge(float (*red)[256 * 4], int tc, int tr, T& s1, T& s2) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[0][threadIdx.x * 4 + q] = s1[q]; red[1][threadIdx.x * 4 + q] = s2[q]; }
    __syncthreads();
    if (tr == 0)
        for (int k = 1; k < RL; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) { s1[q] += red[0][(k * CQ + tc) * 4 + q]; s2[q] += red[1][(k * CQ + tc) * 4 + q]; }
}

// partial[b] = (c, S1, S2) per channel: c = the block's first row, S1 = sum (x - c), S2 = sum (x - c)^2 (bn_stats_partial_kernel's scheme)
__global__ __launch_bounds__(256) void slice_stats_partial_kernel(const float* __restrict__ x, int64_t pitch, float* __restrict__ partial,
                                                                  int64_t rows, int C, int64_t rpb) {
    __shared__ float red[2][256 * 4];
    const int tc = threadIdx.x % CQ, tr = threadIdx.x / CQ;
    const int cg = blockIdx.y * CQ + tc;
    const bool live = cg < C / 4;
    const int64_t r_lo = (int64_t)blockIdx.x * rpb;
    const int64_t r_hi = r_lo + rpb < rows ? r_lo + rpb : rows;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* col = x + cg * 4;
        c = *reinterpret_cast<const f32x4*>(col + r_lo * pitch);
        int64_t r = r_lo + tr;
        for (; r + 3 * RL < r_hi; r += 4 * RL) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(col + (r + u * RL) * pitch);
#pragma unroll
            for (int u = 0; u < 4; ++u) { const f32x4 d = v[u] - c; s1 += d; s2 += d * d; }
        }
        for (; r < r_hi; r += RL) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(col + r * pitch) - c;
            s1 += d;
            s2 += d * d;
        }
    }
    lane_merge(red, tc, tr, s1, s2);
    if (tr == 0 && live) {
        float* dst = partial + (int64_t)blockIdx.x * 3 * C + cg * 4;
        *reinterpret_cast<f32x4*>(dst) = c;
        *reinterpret_cast<f32x4*>(dst + C) = s1;
        *reinterpret_cast<f32x4*>(dst + 2 * C) = s2;
    }
}

// fixed-order sum over the workgroups b of f(b) for one channel: 16 lanes, lane t takes b = t, t + 16, ... in order, the 16 partial sums
// meet in lane order (the shape of bcos_train.hip's finish kernels)
template <typename F>
__device__ __forceinline__ float ordered_block_sum(float* red, int tc, int tr, int nblk, bool live, F f) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (live) {
        int b = tr;
        for (; b + 48 < nblk; b += 64) { a0 += f(b); a1 += f(b + 16); a2 += f(b + 32); a3 += f(b + 48); }
        for (; b < nblk; b += 16) a0 += f(b);
    }
    __syncthreads();
    red[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    float acc = red[tc];
    for (int k = 1; k < 16; ++k) acc += red[k * 16 + tc];
    return acc;
}

// (n_b, mean_b, M2_b) of the workgroups combined in workgroup order (Chan et al.): mean, and the centred second moment over `rows`
__global__ __launch_bounds__(256) void slice_stats_finish_kernel(const float* __restrict__ partial, float* __restrict__ mean_out,
                                                                 float* __restrict__ var_out, int nblk, int C, int64_t rows, int64_t rpb) {
    __shared__ float red[256];
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + tc;
    const bool live = c < C;
    auto nb = [&](int b) { const int64_t lo = (int64_t)b * rpb; return (float)((lo + rpb < rows ? lo + rpb : rows) - lo); };
    const float m = (float)rows;
    const float total = ordered_block_sum(red, tc, tr, nblk, live, [&](int b) {
        const float* q = partial + (int64_t)b * 3 * C + c;
        return nb(b) * q[0] + q[C];
    });
    const float mean = total / m;
    const float m2 = ordered_block_sum(red, tc, tr, nblk, live, [&](int b) {
        const float* q = partial + (int64_t)b * 3 * C + c;
        const float n = nb(b), s1 = q[C];
        const float d = q[0] + s1 / n - mean;
        return q[2 * C] - s1 * s1 / n + n * d * d;
    });
    if (tr == 0 && live) {
        mean_out[c] = mean;
        var_out[c] = fmaxf(m2 / m, 0.f);
    }
}

// what ONE reader of a channel range makes of the shared (mean, var): its own 1 / std, weight / std and running_var update
__global__ __launch_bounds__(256) void bn_reader_finish_kernel(const float* __restrict__ var, const float* __restrict__ weight,
                                                               float* __restrict__ running_var, float* __restrict__ rstd_out,
                                                               float* __restrict__ g_out, int C, float eps, float momentum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float v = var[c];
    const float rstd = rsqrtf(v + eps);
    rstd_out[c] = rstd;
    g_out[c] = weight ? weight[c] * rstd : rstd;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * v;
}

// partial[b] = (sum gate d x, sum gate d) per channel, gate = (x g + shift > 0) as the forward kernel decided it
__global__ __launch_bounds__(256) void slice_relu_bwd_colsums_kernel(const float* __restrict__ d, const float* __restrict__ x, int64_t pitch,
                                                                     const float* __restrict__ gvec, const float* __restrict__ shift,
                                                                     float* __restrict__ partial, int64_t rows, int C, int64_t rpb) {
    __shared__ float red[2][256 * 4];
    const int tc = threadIdx.x % CQ, tr = threadIdx.x / CQ;
    const int cg = blockIdx.y * CQ + tc;
    const bool live = cg < C / 4;
    const int64_t r_lo = (int64_t)blockIdx.x * rpb;
    const int64_t r_hi = r_lo + rpb < rows ? r_lo + rpb : rows;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(gvec + cg * 4);
        f32x4 sh = {0.f, 0.f, 0.f, 0.f};
        if (shift) sh = *reinterpret_cast<const f32x4*>(shift + cg * 4);
        const bool has_shift = shift != nullptr;
        auto rows_u = [&](auto u_c, int64_t r) {                 // U rows in flight: all loads first, then the chain in row order
            constexpr int U = decltype(u_c)::value;
            f32x4 dv[U], xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                dv[u] = *reinterpret_cast<const f32x4*>(d + (r + u * RL) * C + cg * 4);      // (bcos_slice_bn_bwd_acc reads d again: no streaming hint)
                xv[u] = *reinterpret_cast<const f32x4*>(x + (r + u * RL) * pitch + cg * 4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                f32x4 v = xv[u] * sc;                            // (the two roundings of pre_activation)
                if (has_shift) v = v + sh;
#pragma unroll
                for (int q = 0; q < 4; ++q) dv[u][q] = v[q] > 0.f ? dv[u][q] : 0.f;
                s1 += dv[u] * xv[u];
                s2 += dv[u];
            }
        };
        int64_t r = r_lo + tr;
        for (; r + 3 * RL < r_hi; r += 4 * RL) rows_u(std::integral_constant<int, 4>{}, r);
        for (; r < r_hi; r += RL) rows_u(std::integral_constant<int, 1>{}, r);
    }
    lane_merge(red, tc, tr, s1, s2);
    if (tr == 0 && live) {
        float* dst = partial + (int64_t)blockIdx.x * 2 * C + cg * 4;
        *reinterpret_cast<f32x4*>(dst) = s1;
        *reinterpret_cast<f32x4*>(dst + C) = s2;
    }
}

__global__ __launch_bounds__(256) void slice_bn_bwd_finish_kernel(const float* __restrict__ partial, const float* __restrict__ rstd,
                                                                  const float* __restrict__ gvec, float* __restrict__ sgx_out,
                                                                  float* __restrict__ sg_out, float* __restrict__ gw_out,
                                                                  float* __restrict__ coef_out, int nblk, int C, int64_t rows) {
    __shared__ float red[256];
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + tc;
    const bool live = c < C;
    const float sgx = ordered_block_sum(red, tc, tr, nblk, live, [&](int b) { return partial[(int64_t)b * 2 * C + c]; });
    float sg = 0.f;
    if (sg_out) sg = ordered_block_sum(red, tc, tr, nblk, live, [&](int b) { return partial[(int64_t)b * 2 * C + C + c]; });
    if (tr == 0 && live) {
        sgx_out[c] = sgx;
        if (sg_out) sg_out[c] = sg;
        if (gw_out) gw_out[c] = sgx * rstd[c];
        if (coef_out) coef_out[c] = -(gvec[c] * sgx) * rstd[c] * rstd[c] / (float)rows;
    }
}

// G = (accumulate ? G : 0) + gate d g + (x - mean) coef; with mean / coef NULL the arithmetic of slice_affine_bwd_acc_kernel, bit for bit.
// The looping form keeps g / shift in LDS and reads mean / coef (once per row and quad, cached) from memory.
template <int LPR>
__global__ __launch_bounds__(256) void slice_bn_bwd_acc_kernel(const float* __restrict__ d, const float* __restrict__ x, int64_t x_pitch,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ mean, const float* __restrict__ coef,
                                                               float* __restrict__ g, int64_t g_pitch, int64_t rows, int C, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR, l = lane % LPR;
    ChannelConsts<LPR> k;
    k.load(scale, shift, smem, C, l);
    const bool has_scale = scale != nullptr, has_shift = shift != nullptr, has_var = coef != nullptr;
    f32x4 mn = {0.f, 0.f, 0.f, 0.f}, cf = {0.f, 0.f, 0.f, 0.f};
    if constexpr (LPR < 64) {
        if (has_var) {
            cf = *reinterpret_cast<const f32x4*>(coef + l * 4);
            if (mean) mn = *reinterpret_cast<const f32x4*>(mean + l * 4);
        }
    }
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const int64_t row = r0 + sub;
        if (row >= rows) continue;
        for (int c = l * 4; c < C; c += LPR * 4) {
            f32x4 p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d + row * C + c));              // read exactly once
            if (has_scale) p = p * k.scale_at(c);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + row * x_pitch + c);
            const f32x4 v = pre_activation<LPR>(xv, k, has_scale, has_shift, c);
#pragma unroll
            for (int q = 0; q < 4; ++q) p[q] = v[q] > 0.f ? p[q] : 0.f;
            if (has_var) {
                if constexpr (LPR == 64) {
                    cf = *reinterpret_cast<const f32x4*>(coef + c);
                    if (mean) mn = *reinterpret_cast<const f32x4*>(mean + c);
                }
                p = p + (xv - mn) * cf;
            }
            f32x4* dst = reinterpret_cast<f32x4*>(g + row * g_pitch + c);
            if (accumulate) p = *dst + p;
            *dst = p;
        }
    }
}

// row blocks of the column reductions: a function of `rows` alone (see above); at most 1024 workgroups per channel tile
inline void col_plan(int64_t rows, int64_t* blocks, int64_t* rpb) {
    int64_t b = (rows + 127) / 128;
    if (b > 1024) b = 1024;
    *rpb = (rows + b - 1) / b;
    *blocks = (rows + *rpb - 1) / *rpb;
}

// lanes per row and grid of both kernels (the split bcos_channel_affine_rows uses)
inline int lanes_per_row(int C) {
    const int C4 = C / 4;
    return (C4 < 64 && 64 % C4 == 0) ? C4 : 64;
}

inline unsigned grid_for_rows(int64_t rows, int lpr) {
    const int64_t waves = (rows + (64 / lpr) - 1) / (64 / lpr);
    int64_t blocks = (waves + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return (unsigned)blocks;
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

#define BCOS_DENSE_DISPATCH(LAUNCH)     \
    switch (lpr) {                      \
        case 1: LAUNCH(1); break;       \
        case 2: LAUNCH(2); break;       \
        case 4: LAUNCH(4); break;       \
        case 8: LAUNCH(8); break;       \
        case 16: LAUNCH(16); break;     \
        case 32: LAUNCH(32); break;     \
        default: LAUNCH(64); break;     \
    }

extern "C" int bcos_slice_affine_rows(const float* x, int64_t x_pitch, const float* scale, const float* shift, const float* mul, float* y,
                                      int64_t y_pitch, uint32_t* y_absmax, int64_t rows, int C, int relu, void* stream) {
    if (!x || !y || rows <= 0 || C <= 0 || C % 4 != 0 || (relu != 0 && relu != 1))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_rows: NULL x / y, rows or C <= 0, C % 4 != 0 or relu outside {0, 1}");
    if (x_pitch == 0) x_pitch = C;
    if (y_pitch == 0) y_pitch = C;
    if (x_pitch < C || y_pitch < C || x_pitch % 4 != 0 || y_pitch % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_rows: a pitch must be 0 or a multiple of 4 that is >= C");
    if (misaligned(x) || misaligned(y) || misaligned(scale) || misaligned(shift) || misaligned(mul) || (reinterpret_cast<uintptr_t>(y_absmax) & 3))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_rows: tensors must be 16-byte aligned (y_absmax: 4-byte)");
    const int lpr = lanes_per_row(C);
    if (lpr == 64 && C > MAX_LDS_C) return bcos_set_error(BCOS_E_NOSUP, "bcos_slice_affine_rows: C > 8192");
    const size_t lds = lpr == 64 ? (size_t)2 * C * sizeof(float) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BCOS_SAR(L) hipLaunchKernelGGL(slice_affine_rows_kernel<L>, dim3(grid_for_rows(rows, lpr)), dim3(256), lds, st, x, x_pitch, scale, shift, \
                                       mul, y, y_pitch, y_absmax, rows, C, relu)
    BCOS_DENSE_DISPATCH(BCOS_SAR)
#undef BCOS_SAR
    return check_launch("slice_affine_rows launch");
}

extern "C" int bcos_slice_affine_bwd_acc(const float* d, const float* x, int64_t x_pitch, const float* scale, const float* shift, float* g,
                                         int64_t g_pitch, int64_t rows, int C, int relu, int accumulate, void* stream) {
    if (!d || !g || rows <= 0 || C <= 0 || C % 4 != 0 || (relu != 0 && relu != 1) || (accumulate != 0 && accumulate != 1))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_bwd_acc: NULL d / g, rows or C <= 0, C % 4 != 0, relu or accumulate outside {0, 1}");
    if (relu && !x) return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_bwd_acc: relu needs x (the gate is rebuilt from the forward's input)");
    if (x_pitch == 0) x_pitch = C;
    if (g_pitch == 0) g_pitch = C;
    if (x_pitch < C || g_pitch < C || x_pitch % 4 != 0 || g_pitch % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_bwd_acc: a pitch must be 0 or a multiple of 4 that is >= C");
    if (misaligned(d) || misaligned(x) || misaligned(g) || misaligned(scale) || misaligned(shift))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_affine_bwd_acc: tensors must be 16-byte aligned");
    const int lpr = lanes_per_row(C);
    if (lpr == 64 && C > MAX_LDS_C) return bcos_set_error(BCOS_E_NOSUP, "bcos_slice_affine_bwd_acc: C > 8192");
    const size_t lds = lpr == 64 ? (size_t)2 * C * sizeof(float) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BCOS_SAB(L) hipLaunchKernelGGL(slice_affine_bwd_acc_kernel<L>, dim3(grid_for_rows(rows, lpr)), dim3(256), lds, st, d, x, x_pitch, scale, \
                                       shift, g, g_pitch, rows, C, relu, accumulate)
    BCOS_DENSE_DISPATCH(BCOS_SAB)
#undef BCOS_SAB
    return check_launch("slice_affine_bwd_acc launch");
}

extern "C" int bcos_slice_col_ws_floats(int64_t rows, int C, int64_t* floats) {
    if (rows <= 0 || C <= 0 || C % 4 != 0 || !floats) return bcos_set_error(BCOS_E_INVAL, "bcos_slice_col_ws_floats: rows or C <= 0, C % 4 != 0 or NULL floats");
    int64_t blocks, rpb;
    col_plan(rows, &blocks, &rpb);
    *floats = blocks * 3 * C;
    return BCOS_OK;
}

extern "C" int bcos_slice_batch_stats(const float* x, int64_t x_pitch, float* mean, float* var, float* workspace, int64_t workspace_floats,
                                      int64_t rows, int C, void* stream) {
    if (!x || !mean || !var || !workspace || rows <= 0 || C <= 0 || C % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_batch_stats: NULL x / mean / var / workspace, rows or C <= 0 or C % 4 != 0");
    if (x_pitch == 0) x_pitch = C;
    if (x_pitch < C || x_pitch % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_batch_stats: a pitch must be 0 or a multiple of 4 that is >= C");
    if (misaligned(x) || misaligned(workspace) || (reinterpret_cast<uintptr_t>(mean) & 3) || (reinterpret_cast<uintptr_t>(var) & 3))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_batch_stats: x and workspace must be 16-byte aligned (mean, var: 4-byte)");
    int64_t blocks, rpb;
    col_plan(rows, &blocks, &rpb);
    if (workspace_floats < blocks * 3 * C) return bcos_set_error(BCOS_E_INVAL, "bcos_slice_batch_stats: workspace smaller than bcos_slice_col_ws_floats");
    const unsigned tiles = (unsigned)((C / 4 + CQ - 1) / CQ);
    if (tiles > 65535u) return bcos_set_error(BCOS_E_NOSUP, "bcos_slice_batch_stats: C > 2097120");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(slice_stats_partial_kernel, dim3((unsigned)blocks, tiles), dim3(256), 0, st, x, x_pitch, workspace, rows, C, rpb);
    hipLaunchKernelGGL(slice_stats_finish_kernel, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st, workspace, mean, var, (int)blocks, C, rows, rpb);
    return check_launch("slice_batch_stats launch");
}

extern "C" int bcos_bn_reader_finish(const float* var, const float* weight, float* running_var, float* rstd, float* g, int C, float eps,
                                     float momentum, void* stream) {
    if (!var || !rstd || !g || C <= 0 || !(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f))
        return bcos_set_error(BCOS_E_INVAL, "bcos_bn_reader_finish: NULL var / rstd / g, C <= 0, eps < 0 or momentum outside [0, 1]");
    if ((reinterpret_cast<uintptr_t>(var) & 3) || (reinterpret_cast<uintptr_t>(weight) & 3) || (reinterpret_cast<uintptr_t>(running_var) & 3) ||
        (reinterpret_cast<uintptr_t>(rstd) & 3) || (reinterpret_cast<uintptr_t>(g) & 3))
        return bcos_set_error(BCOS_E_INVAL, "bcos_bn_reader_finish: vectors must be 4-byte aligned");
    hipLaunchKernelGGL(bn_reader_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), var, weight,
                       running_var, rstd, g, C, eps, momentum);
    return check_launch("bn_reader_finish launch");
}

extern "C" int bcos_slice_relu_bwd_colsums(const float* d, const float* x, int64_t x_pitch, const float* gvec, const float* shift,
                                           const float* rstd, float* sgx, float* sg, float* gw, float* coef, float* workspace,
                                           int64_t workspace_floats, int64_t rows, int C, void* stream) {
    if (!d || !x || !gvec || !sgx || !workspace || rows <= 0 || C <= 0 || C % 4 != 0 || ((gw || coef) && !rstd))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_relu_bwd_colsums: NULL d / x / gvec / sgx / workspace, rows or C <= 0, C % 4 != 0, or gw / coef without rstd");
    if (x_pitch == 0) x_pitch = C;
    if (x_pitch < C || x_pitch % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_relu_bwd_colsums: a pitch must be 0 or a multiple of 4 that is >= C");
    if (misaligned(d) || misaligned(x) || misaligned(gvec) || misaligned(shift) || misaligned(workspace))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_relu_bwd_colsums: d, x, gvec, shift and workspace must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(rstd) & 3) || (reinterpret_cast<uintptr_t>(sgx) & 3) || (reinterpret_cast<uintptr_t>(sg) & 3) ||
        (reinterpret_cast<uintptr_t>(gw) & 3) || (reinterpret_cast<uintptr_t>(coef) & 3))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_relu_bwd_colsums: rstd, sgx, sg, gw and coef must be 4-byte aligned");
    int64_t blocks, rpb;
    col_plan(rows, &blocks, &rpb);
    if (workspace_floats < blocks * 2 * C) return bcos_set_error(BCOS_E_INVAL, "bcos_slice_relu_bwd_colsums: workspace smaller than bcos_slice_col_ws_floats");
    const unsigned tiles = (unsigned)((C / 4 + CQ - 1) / CQ);
    if (tiles > 65535u) return bcos_set_error(BCOS_E_NOSUP, "bcos_slice_relu_bwd_colsums: C > 2097120");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(slice_relu_bwd_colsums_kernel, dim3((unsigned)blocks, tiles), dim3(256), 0, st, d, x, x_pitch, gvec, shift, workspace, rows, C, rpb);
    hipLaunchKernelGGL(slice_bn_bwd_finish_kernel, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st, workspace, rstd, gvec, sgx, sg, gw, coef, (int)blocks, C,
                       rows);
    return check_launch("slice_relu_bwd_colsums launch");
}

extern "C" int bcos_slice_bn_bwd_acc(const float* d, const float* x, int64_t x_pitch, const float* scale, const float* shift, const float* mean,
                                     const float* coef, float* g, int64_t g_pitch, int64_t rows, int C, int accumulate, void* stream) {
    if (!d || !x || !g || rows <= 0 || C <= 0 || C % 4 != 0 || (accumulate != 0 && accumulate != 1) || (mean && !coef))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_bn_bwd_acc: NULL d / x / g, rows or C <= 0, C % 4 != 0, accumulate outside {0, 1} or mean without coef");
    if (x_pitch == 0) x_pitch = C;
    if (g_pitch == 0) g_pitch = C;
    if (x_pitch < C || g_pitch < C || x_pitch % 4 != 0 || g_pitch % 4 != 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_bn_bwd_acc: a pitch must be 0 or a multiple of 4 that is >= C");
    if (misaligned(d) || misaligned(x) || misaligned(g) || misaligned(scale) || misaligned(shift) || misaligned(mean) || misaligned(coef))
        return bcos_set_error(BCOS_E_INVAL, "bcos_slice_bn_bwd_acc: tensors must be 16-byte aligned");
    const int lpr = lanes_per_row(C);
    if (lpr == 64 && C > MAX_LDS_C) return bcos_set_error(BCOS_E_NOSUP, "bcos_slice_bn_bwd_acc: C > 8192");
    const size_t lds = lpr == 64 ? (size_t)2 * C * sizeof(float) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BCOS_SBB(L) hipLaunchKernelGGL(slice_bn_bwd_acc_kernel<L>, dim3(grid_for_rows(rows, lpr)), dim3(256), lds, st, d, x, x_pitch, scale, shift, \
                                       mean, coef, g, g_pitch, rows, C, accumulate)
    BCOS_DENSE_DISPATCH(BCOS_SBB)
#undef BCOS_SBB
    return check_launch("slice_bn_bwd_acc launch");
}
