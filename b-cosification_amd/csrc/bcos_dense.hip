// bcos_dense.hip -- the two streaming kernels a densely connected (DenseNet) plan needs around the contraction kernels: the
// pre-activation BatchNormUncentered + ReLU a dense layer / transition / head applies to a channel SLICE of the block's concatenated
// feature buffer (torchvision _DenseLayer: norm1 -> relu1 -> conv1 over cat(features); reference standard_models.py:56-63,
// batchnorm_uncentered.py:46-60), and its input gradient accumulated into the same slice of the block's gradient buffer.
// Both walk rows of C floats inside rows of `pitch` floats with 16-byte accesses; a wavefront owns whole rows (C / 4 lanes per row
// where that divides 64, otherwise 64 lanes looping over the row), so the row maximum is a cross-lane reduction without atomics.
// Per-channel constants sit in registers (a lane keeps its channel quad for every row) or in LDS (looping form).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"

// x * scale + shift is TWO roundings here, as in bcos_channel_affine_rows (bcos_train.hip), whose bits bcos_slice_affine_rows must
// reproduce; and the gate of the backward kernel is decided on exactly the value the forward kernel compared with zero.
#pragma clang fp contract(off)

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int MAX_LDS_C = 8192;            // scale + shift of the looping form: 2 x 32 KiB of dynamic LDS at most

inline int check_launch(const char* what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error(what, err);
    return BCOS_OK;
}

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
