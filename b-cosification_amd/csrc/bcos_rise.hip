// bcos_rise.hip -- the device side of the RISE baseline explainer (interpretability/explanation_methods/explainers/rise.py of the
// reference).  The reference keeps n upsampled, shifted random grids as float masks [n, 1, H, W] (rise.py:34-57), multiplies the image
// by all of them (rise.py:79) and reduces the class probabilities over the masks with one matrix product (rise.py:93-95).  A mask is an
// s x s bit grid and two shifts -- four int32 -- so the bank is [n, 4] and the mask values are evaluated where they are needed
// (bcos_rise_mask.h, the definition in include/bcos_hip.h):
//   bcos_rise_masks        the dense masks of a window of the bank (tests, and the module path of the explainer);
//   bcos_prep_input_rise   the PREPARED network input of n masked copies straight from the one source image;
//   bcos_rise_accumulate   out[t] = (sum_i scores[i, t] * m_i) / n / p1 in a fixed order, from scores that never left the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"
#include "bcos_rise_mask.h"      // (switches fp contraction off for this translation unit)

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ uint64_t grid_bits(const i32x4 r) { return (uint64_t)(uint32_t)r[0] | ((uint64_t)(uint32_t)r[1] << 32); }

// a shift the caller vouched for is still kept inside its cell: the upsampled position then stays below U
__device__ __forceinline__ int clamp_shift(int v, int cell) { return min(max(v, 0), cell - 1); }

// ---- dense masks of bank rows [first, first + n) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void rise_masks_kernel(const i32x4* __restrict__ bank, float* __restrict__ out, int n, int s, int HW,
                                                         int W, int cell_h, int cell_w) {
    const int64_t total = (int64_t)n * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    const int Uh = (s + 1) * cell_h, Uw = (s + 1) * cell_w;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / HW;
        const int hw = (int)(i - m * HW);
        const int h = hw / W, w = hw - h * W;
        const i32x4 r = bank[m];
        out[i] = rise_mask_value(grid_bits(r), s, rise_axis(h + clamp_shift(r[2], cell_h), s, Uh),
                                 rise_axis(w + clamp_shift(r[3], cell_w), s, Uw));
    }
}

// ---- prepared input of n masked copies of one 6-channel image ------------------------------------------------------------------------
// The shape of prep_input_occluded_kernel (bcos_occlusion.hip) and the arithmetic of prep_input_kernel: o = (v - mean) / std on
// v = x * m, ONE fp32 product per element (rise.py:79), so the bits are those of bcos_prep_input on the materialised copy.  A wavefront
// lies inside one copy except where a copy ends, so the bank row is fetched for the wavefront's first lane (a uniform address: a scalar
// load) and re-read per lane only by the wavefronts that straddle two copies.
__global__ __launch_bounds__(TPB) void prep_input_rise_kernel(const float* __restrict__ x, const i32x4* __restrict__ bank,
                                                              float* __restrict__ out, const float* __restrict__ mean6,
                                                              const float* __restrict__ std6, unsigned* __restrict__ absmax, int n, int s,
                                                              int HW, int W, int cell_h, int cell_w, int Cpad) {
    const int64_t total = (int64_t)n * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    const int Uh = (s + 1) * cell_h, Uw = (s + 1) * cell_w;
    float mu[6], sd[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { mu[c] = mean6[c]; sd[c] = std6[c]; }
    const bool wide = Cpad == 8 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const int m = (int)(i / HW);
        const int hw = (int)(i - (int64_t)m * HW);
        const int h = hw / W, w = hw - h * W;
        const int m_first = __builtin_amdgcn_readfirstlane(m);
        i32x4 r = bank[m_first];
        if (m != m_first) r = bank[m];
        const float mask = rise_mask_value(grid_bits(r), s, rise_axis(h + clamp_shift(r[2], cell_h), s, Uh),
                                           rise_axis(w + clamp_shift(r[3], cell_w), s, Uw));
        const float* src = x + hw;
        float* dst = out + i * Cpad;
        unsigned mx = 0u;
        float o[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float v = src[(int64_t)c * HW] * mask;
            o[c] = (v - mu[c]) / sd[c];
            mx = max(mx, __float_as_uint(o[c]) & 0x7fffffffu);
        }
        if (wide) {                                                             // the usual padded pixel: two 16-byte stores
            reinterpret_cast<f32x4*>(dst)[0] = f32x4{o[0], o[1], o[2], o[3]};
            reinterpret_cast<f32x4*>(dst)[1] = f32x4{o[4], o[5], 0.f, 0.f};
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) dst[c] = o[c];
            for (int c = 6; c < Cpad; ++c) dst[c] = 0.f;
        }
        if (absmax) absmax[i] = mx;         // per-pixel max |value| bit pattern, the convention of prep_input_kernel
    }
}

// ---- out[t] = (sum_i scores[i, t] * m_i) / n / p1 ---------------------------------------------------------------------------------------
// A workgroup owns a tile of ACC_TH x ACC_TW pixels (one pixel per thread; a wavefront covers 2 rows x 32 columns, so a store of one
// target is two full 128-byte lines) and a slice of TS targets.
//   tables   a mask shifts the tile by (shift_r, shift_c) inside one cell, so the tile meets ACC_TH + cell_h - 1 upsampled rows and
//            ACC_TW + cell_w - 1 columns in all: their axis records (two mirrored indices and the weight; the only integer and fp32
//            divisions of the kernel) go into LDS once per workgroup.
//   chunks   ACC_CH = 64 masks at a time, the chunk of the summation order: bank rows and the slice's scores are staged in LDS; every
//            thread walks the chunk in ascending i, evaluates m once per mask (two table reads, four bit tests, six flops) and adds the
//            TS separately rounded products to the chunk sums; the chunk sums are then added to the totals.  Both live in registers.
// Every output element is the chain the header fixes, whatever T, TS or the grid.
constexpr int ACC_TH = 8, ACC_TW = 32, ACC_CH = 64;
constexpr int ACC_TABLE_MAX = 3584;                // axis records of both tables (8 bytes each): 28 KiB + 3 KiB of staging

struct AxisRec {
    int k;                                          // index pair: k0 | k1 << 8 (rows: already multiplied by s)
    float f;
};

template <int TS>
__global__ __launch_bounds__(TPB) void rise_accumulate_kernel(const float* __restrict__ scores, const i32x4* __restrict__ bank,
                                                              float* __restrict__ out, int n, int T, int s, int H, int W, int cell_h,
                                                              int cell_w, float fn, float p1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    i32x4* s_bank = reinterpret_cast<i32x4*>(smem);                                       // [ACC_CH]
    float* s_sc = reinterpret_cast<float*>(smem + ACC_CH * 16);                           // [ACC_CH][TS]
    AxisRec* s_row = reinterpret_cast<AxisRec*>(smem + ACC_CH * 16 + ACC_CH * 8 * 4);     // [ACC_TH + cell_h - 1]
    const int nrow = ACC_TH + cell_h - 1, ncol = ACC_TW + cell_w - 1;
    AxisRec* s_col = s_row + nrow;                                                        // [ACC_TW + cell_w - 1]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int th0 = blockIdx.y * ACC_TH, tw0 = blockIdx.x * ACC_TW;
    const int lr = wave * 2 + (lane >> 5), lc = lane & 31;
    const int h = th0 + lr, w = tw0 + lc;
    const bool live = h < H && w < W;
    const int t0 = blockIdx.z * TS;
    const int nt = min(TS, T - t0);

    // (positions of the tile's pixels beyond the image are clamped to the last one a mask can reach: p < U always)
    for (int j = tid; j < nrow; j += TPB) {
        const RiseAxis a = rise_axis(min(th0 + j, H + cell_h - 2), s, (s + 1) * cell_h);
        s_row[j] = AxisRec{(a.k0 * s) | ((a.k1 * s) << 8), a.f};
    }
    for (int j = tid; j < ncol; j += TPB) {
        const RiseAxis a = rise_axis(min(tw0 + j, W + cell_w - 2), s, (s + 1) * cell_w);
        s_col[j] = AxisRec{a.k0 | (a.k1 << 8), a.f};
    }

    float tot[TS];
#pragma unroll
    for (int k = 0; k < TS; ++k) tot[k] = 0.f;
    for (int base = 0; base < n; base += ACC_CH) {
        const int cnt = min(ACC_CH, n - base);
        __syncthreads();                                           // the tables are written; the previous chunk is consumed
        if (tid < cnt) s_bank[tid] = bank[base + tid];
        for (int e = tid; e < cnt * TS; e += TPB) {
            const int i = e / TS, k = e - i * TS;
            s_sc[e] = k < nt ? scores[(int64_t)(base + i) * T + t0 + k] : 0.f;
        }
        __syncthreads();
        float acc[TS];
#pragma unroll
        for (int k = 0; k < TS; ++k) acc[k] = 0.f;
        for (int i = 0; i < cnt; ++i) {
            const i32x4 b = s_bank[i];
            const AxisRec rr = s_row[lr + clamp_shift(b[2], cell_h)];
            const AxisRec cc = s_col[lc + clamp_shift(b[3], cell_w)];
            const float m = rise_blend(grid_bits(b), rr.k & 255, rr.k >> 8, rr.f, cc.k & 255, cc.k >> 8, cc.f);
#pragma unroll
            for (int k = 0; k < TS; ++k) {
                const float prod = s_sc[i * TS + k] * m;           // rounded on its own (no contraction in this file)
                acc[k] += prod;
            }
        }
#pragma unroll
        for (int k = 0; k < TS; ++k) tot[k] += acc[k];
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < TS; ++k)
            if (k < nt) out[((int64_t)(t0 + k) * H + h) * W + w] = tot[k] / fn / p1;
    }
}

// what the three entry points share: 2 <= s <= 8 and image sizes whose upsampled extent 2 U stays below 2^24
inline const char* check_geometry(int s, int H, int W, int* cell_h, int* cell_w) {
    if (s < 2 || s > 8) return "s must be in 2..8";
    if (H <= 0 || W <= 0) return "H and W must be positive";
    if ((int64_t)H * W > INT32_MAX) return "H * W exceeds 2^31 - 1";
    *cell_h = (H + s - 1) / s;
    *cell_w = (W + s - 1) / s;
    if (2 * (int64_t)(s + 1) * *cell_h >= (1 << 24) || 2 * (int64_t)(s + 1) * *cell_w >= (1 << 24))
        return "an image side whose upsampled extent 2 (s + 1) ceil(size / s) reaches 2^24";
    return nullptr;
}

inline int fail(const char* who, const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return bcos_set_error(BCOS_E_INVAL, msg);
}

}  // namespace

extern "C" int bcos_rise_masks(const int32_t* bank, float* out, int n_bank, int first, int n, int s, int H, int W, void* stream) {
    static const char* who = "bcos_rise_masks";
    if (!bank || !out) return fail(who, "NULL pointer");
    int cell_h = 0, cell_w = 0;
    if (const char* why = check_geometry(s, H, W, &cell_h, &cell_w)) return fail(who, why);
    if (n_bank <= 0 || first < 0 || n <= 0 || (int64_t)first + n > n_bank) return fail(who, "rows [first, first + n) leave the bank");
    if (reinterpret_cast<uintptr_t>(bank) & 15) return fail(who, "bank must be 16-byte aligned");
    if ((int64_t)n > INT64_MAX / ((int64_t)H * W)) return fail(who, "n * H * W overflows");
    const int64_t total = (int64_t)n * H * W;
    int64_t blocks = (total + TPB - 1) / TPB;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(rise_masks_kernel, dim3((unsigned)blocks), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const i32x4*>(bank) + first, out, n, s, H * W, W, cell_h, cell_w);
    return check_launch("rise_masks_kernel");
}

extern "C" int bcos_prep_input_rise(const float* x, const int32_t* bank, float* out, const float* mean6, const float* std6,
                                    uint32_t* absmax_out, int n_bank, int first, int n, int s, int Cx, int H, int W, int Cpad,
                                    int add_inverse, void* stream) {
    static const char* who = "bcos_prep_input_rise";
    if (!x || !bank || !out || !mean6 || !std6) return fail(who, "NULL pointer");
    int cell_h = 0, cell_w = 0;
    if (const char* why = check_geometry(s, H, W, &cell_h, &cell_w)) return fail(who, why);
    if (n_bank <= 0 || first < 0 || n <= 0 || (int64_t)first + n > n_bank) return fail(who, "copies [first, first + n) leave the bank");
    if (add_inverse || Cx != 6) return fail(who, "only the 6-channel input (masking before AddInverse is another operator)");
    if (Cpad < 6) return fail(who, "Cpad < 6");
    if ((int64_t)n > INT64_MAX / ((int64_t)H * W) / Cpad) return fail(who, "n * H * W * Cpad overflows");
    if (reinterpret_cast<uintptr_t>(bank) & 15) return fail(who, "bank must be 16-byte aligned");
    const int64_t total = (int64_t)n * H * W;
    int64_t blocks = (total + TPB - 1) / TPB;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(prep_input_rise_kernel, dim3((unsigned)blocks), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), x,
                       reinterpret_cast<const i32x4*>(bank) + first, out, mean6, std6, absmax_out, n, s, H * W, W, cell_h, cell_w, Cpad);
    return check_launch("prep_input_rise_kernel");
}

extern "C" int bcos_rise_accumulate(const float* scores, const int32_t* bank, const int32_t* bank_host, float* out, int n, int T, int s,
                                    int H, int W, float p1, void* stream) {
    static const char* who = "bcos_rise_accumulate";
    if (!scores || !bank || !out) return fail(who, "NULL pointer");
    if (n <= 0 || T <= 0) return fail(who, "n and T must be positive");
    int cell_h = 0, cell_w = 0;
    if (const char* why = check_geometry(s, H, W, &cell_h, &cell_w)) return fail(who, why);
    if (!(p1 > 0.f) || !(p1 <= 3.0e38f)) return fail(who, "p1 must be positive and finite");
    if (reinterpret_cast<uintptr_t>(bank) & 15) return fail(who, "bank must be 16-byte aligned");
    // (H * W <= 2^31 - 1 and n, T <= 2^31 - 1: T * H * W and n * T fit 64-bit offsets)
    if (bank_host) {
        const uint64_t above = s == 8 ? 0ull : ~0ull << (s * s);
        for (int i = 0; i < n; ++i) {
            const int32_t* r = bank_host + 4 * (int64_t)i;
            const uint64_t bits = (uint64_t)(uint32_t)r[0] | ((uint64_t)(uint32_t)r[1] << 32);
            if (bits & above) return fail(who, "a bank row with grid bits set at or above s * s");
            if (r[2] < 0 || r[2] >= cell_h || r[3] < 0 || r[3] >= cell_w) return fail(who, "a bank row whose shift leaves its cell");
        }
    }
    const int tiles_w = (W + ACC_TW - 1) / ACC_TW, tiles_h = (H + ACC_TH - 1) / ACC_TH;
    const int nrec = ACC_TH + cell_h - 1 + ACC_TW + cell_w - 1;
    if (tiles_h > 65535 || nrec > ACC_TABLE_MAX)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_rise_accumulate: H exceeds 65535 * 8, or ceil(H / s) + ceil(W / s) exceeds 3546 (the axis tables are held in LDS)");
    const int TS = T == 1 ? 1 : T <= 4 ? 4 : 8;                    // targets per workgroup; the bits do not depend on it
    const int slices = (T + TS - 1) / TS;
    if (slices > 65535) return bcos_set_error(BCOS_E_NOSUP, "bcos_rise_accumulate: T exceeds 65535 * 8");
    const size_t lds = ACC_CH * 16 + ACC_CH * 8 * 4 + (size_t)nrec * sizeof(AxisRec);
    const dim3 grid((unsigned)tiles_w, (unsigned)tiles_h, (unsigned)slices);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const i32x4* b4 = reinterpret_cast<const i32x4*>(bank);
    const float fn = (float)n;
    if (TS == 1) hipLaunchKernelGGL(rise_accumulate_kernel<1>, grid, dim3(TPB), lds, st, scores, b4, out, n, T, s, H, W, cell_h, cell_w, fn, p1);
    else if (TS == 4) hipLaunchKernelGGL(rise_accumulate_kernel<4>, grid, dim3(TPB), lds, st, scores, b4, out, n, T, s, H, W, cell_h, cell_w, fn, p1);
    else hipLaunchKernelGGL(rise_accumulate_kernel<8>, grid, dim3(TPB), lds, st, scores, b4, out, n, T, s, H, W, cell_h, cell_w, fn, p1);
    return check_launch("rise_accumulate_kernel");
}
