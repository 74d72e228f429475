// bcos_head.hip -- the start of the explanation pass for a LINEAR FUNCTIONAL of the logits, f = sum_k c_k y_k.  In explanation mode the
// network is linear in the head cotangent (scales, gates and variances are detached, the LogitLayer bias is a constant:
// bcos/common.py:163-181), so W_f(x) = sum_k c_k W_k(x) and only the first launch of the pass knows about the functional:
//   bcos_head_rankm_grad      the sparse form (at most 8 classes per image): bcos_head_rank1_grad_ex with a short sum of weight rows --
//                             contrastive explanations y_a - y_b, any few-term functional;
//   bcos_head_cotangent_grad  the dense form: bcos_head_onehot_grad with a cotangent row per image instead of a one-hot one -- the
//                             mean-corrected explanation y_t - mean_k y_k (interpretability/explanation_methods/explainers/ours.py:28-33).
// Both are streaming kernels: one wavefront per row, 16-byte accesses, row maxima for the f16x2 contraction that reads the result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int MAX_TERMS = 8;                 // include/bcos_hip.h: 1 <= J <= 8
constexpr int64_t MAX_HEAD_BLOCKS = 16384;   // (the grid of head_rank1_kernel, bcos_elementwise.hip)

// v[n, r, :] = sum_j a_j * w[cls[n, j], :],  a_j = ((coef * scale[n, r, cls[n, j]]) * row_scale[n r]) * c[n, j]  -- the factors of
// head_rank1_kernel in its order, the functional's coefficient last, so that J = 1 with c = 1 gives its bits.  The sum is ONE fp32 chain in
// ascending j of separately rounded products (no fused multiply-add: the documented value does not depend on the compiler's contraction).
// A wave owns a row: the J scale values of the row are read once, the J weight rows (at most 8 x D floats, shared by every row of the
// image) come out of L2; the J loads of a column are issued together before the chain consumes them.
template <int J>
__global__ __launch_bounds__(256) void head_rankm_kernel(const int64_t* __restrict__ cls, const float* __restrict__ cf,
                                                         const float* __restrict__ scale, const float* __restrict__ w,
                                                         const float* __restrict__ row_scale, const float* __restrict__ mul,
                                                         const float* __restrict__ mul2, const float* __restrict__ gate2,
                                                         float* __restrict__ out, float* __restrict__ out2, unsigned* __restrict__ out_absmax,
                                                         unsigned* __restrict__ out2_absmax, int64_t rows, int R, int K, int D4, float coef,
                                                         int gate_from_mul) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave; row < rows; row += nwaves) {
        const int64_t n = row / R;
        float a[J];
        const f32x4* wr[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            // a class outside [0, K) contributes nothing and is never used as an index (the host validates user-given classes --
            // bcos_hip/ops.py: check_functional_classes --, this keeps a raw C-ABI caller off out-of-range reads)
            const int64_t kc = cls[n * J + j];
            const bool k_ok = kc >= 0 && kc < (int64_t)K;
            const int k = k_ok ? (int)kc : 0;
            float aj = k_ok ? coef * scale[row * K + k] : 0.f;
            if (row_scale) aj *= row_scale[row];
            a[j] = aj * cf[n * J + j];
            wr[j] = reinterpret_cast<const f32x4*>(w + (int64_t)k * D4 * 4);
        }
        unsigned mx = 0u, mx2 = 0u;
        for (int d = lane; d < D4; d += 64) {
            const int64_t i = row * D4 + d;
            f32x4 wv[J];
#pragma unroll
            for (int j = 0; j < J; ++j) wv[j] = wr[j][d];
            f32x4 v = wv[0] * a[0];
#pragma unroll
            for (int j = 1; j < J; ++j) v += wv[j] * a[j];
            f32x4 o = v, m = {0.f, 0.f, 0.f, 0.f};
            if (mul) { m = reinterpret_cast<const f32x4*>(mul)[i]; o *= m; }
            reinterpret_cast<f32x4*>(out)[i] = o;
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = max(mx, __float_as_uint(o[q]) & 0x7fffffffu);
            if (out2) {                      // the second output of the gradient epilogue (bcos_epilogue.out2): v [* mul2] [gated]
                f32x4 o2 = v;
                if (mul2) o2 *= reinterpret_cast<const f32x4*>(mul2)[i];
                if (gate_from_mul) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) o2[q] = (__float_as_uint(m[q]) & 1u) ? o2[q] : 0.f;
                } else if (gate2) {
                    const f32x4 gt = reinterpret_cast<const f32x4*>(gate2)[i];
#pragma unroll
                    for (int q = 0; q < 4; ++q) o2[q] = gt[q] > 0.f ? o2[q] : 0.f;
                }
                reinterpret_cast<f32x4*>(out2)[i] = o2;
#pragma unroll
                for (int q = 0; q < 4; ++q) mx2 = max(mx2, __float_as_uint(o2[q]) & 0x7fffffffu);
            }
        }
        if (out_absmax || out2_absmax) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
                mx2 = max(mx2, (unsigned)__shfl_xor((int)mx2, o));
            }
            if (lane == 0 && out_absmax) out_absmax[row] = mx;
            if (lane == 0 && out2_absmax) out2_absmax[row] = mx2;
        }
    }
}

// glin[n, r, k] = (cot[n, k] * scale[n, r, k]) * coef for k < K, zero in the pad columns K .. Kp - 1 (Kp = K rounded up to 4); per-row
// max |glin|.  One wavefront per row: one read of scale, one 16-byte write of glin (the rows of glin are Kp floats apart and always
// aligned); the cotangent row of the image comes out of L2.  VEC: K % 4 == 0 and aligned scale / cot -- 16-byte reads as well.
template <bool VEC>
__global__ __launch_bounds__(256) void head_cotangent_kernel(const float* __restrict__ cot, const float* __restrict__ scale,
                                                             float* __restrict__ glin, unsigned* __restrict__ out_absmax, int64_t rows,
                                                             int R, int K, int Kp4, float coef) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave; row < rows; row += nwaves) {
        const int64_t n = row / R;
        const float* sr = scale + row * K;
        const float* cr = cot + n * K;
        unsigned mx = 0u;
        for (int c4 = lane; c4 < Kp4; c4 += 64) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                s = reinterpret_cast<const f32x4*>(sr)[c4];
                c = reinterpret_cast<const f32x4*>(cr)[c4];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = c4 * 4 + q;
                    if (k < K) { s[q] = sr[k]; c[q] = cr[k]; }
                }
            }
            const f32x4 g = (c * s) * coef;
            reinterpret_cast<f32x4*>(glin)[row * Kp4 + c4] = g;
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = max(mx, __float_as_uint(g[q]) & 0x7fffffffu);
        }
        if (out_absmax) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
            if (lane == 0) out_absmax[row] = mx;
        }
    }
}

inline unsigned head_grid(int64_t rows) {
    int64_t blocks = (rows + 3) / 4;
    if (blocks > MAX_HEAD_BLOCKS) blocks = MAX_HEAD_BLOCKS;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int bcos_head_rankm_grad(const int64_t* cls, const float* coef, int J, const float* scale, const float* w, const float* row_scale,
                                    const float* mul, const float* mul2, const float* gate2, int gate2_from_mul, float* out, float* out2,
                                    uint32_t* out_absmax, uint32_t* out2_absmax, int N, int R, int K, int D, float inv_temperature,
                                    void* stream) {
    if (!cls || !coef || !scale || !w || !out) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: NULL cls / coef / scale / w / out");
    if (N <= 0 || R <= 0 || K <= 0 || D <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: N, R, K and D must be positive");
    if (D % 4 != 0) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: D must be a multiple of 4");
    if (J < 1) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: J must be at least 1");
    if (J > MAX_TERMS)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_head_rankm_grad: more than 8 terms per image (use bcos_head_cotangent_grad, the dense form)");
    if ((mul2 || gate2 || gate2_from_mul || out2_absmax) && !out2)
        return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: mul2 / gate2 / out2_absmax belong to out2");
    if (gate2_from_mul && (!mul || gate2)) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: gate2_from_mul needs mul and excludes gate2");
    if (misaligned16(w) || misaligned16(mul) || misaligned16(mul2) || misaligned16(gate2) || misaligned16(out) || misaligned16(out2))
        return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: tensors must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(cls) & 7) || (reinterpret_cast<uintptr_t>(coef) & 3))
        return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: cls / coef must be aligned to their element size");
    const int64_t rows = (int64_t)N * R;
    if (rows > INT64_MAX / K || rows > INT64_MAX / D) return bcos_set_error(BCOS_E_INVAL, "bcos_head_rankm_grad: N * R * K or N * R * D overflows");
    const float c = inv_temperature / (float)R;
    const int gfm = gate2_from_mul ? 1 : 0;
#define BCOS_RANKM_CASE(JJ)                                                                                                              \
    case JJ:                                                                                                                             \
        hipLaunchKernelGGL(head_rankm_kernel<JJ>, dim3(head_grid(rows)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cls, coef, \
                           scale, w, row_scale, mul, mul2, gate2, out, out2, out_absmax, out2_absmax, rows, R, K, D / 4, c, gfm);       \
        break;
    switch (J) {
        BCOS_RANKM_CASE(1) BCOS_RANKM_CASE(2) BCOS_RANKM_CASE(3) BCOS_RANKM_CASE(4)
        BCOS_RANKM_CASE(5) BCOS_RANKM_CASE(6) BCOS_RANKM_CASE(7) BCOS_RANKM_CASE(8)
    }
#undef BCOS_RANKM_CASE
    return check_launch("head_rankm_kernel");
}

extern "C" int bcos_head_cotangent_grad(const float* cot, const float* scale, float* glin, uint32_t* out_absmax, int N, int R, int K,
                                        float inv_temperature, void* stream) {
    if (!cot || !scale || !glin) return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: NULL cot / scale / glin");
    if (N <= 0 || R <= 0 || K <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: N, R and K must be positive");
    if (K > INT32_MAX - 3) return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: K exceeds 2^31 - 4");
    if (misaligned16(glin)) return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: glin must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(cot) | reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(out_absmax)) & 3)
        return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: cot / scale / out_absmax must be 4-byte aligned");
    const int64_t rows = (int64_t)N * R;
    const int Kp4 = (K + 3) / 4;
    if (rows > INT64_MAX / ((int64_t)Kp4 * 4)) return bcos_set_error(BCOS_E_INVAL, "bcos_head_cotangent_grad: N * R * Kp overflows");
    const float c = inv_temperature / (float)R;
    const bool vec = K % 4 == 0 && !misaligned16(cot) && !misaligned16(scale);
    if (vec)
        hipLaunchKernelGGL(head_cotangent_kernel<true>, dim3(head_grid(rows)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cot, scale,
                           glin, out_absmax, rows, R, K, Kp4, c);
    else
        hipLaunchKernelGGL(head_cotangent_kernel<false>, dim3(head_grid(rows)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cot, scale,
                           glin, out_absmax, rows, R, K, Kp4, c);
    return check_launch("head_cotangent_kernel");
}
