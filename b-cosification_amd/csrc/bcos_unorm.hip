// bcos_unorm.hip -- the uncentered position / group norms of the B-cos v2 norm ablations on gfx950
// (bcos/modules/norms/uncentered_norms/posnorm_uncentered.py:39-58, groupnorm_uncentered.py:21-61): the variance is the CENTRED second
// moment, but the value that is divided is x itself, not x - mean:
//     m = mean_S x,  var = mean_S (x - m)^2,  r = 1 / sqrt(var + eps),  y = w x r + b
//     explanation mode (var a constant):   gx = h r,                                   h = gy w
//     training mode:                       gx = r h - r^3 (x - m) (sum_S h x) / n
// Row form (S = a row of x [rows, D]: a pixel's channels on the NHWC image): one wavefront per row, the twins of layernorm_*_kernel in
// bcos_vit.hip.  Group form (S = an (image, group) of x [N, HW, C]): one workgroup per (image, group), the twins of groupnorm_*_kernel.
// Two-pass variance everywhere (mean, then centred squares), butterfly / fixed-order reductions, no atomics, no scratch: a call repeated
// gives the same bits, and no output depends on which optional outputs were requested.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <initializer_list>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int TPB = 256;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

// ---- row form -----------------------------------------------------------------------------------------------------------------------
// VEC: rows of up to 256 floats (D % 4 == 0, 16-byte aligned tensors) live in ONE float4 per lane -- read once, written once, 16-byte
// accesses.  Other widths and misaligned views take the strided loop.
template <bool VEC>
__global__ __launch_bounds__(TPB) void unorm_rows_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, float* __restrict__ y,
                                                             float* __restrict__ rstd_out, int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    if constexpr (VEC) {
        const bool on = lane * 4 < D;
        f32x4 wv = {1.f, 1.f, 1.f, 1.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if (on && w) wv = *reinterpret_cast<const f32x4*>(w + lane * 4);
        if (on && b) bv = *reinterpret_cast<const f32x4*>(b + lane * 4);
        for (int64_t r = wave; r < rows; r += nwaves) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (on) v = *reinterpret_cast<const f32x4*>(x + r * D + lane * 4);
            const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)D;
            f32x4 d = v - mean;
            if (!on) d = f32x4{0.f, 0.f, 0.f, 0.f};
            const float var = wave_sum(fmaf(d[0], d[0], d[1] * d[1]) + fmaf(d[2], d[2], d[3] * d[3])) / (float)D;
            const float sd = sqrtf(var + eps);
            f32x4 o = {v[0] / sd, v[1] / sd, v[2] / sd, v[3] / sd};        // the value itself, not d
            o = o * wv + bv;
            if (on) *reinterpret_cast<f32x4*>(y + r * D + lane * 4) = o;
            if (rstd_out && lane == 0) rstd_out[r] = 1.0f / sd;
        }
    } else {
        for (int64_t r = wave; r < rows; r += nwaves) {
            const float* src = x + r * D;
            float s = 0.f;
            for (int c = lane; c < D; c += 64) s += src[c];
            const float mean = wave_sum(s) / (float)D;
            float v = 0.f;
            for (int c = lane; c < D; c += 64) { const float d = src[c] - mean; v = fmaf(d, d, v); }
            const float var = wave_sum(v) / (float)D;
            const float sd = sqrtf(var + eps);
            float* dst = y + r * D;
            for (int c = lane; c < D; c += 64) {
                float o = src[c] / sd;
                if (w) o *= w[c];
                if (b) o += b[c];
                dst[c] = o;
            }
            if (rstd_out && lane == 0) rstd_out[r] = 1.0f / sd;
        }
    }
}

// explanation mode: the variance is a constant and nothing else of y depends on the row, so the gradient is elementwise:
//   out = gy w rstd (+ addend);  out2 = out * mul2 (the scale of the B-cos layer that produced x).  No reduction at all -- the centred
// twin subtracts mean(h).
template <bool VEC>
__global__ __launch_bounds__(TPB) void unorm_rows_bwd_detached_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                                      const float* __restrict__ rstd, const float* __restrict__ addend,
                                                                      const float* __restrict__ mul2, float* __restrict__ out,
                                                                      float* __restrict__ out2, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    if constexpr (VEC) {
        const bool on = lane * 4 < D;
        if (!on) return;                                    // (no wavefront reduction below: idle lanes may leave)
        f32x4 wv = {1.f, 1.f, 1.f, 1.f};
        if (w) wv = *reinterpret_cast<const f32x4*>(w + lane * 4);
        for (int64_t r = wave; r < rows; r += nwaves) {
            const int64_t off = r * D + lane * 4;
            f32x4 ad = {0.f, 0.f, 0.f, 0.f}, m2 = {1.f, 1.f, 1.f, 1.f};
            const f32x4 g = *reinterpret_cast<const f32x4*>(gy + off);
            if (addend) ad = *reinterpret_cast<const f32x4*>(addend + off);
            if (mul2) m2 = *reinterpret_cast<const f32x4*>(mul2 + off);
            const f32x4 o = g * wv * rstd[r] + ad;
            const f32x4 o2 = o * m2;
            if (out) *reinterpret_cast<f32x4*>(out + off) = o;
            if (out2) *reinterpret_cast<f32x4*>(out2 + off) = o2;
        }
    } else {
        for (int64_t r = wave; r < rows; r += nwaves) {
            const float rs = rstd[r];
            for (int c = lane; c < D; c += 64) {
                const int64_t i = r * D + c;
                float o = gy[i] * (w ? w[c] : 1.f) * rs;
                if (addend) o += addend[i];
                if (out) out[i] = o;
                if (out2) out2[i] = mul2 ? o * mul2[i] : o;
            }
        }
    }
}

// training mode: gx = rs h - rs^3 (x - mean) (sum h x) / n (+ addend), h = gy w; xr = x rs is written out for the weight gradient
// (sum_rows gy xr, a column reduction).  The mean is recomputed from the row.
template <bool VEC>
__global__ __launch_bounds__(TPB) void unorm_rows_bwd_full_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                  const float* __restrict__ w, const float* __restrict__ rstd,
                                                                  const float* __restrict__ addend, float* __restrict__ gx,
                                                                  float* __restrict__ xr, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    if constexpr (VEC) {
        const bool on = lane * 4 < D;
        f32x4 wv = {1.f, 1.f, 1.f, 1.f};
        if (on && w) wv = *reinterpret_cast<const f32x4*>(w + lane * 4);
        for (int64_t r = wave; r < rows; r += nwaves) {
            const int64_t off = r * D + lane * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f}, ad = {0.f, 0.f, 0.f, 0.f};
            if (on) v = *reinterpret_cast<const f32x4*>(x + off);
            if (on) g = *reinterpret_cast<const f32x4*>(gy + off);
            if (on && addend) ad = *reinterpret_cast<const f32x4*>(addend + off);
            const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)D;
            const f32x4 h = g * wv;
            const float shx = wave_sum(fmaf(h[0], v[0], h[1] * v[1]) + fmaf(h[2], v[2], h[3] * v[3]));
            const float rs = rstd[r];
            const float coef = rs * rs * rs * (shx / (float)D);
            const f32x4 o = rs * h - coef * (v - mean) + ad;
            if (on) *reinterpret_cast<f32x4*>(gx + off) = o;
            if (on && xr) *reinterpret_cast<f32x4*>(xr + off) = v * rs;
        }
    } else {
        for (int64_t r = wave; r < rows; r += nwaves) {
            const float* xs = x + r * D;
            const float* gs = gy + r * D;
            float s = 0.f, shx = 0.f;
            for (int c = lane; c < D; c += 64) {
                s += xs[c];
                shx = fmaf(gs[c] * (w ? w[c] : 1.0f), xs[c], shx);
            }
            const float mean = wave_sum(s) / (float)D;
            const float rs = rstd[r];
            const float coef = rs * rs * rs * (wave_sum(shx) / (float)D);
            for (int c = lane; c < D; c += 64) {
                const float h = gs[c] * (w ? w[c] : 1.0f);
                const float g = rs * h - coef * (xs[c] - mean);
                gx[r * D + c] = addend ? g + addend[r * D + c] : g;
                if (xr) xr[r * D + c] = xs[c] * rs;
            }
        }
    }
}

inline unsigned grid_rows(int64_t rows) {
    int64_t b = (rows * 64 + TPB - 1) / TPB;
    if (b < 1) b = 1;
    if (b > 256 * 8) b = 256 * 8;
    return (unsigned)b;
}

// ---- group form on NHWC tensors: one workgroup per (image, group) ---------------------------------------------------------------------
// Group g owns the channels [g cg, (g + 1) cg) of every pixel.  The passes over the group's HW x cg values (mean, centred squares,
// normalise) re-read it from L2: the group of one image is at most a few MB.
__device__ inline float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int k = 0; k < TPB / 64; ++k) t += red[k];
    return t;
}

__global__ __launch_bounds__(TPB) void unorm_group_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ y,
                                                              float* __restrict__ rstd_out, int HW, int C, int G, float eps) {
    __shared__ float red[TPB / 64];
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cg = C / G;
    const int64_t base = (int64_t)n * HW * C + g * cg;
    const int64_t m = (int64_t)HW * cg;
    float s = 0.f;
    for (int64_t e = threadIdx.x; e < m; e += TPB) s += x[base + (e / cg) * C + e % cg];
    const float mean = block_sum(s, red) / (float)m;
    float v = 0.f;
    for (int64_t e = threadIdx.x; e < m; e += TPB) { const float d = x[base + (e / cg) * C + e % cg] - mean; v = fmaf(d, d, v); }
    const float var = block_sum(v, red) / (float)m;
    const float sd = sqrtf(var + eps);
    for (int64_t e = threadIdx.x; e < m; e += TPB) {
        const int c = (int)(e % cg);
        const int64_t i = base + (e / cg) * C + c;
        float o = x[i] / sd;
        if (w) o *= w[g * cg + c];
        if (b) o += b[g * cg + c];
        y[i] = o;
    }
    if (rstd_out && threadIdx.x == 0) rstd_out[blockIdx.x] = 1.0f / sd;
}

// explanation mode: gx = gy w rstd, elementwise
__global__ __launch_bounds__(TPB) void unorm_group_bwd_detached_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                                       const float* __restrict__ rstd, float* __restrict__ gx,
                                                                       int HW, int C, int G) {
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cg = C / G;
    const int64_t base = (int64_t)n * HW * C + g * cg;
    const int64_t m = (int64_t)HW * cg;
    const float rs = rstd[blockIdx.x];
    for (int64_t e = threadIdx.x; e < m; e += TPB) {
        const int c = (int)(e % cg);
        const int64_t i = base + (e / cg) * C + c;
        gx[i] = gy[i] * (w ? w[g * cg + c] : 1.0f) * rs;
    }
}

// training mode: per (image, group) with m values, gx = rs h - rs^3 (x - mean) (sum h x) / m; xr = x rs for the weight gradient
__global__ __launch_bounds__(TPB) void unorm_group_bwd_full_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                   const float* __restrict__ w, const float* __restrict__ rstd,
                                                                   float* __restrict__ gx, float* __restrict__ xr, int HW, int C, int G) {
    __shared__ float red[TPB / 64];
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cg = C / G;
    const int64_t base = (int64_t)n * HW * C + g * cg;
    const int64_t m = (int64_t)HW * cg;
    const float rs = rstd[blockIdx.x];
    float s = 0.f, shx = 0.f;
    for (int64_t e = threadIdx.x; e < m; e += TPB) {
        const int c = (int)(e % cg);
        const int64_t i = base + (e / cg) * C + c;
        s += x[i];
        shx = fmaf(gy[i] * (w ? w[g * cg + c] : 1.0f), x[i], shx);
    }
    const float mean = block_sum(s, red) / (float)m;
    const float coef = rs * rs * rs * (block_sum(shx, red) / (float)m);
    for (int64_t e = threadIdx.x; e < m; e += TPB) {
        const int c = (int)(e % cg);
        const int64_t i = base + (e / cg) * C + c;
        const float h = gy[i] * (w ? w[g * cg + c] : 1.0f);
        gx[i] = rs * h - coef * (x[i] - mean);
        if (xr) xr[i] = x[i] * rs;
    }
}

bool vec_ok(int D, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= reinterpret_cast<uintptr_t>(q);
    return D % 4 == 0 && D <= 256 && (bits & 15) == 0;
}

int group_args(const char* who, const void* a, const void* b, const void* c, int N, int HW, int C, int G) {
    if (!a || !b || !c || N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G != 0) {
        static thread_local char msg[160];
        snprintf(msg, sizeof msg, "%s: NULL required pointer, a size <= 0, or C not divisible by the group count", who);
        return bcos_set_error(BCOS_E_INVAL, msg);
    }
    if ((int64_t)N * G >= ((int64_t)1 << 31)) return bcos_set_error(BCOS_E_NOSUP, "bcos_groupnorm_unc: too many groups");
    return BCOS_OK;
}

}  // namespace

extern "C" int bcos_layernorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int64_t rows,
                                      int D, float eps, void* stream) {
    if (!x || !y || rows <= 0 || D <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_layernorm_unc_fwd: NULL x / y, or rows / D <= 0");
    if (vec_ok(D, {x, weight, bias, y}))
        hipLaunchKernelGGL(unorm_rows_fwd_kernel<true>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y, rstd_out,
                           rows, D, eps);
    else
        hipLaunchKernelGGL(unorm_rows_fwd_kernel<false>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y, rstd_out,
                           rows, D, eps);
    return check_launch("unorm_rows_fwd_kernel");
}

extern "C" int bcos_layernorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, const float* addend,
                                               const float* mul2, float* out, float* out2, int64_t rows, int D, void* stream) {
    if (!gy || !rstd || (!out && !out2) || rows <= 0 || D <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_layernorm_unc_bwd_detached: NULL gy / rstd, neither out nor out2, or rows / D <= 0");
    if (vec_ok(D, {gy, weight, addend, mul2, out, out2}))
        hipLaunchKernelGGL(unorm_rows_bwd_detached_kernel<true>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, weight, rstd,
                           addend, mul2, out, out2, rows, D);
    else
        hipLaunchKernelGGL(unorm_rows_bwd_detached_kernel<false>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, weight, rstd,
                           addend, mul2, out, out2, rows, D);
    return check_launch("unorm_rows_bwd_detached_kernel");
}

extern "C" int bcos_layernorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, const float* addend,
                                      float* gx, float* xr_out, int64_t rows, int D, void* stream) {
    if (!gy || !x || !rstd || !gx || rows <= 0 || D <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_layernorm_unc_bwd: NULL gy / x / rstd / gx, or rows / D <= 0");
    if (vec_ok(D, {gy, x, weight, addend, gx, xr_out}))
        hipLaunchKernelGGL(unorm_rows_bwd_full_kernel<true>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, x, weight, rstd,
                           addend, gx, xr_out, rows, D);
    else
        hipLaunchKernelGGL(unorm_rows_bwd_full_kernel<false>, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, x, weight, rstd,
                           addend, gx, xr_out, rows, D);
    return check_launch("unorm_rows_bwd_full_kernel");
}

extern "C" int bcos_groupnorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int N, int HW,
                                      int C, int G, float eps, void* stream) {
    if (const int rc = group_args("bcos_groupnorm_unc_fwd", x, y, y, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(unorm_group_fwd_kernel, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y, rstd_out, HW,
                       C, G, eps);
    return check_launch("unorm_group_fwd_kernel");
}

extern "C" int bcos_groupnorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, float* gx, int N, int HW, int C,
                                               int G, void* stream) {
    if (const int rc = group_args("bcos_groupnorm_unc_bwd_detached", gy, rstd, gx, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(unorm_group_bwd_detached_kernel, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), gy, weight, rstd, gx, HW,
                       C, G);
    return check_launch("unorm_group_bwd_detached_kernel");
}

extern "C" int bcos_groupnorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xr_out,
                                      int N, int HW, int C, int G, void* stream) {
    if (!x) return bcos_set_error(BCOS_E_INVAL, "bcos_groupnorm_unc_bwd: NULL x");
    if (const int rc = group_args("bcos_groupnorm_unc_bwd", gy, rstd, gx, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(unorm_group_bwd_full_kernel, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), gy, x, weight, rstd, gx, xr_out,
                       HW, C, G);
    return check_launch("unorm_group_bwd_full_kernel");
}
