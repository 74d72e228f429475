// bcos_norms.hip -- the row and group norms of the B-cos networks on gfx950, centred and uncentered, as ONE family of kernels:
//   centred     DetachableLayerNorm / DetachablePositionNorm2d / DetachableGroupNorm2d (bcos/modules/norms/centered_norms.py:93-298):
//                   m = mean_S x,  var = mean_S (x - m)^2,  r = 1 / sqrt(var + eps),  xh = (x - m) r,  y = w xh + b
//                   explanation mode (var a constant, m not):   gx = h r - mean_S(h r),                          h = gy w
//                   training mode:                              gx = r (h - mean_S h - xh mean_S(h xh))
//   uncentered  the position / group norms of the B-cos v2 norm ablations (uncentered_norms/posnorm_uncentered.py:39-58,
//               groupnorm_uncentered.py:21-61): the variance is the same CENTRED second moment, but the value that is divided is x itself:
//                   y = w x r + b
//                   explanation mode (var a constant):          gx = h r
//                   training mode:                              gx = r h - r^3 (x - m) (sum_S h x) / n
// Row form (S = a row of x [rows, D]: a token, or a pixel's channels on the NHWC image): one wavefront per row.  Group form (S = an
// (image, group) of x [N, HW, C]): one workgroup per (image, group).  CENTERED is a template parameter of every kernel and the two
// flavours differ inside `if constexpr (CENTERED)` only: each keeps its own arithmetic expressions as written (the compiler contracts
// floating-point expressions, a reordered one may round differently).  Two-pass variance everywhere (mean, then centred squares),
// butterfly / fixed-order reductions, no atomics, no scratch: a call repeated gives the same bits, and no output depends on which
// optional outputs were requested.
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

// ---- row form: one wavefront per row ------------------------------------------------------------------------------------------------
// VEC: rows of up to 256 floats (D % 4 == 0, 16-byte aligned tensors) live in ONE float4 per lane -- read once, two wavefront
// reductions, written once, 16-byte accesses.  Other widths and misaligned views take the strided loop.  The centred flavour can
// also emit the row's max |y| (what the split-f16 contraction reading y scales its operand by): it falls out of the registers.  The
// uncentered entry points have no such output and their instantiations carry no code for it.
template <bool VEC, bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_rows_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ y,
                                                            float* __restrict__ rstd_out, unsigned* __restrict__ absmax_out,
                                                            int64_t rows, int D, float eps) {
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
            f32x4 o;
            if constexpr (CENTERED) o = f32x4{d[0] / sd, d[1] / sd, d[2] / sd, d[3] / sd};
            else o = f32x4{v[0] / sd, v[1] / sd, v[2] / sd, v[3] / sd};        // the value itself, not d
            o = o * wv + bv;
            if (on) *reinterpret_cast<f32x4*>(y + r * D + lane * 4) = o;
            if (rstd_out && lane == 0) rstd_out[r] = 1.0f / sd;
            if constexpr (CENTERED) {
                if (absmax_out) {
                    const unsigned m = wave_max_u32(on ? absbits4(o) : 0u);
                    if (lane == 0) absmax_out[r] = m;
                }
            }
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
            unsigned m = 0u;
            for (int c = lane; c < D; c += 64) {
                float o;
                if constexpr (CENTERED) o = (src[c] - mean) / sd;
                else o = src[c] / sd;
                if (w) o *= w[c];
                if (b) o += b[c];
                dst[c] = o;
                if constexpr (CENTERED) m = max(m, __float_as_uint(o) & 0x7fffffffu);
            }
            if (rstd_out && lane == 0) rstd_out[r] = 1.0f / sd;
            if constexpr (CENTERED) {
                if (absmax_out) {
                    m = wave_max_u32(m);
                    if (lane == 0) absmax_out[r] = m;
                }
            }
        }
    }
}

// Row statistics of the LayerNorm for a contraction that reads x itself (bcos_epilogue.row_scale / a_sumsq): same reductions as
// norm_rows_fwd_kernel (mean, then the centered second moment), plus |gamma xhat + beta|^2 and max |x|; nothing row-sized is written.
// Centred only: nothing uncentered reads row statistics.
__global__ __launch_bounds__(TPB) void layernorm_stats_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ rstd_out,
                                                              float* __restrict__ zss_out, unsigned* __restrict__ absmax_out,
                                                              int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const float* src = x + r * D;
        float s = 0.f;
        unsigned m = 0u;
        for (int c = lane; c < D; c += 64) { s += src[c]; m = max(m, __float_as_uint(src[c]) & 0x7fffffffu); }
        const float mean = wave_sum(s) / (float)D;
        float v = 0.f;
        for (int c = lane; c < D; c += 64) { const float d = src[c] - mean; v = fmaf(d, d, v); }
        const float var = wave_sum(v) / (float)D;
        const float sd = sqrtf(var + eps);
        if (lane == 0) rstd_out[r] = 1.0f / sd;
        if (zss_out) {
            float zs = 0.f;
            for (int c = lane; c < D; c += 64) {
                float o = (src[c] - mean) / sd;
                if (w) o *= w[c];
                if (b) o += b[c];
                zs = fmaf(o, o, zs);
            }
            zs = wave_sum(zs);
            if (lane == 0) zss_out[r] = zs;
        }
        if (absmax_out) {
            m = wave_max_u32(m);
            if (lane == 0) absmax_out[r] = m;
        }
    }
}

// The same statistics for rows of up to 256 floats (D % 4 == 0), SIXTEEN lanes per row: a wavefront holds four rows at once (NV
// 16-byte pieces per lane, four-step reductions), so a workgroup keeps 16 rows of loads in flight where the one-row-per-wavefront
// form above keeps four -- the kernel is one dependent chain per row (load, mean, centred moment, output norm) and nothing else.
__device__ inline float sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int NV>
__global__ __launch_bounds__(TPB) void layernorm_stats16_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ b, float* __restrict__ rstd_out,
                                                                float* __restrict__ zss_out, unsigned* __restrict__ absmax_out,
                                                                int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    f32x4 wv[NV], bv[NV];
    bool on[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (sub + 16 * i) * 4;
        on[i] = c < D;
        wv[i] = (on[i] && w) ? *reinterpret_cast<const f32x4*>(w + c) : f32x4{1.f, 1.f, 1.f, 1.f};
        bv[i] = (on[i] && b) ? *reinterpret_cast<const f32x4*>(b + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t r0 = wave * 4; r0 < rows; r0 += nwaves * 4) {
        const int64_t r = r0 + grp;
        const bool live = r < rows;
        f32x4 v[NV];
        float s = 0.f;
        unsigned m = 0u;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = (live && on[i]) ? *reinterpret_cast<const f32x4*>(x + r * D + (sub + 16 * i) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            m = max(m, absbits4(v[i]));
        }
        const float mean = sum16(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = on[i] ? v[i] - mean : f32x4{0.f, 0.f, 0.f, 0.f};
            q += fmaf(v[i][0], v[i][0], v[i][1] * v[i][1]) + fmaf(v[i][2], v[i][2], v[i][3] * v[i][3]);
        }
        const float sd = sqrtf(sum16(q) / (float)D + eps);
        if (sub == 0 && live) rstd_out[r] = 1.0f / sd;
        if (zss_out) {
            float zs = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                f32x4 o = {v[i][0] / sd, v[i][1] / sd, v[i][2] / sd, v[i][3] / sd};       // (the value norm_rows_fwd_kernel writes)
                o = o * wv[i] + bv[i];
                if (!on[i]) o = f32x4{0.f, 0.f, 0.f, 0.f};
                zs += fmaf(o[0], o[0], o[1] * o[1]) + fmaf(o[2], o[2], o[3] * o[3]);
            }
            zs = sum16(zs);
            if (sub == 0 && live) zss_out[r] = zs;
        }
        if (absmax_out) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
            if (sub == 0 && live) absmax_out[r] = m;
        }
    }
}

// explanation mode: the variance is a constant.  h = gy w rstd.
//   centred (the mean is not a constant, centered_norms.py:204-215):   y = w (x - mean(x)) / std   =>   gx = h - mean(h)
//   uncentered: nothing else of y depends on the row, so the gradient is elementwise:               gx = h, no reduction at all
// out = gx (+ addend); out2 = out * mul2 (the scale of the B-cos layer that produced x), both optional extras; the centred flavour can
// also emit the row maxima of out2.
template <bool VEC, bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_rows_bwd_detached_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                                     const float* __restrict__ rstd, const float* __restrict__ addend,
                                                                     const float* __restrict__ mul2, float* __restrict__ out,
                                                                     float* __restrict__ out2, unsigned* __restrict__ absmax2_out,
                                                                     int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    if constexpr (VEC) {
        const bool on = lane * 4 < D;
        if constexpr (!CENTERED) {
            if (!on) return;                                // (no wavefront reduction below: idle lanes may leave)
        }
        f32x4 wv = {1.f, 1.f, 1.f, 1.f};
        if (on && w) wv = *reinterpret_cast<const f32x4*>(w + lane * 4);
        for (int64_t r = wave; r < rows; r += nwaves) {
            const int64_t off = r * D + lane * 4;
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, ad = {0.f, 0.f, 0.f, 0.f}, m2 = {1.f, 1.f, 1.f, 1.f};
            if (on) g = *reinterpret_cast<const f32x4*>(gy + off);
            if (on && addend) ad = *reinterpret_cast<const f32x4*>(addend + off);
            if (on && mul2) m2 = *reinterpret_cast<const f32x4*>(mul2 + off);
            f32x4 o;
            if constexpr (CENTERED) {
                const float rs = rstd[r];
                const f32x4 h = g * wv * rs;
                const float mh = wave_sum((h[0] + h[1]) + (h[2] + h[3])) / (float)D;
                o = h - mh + ad;
            } else {
                o = g * wv * rstd[r] + ad;
            }
            const f32x4 o2 = o * m2;
            if (on && out) *reinterpret_cast<f32x4*>(out + off) = o;
            if (on && out2) *reinterpret_cast<f32x4*>(out2 + off) = o2;
            if constexpr (CENTERED) {
                if (absmax2_out) {
                    const unsigned m = wave_max_u32(on ? absbits4(o2) : 0u);
                    if (lane == 0) absmax2_out[r] = m;
                }
            }
        }
    } else {
        for (int64_t r = wave; r < rows; r += nwaves) {
            const float rs = rstd[r];
            if constexpr (CENTERED) {
                const float* g = gy + r * D;
                float s = 0.f;
                for (int c = lane; c < D; c += 64) s += g[c] * (w ? w[c] : 1.f) * rs;
                const float mh = wave_sum(s) / (float)D;
                unsigned m = 0u;
                for (int c = lane; c < D; c += 64) {
                    float o = g[c] * (w ? w[c] : 1.f) * rs - mh;
                    if (addend) o += addend[r * D + c];
                    if (out) out[r * D + c] = o;
                    const float o2 = mul2 ? o * mul2[r * D + c] : o;
                    if (out2) out2[r * D + c] = o2;
                    m = max(m, __float_as_uint(o2) & 0x7fffffffu);
                }
                if (absmax2_out) {
                    m = wave_max_u32(m);
                    if (lane == 0) absmax2_out[r] = m;
                }
            } else {
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
}

// training mode, nothing detached (+ addend: the residual stream's gradient joins here).  h = gy w; the second output is what the weight
// gradient (sum_rows gy xn, a column reduction) multiplies gy by.  The mean is recomputed from the row.
//   centred (F.layer_norm's gradient):  xn = x_hat = (x - mean) rstd,   gx = rstd (h - mean(h) - x_hat mean(h x_hat))
//   uncentered:                         xn = x rstd,                    gx = rs h - rs^3 (x - mean) (sum h x) / n
// The float4 form is written for the uncentered flavour only: the centred one stays on the strided loop (its float4 form sums in
// another order, so it is a change of bits and belongs to a change of its own).
template <bool VEC, bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_rows_bwd_full_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                 const float* __restrict__ w, const float* __restrict__ rstd,
                                                                 const float* __restrict__ addend, float* __restrict__ gx,
                                                                 float* __restrict__ xn, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    if constexpr (VEC) {
        static_assert(!CENTERED, "the centred full row gradient has no float4 form");
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
            if (on && xn) *reinterpret_cast<f32x4*>(xn + off) = v * rs;
        }
    } else {
        for (int64_t r = wave; r < rows; r += nwaves) {
            const float* xs = x + r * D;
            const float* gs = gy + r * D;
            if constexpr (CENTERED) {
                float s = 0.f;
                for (int c = lane; c < D; c += 64) s += xs[c];
                const float mean = wave_sum(s) / (float)D;
                const float rs = rstd[r];
                float sh = 0.f, shx = 0.f;
                for (int c = lane; c < D; c += 64) {
                    const float xh = (xs[c] - mean) * rs;
                    const float h = gs[c] * (w ? w[c] : 1.0f);
                    sh += h;
                    shx = fmaf(h, xh, shx);
                }
                const float mh = wave_sum(sh) / (float)D, mhx = wave_sum(shx) / (float)D;
                for (int c = lane; c < D; c += 64) {
                    const float xh = (xs[c] - mean) * rs;
                    const float h = gs[c] * (w ? w[c] : 1.0f);
                    const float g = rs * (h - mh - xh * mhx);
                    gx[r * D + c] = addend ? g + addend[r * D + c] : g;
                    if (xn) xn[r * D + c] = xh;
                }
            } else {
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
                    if (xn) xn[r * D + c] = xs[c] * rs;
                }
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

template <bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_group_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
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
        float o;
        if constexpr (CENTERED) o = (x[i] - mean) / sd;
        else o = x[i] / sd;
        if (w) o *= w[g * cg + c];
        if (b) o += b[g * cg + c];
        y[i] = o;
    }
    if (rstd_out && threadIdx.x == 0) rstd_out[blockIdx.x] = 1.0f / sd;
}

// explanation mode (variance constant), h = gy w rstd:  centred gx = h - mean_group(h) (the mean stays differentiable);  uncentered
// gx = h, elementwise
template <bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_group_bwd_detached_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                                      const float* __restrict__ rstd, float* __restrict__ gx,
                                                                      int HW, int C, int G) {
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cg = C / G;
    const int64_t base = (int64_t)n * HW * C + g * cg;
    const int64_t m = (int64_t)HW * cg;
    const float rs = rstd[blockIdx.x];
    float mh = 0.f;
    if constexpr (CENTERED) {
        __shared__ float red[TPB / 64];
        float s = 0.f;
        for (int64_t e = threadIdx.x; e < m; e += TPB) {
            const int c = (int)(e % cg);
            s += gy[base + (e / cg) * C + c] * (w ? w[g * cg + c] : 1.0f) * rs;
        }
        mh = block_sum(s, red) / (float)m;
    }
    for (int64_t e = threadIdx.x; e < m; e += TPB) {
        const int c = (int)(e % cg);
        const int64_t i = base + (e / cg) * C + c;
        if constexpr (CENTERED) gx[i] = gy[i] * (w ? w[g * cg + c] : 1.0f) * rs - mh;
        else gx[i] = gy[i] * (w ? w[g * cg + c] : 1.0f) * rs;
    }
}

// training mode, nothing detached: per (image, group) with m values, h = gy w; xn is written out for the weight gradient (a column
// reduction).  Centred (F.group_norm's gradient): xn = x_hat = (x - mean) rstd,  gx = rstd (h - mean(h) - x_hat mean(h x_hat));
// uncentered: xn = x rstd,  gx = rs h - rs^3 (x - mean) (sum h x) / m
template <bool CENTERED>
__global__ __launch_bounds__(TPB) void norm_group_bwd_full_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                  const float* __restrict__ w, const float* __restrict__ rstd,
                                                                  float* __restrict__ gx, float* __restrict__ xn, int HW, int C, int G) {
    __shared__ float red[TPB / 64];
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cg = C / G;
    const int64_t base = (int64_t)n * HW * C + g * cg;
    const int64_t m = (int64_t)HW * cg;
    const float rs = rstd[blockIdx.x];
    if constexpr (CENTERED) {
        float s = 0.f;
        for (int64_t e = threadIdx.x; e < m; e += TPB) s += x[base + (e / cg) * C + e % cg];
        const float mean = block_sum(s, red) / (float)m;
        float sh = 0.f, shx = 0.f;
        for (int64_t e = threadIdx.x; e < m; e += TPB) {
            const int c = (int)(e % cg);
            const int64_t i = base + (e / cg) * C + c;
            const float xh = (x[i] - mean) * rs;
            const float h = gy[i] * (w ? w[g * cg + c] : 1.0f);
            sh += h;
            shx = fmaf(h, xh, shx);
        }
        const float mh = block_sum(sh, red) / (float)m;
        const float mhx = block_sum(shx, red) / (float)m;
        for (int64_t e = threadIdx.x; e < m; e += TPB) {
            const int c = (int)(e % cg);
            const int64_t i = base + (e / cg) * C + c;
            const float xh = (x[i] - mean) * rs;
            const float h = gy[i] * (w ? w[g * cg + c] : 1.0f);
            gx[i] = rs * (h - mh - xh * mhx);
            if (xn) xn[i] = xh;
        }
    } else {
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
            if (xn) xn[i] = x[i] * rs;
        }
    }
}

// ---- host side: one launcher per kernel, both flavours' entry points call it ----------------------------------------------------------
bool vec_ok(int D, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= reinterpret_cast<uintptr_t>(q);
    return D % 4 == 0 && D <= 256 && (bits & 15) == 0;
}

template <bool CENTERED>
int rows_fwd(const char* refusal, const float* x, const float* weight, const float* bias, float* y, float* rstd_out, uint32_t* y_absmax,
             int64_t rows, int D, float eps, void* stream) {
    if (!x || !y || rows <= 0 || D <= 0) return bcos_set_error(BCOS_E_INVAL, refusal);
    if (vec_ok(D, {x, weight, bias, y}))
        hipLaunchKernelGGL((norm_rows_fwd_kernel<true, CENTERED>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y,
                           rstd_out, y_absmax, rows, D, eps);
    else
        hipLaunchKernelGGL((norm_rows_fwd_kernel<false, CENTERED>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y,
                           rstd_out, y_absmax, rows, D, eps);
    return check_launch("norm_rows_fwd_kernel");
}

template <bool CENTERED>
int rows_bwd_detached(const char* refusal, const float* gy, const float* weight, const float* rstd, const float* addend, const float* mul2,
                      float* out, float* out2, uint32_t* out2_absmax, int64_t rows, int D, void* stream) {
    if (!gy || !rstd || (!out && !out2) || rows <= 0 || D <= 0 || (out2_absmax && !out2)) return bcos_set_error(BCOS_E_INVAL, refusal);
    if (vec_ok(D, {gy, weight, addend, mul2, out, out2}))
        hipLaunchKernelGGL((norm_rows_bwd_detached_kernel<true, CENTERED>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, weight,
                           rstd, addend, mul2, out, out2, out2_absmax, rows, D);
    else
        hipLaunchKernelGGL((norm_rows_bwd_detached_kernel<false, CENTERED>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, weight,
                           rstd, addend, mul2, out, out2, out2_absmax, rows, D);
    return check_launch("norm_rows_bwd_detached_kernel");
}

template <bool CENTERED>
int rows_bwd_full(const char* refusal, const float* gy, const float* x, const float* weight, const float* rstd, const float* addend,
                  float* gx, float* xn_out, int64_t rows, int D, void* stream) {
    if (!gy || !x || !rstd || !gx || rows <= 0 || D <= 0) return bcos_set_error(BCOS_E_INVAL, refusal);
    if constexpr (!CENTERED) {
        if (vec_ok(D, {gy, x, weight, addend, gx, xn_out})) {
            hipLaunchKernelGGL((norm_rows_bwd_full_kernel<true, false>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, x, weight,
                               rstd, addend, gx, xn_out, rows, D);
            return check_launch("norm_rows_bwd_full_kernel");
        }
    }
    hipLaunchKernelGGL((norm_rows_bwd_full_kernel<false, CENTERED>), dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), gy, x, weight,
                       rstd, addend, gx, xn_out, rows, D);
    return check_launch("norm_rows_bwd_full_kernel");
}

// the shared refusals of the group entry points
int group_args(const char* who, std::initializer_list<const void*> required, int N, int HW, int C, int G) {
    static thread_local char msg[160];
    bool null = false;
    for (const void* q : required) null |= !q;
    if (null || N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G != 0) {
        snprintf(msg, sizeof msg, "%s: NULL required pointer, a size <= 0, or C not divisible by the group count", who);
        return bcos_set_error(BCOS_E_INVAL, msg);
    }
    if ((int64_t)N * G >= ((int64_t)1 << 31)) {
        snprintf(msg, sizeof msg, "%s: too many groups", who);
        return bcos_set_error(BCOS_E_NOSUP, msg);
    }
    return BCOS_OK;
}

template <bool CENTERED>
int group_fwd(const char* who, const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int N, int HW, int C,
              int G, float eps, void* stream) {
    if (const int rc = group_args(who, {x, y}, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(norm_group_fwd_kernel<CENTERED>, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), x, weight, bias, y, rstd_out,
                       HW, C, G, eps);
    return check_launch("norm_group_fwd_kernel");
}

template <bool CENTERED>
int group_bwd_detached(const char* who, const float* gy, const float* weight, const float* rstd, float* gx, int N, int HW, int C, int G,
                       void* stream) {
    if (const int rc = group_args(who, {gy, rstd, gx}, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(norm_group_bwd_detached_kernel<CENTERED>, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), gy, weight, rstd, gx,
                       HW, C, G);
    return check_launch("norm_group_bwd_detached_kernel");
}

template <bool CENTERED>
int group_bwd_full(const char* who, const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xn_out,
                   int N, int HW, int C, int G, void* stream) {
    if (const int rc = group_args(who, {gy, x, rstd, gx}, N, HW, C, G)) return rc;
    hipLaunchKernelGGL(norm_group_bwd_full_kernel<CENTERED>, dim3((unsigned)(N * G)), dim3(TPB), 0, STREAM(stream), gy, x, weight, rstd, gx,
                       xn_out, HW, C, G);
    return check_launch("norm_group_bwd_full_kernel");
}

}  // namespace

// ---- centred ----------------------------------------------------------------------------------------------------------------------------
extern "C" int bcos_layernorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out,
                                  uint32_t* y_absmax, int64_t rows, int D, float eps, void* stream) {
    return rows_fwd<true>("bcos_layernorm_fwd: bad argument", x, weight, bias, y, rstd_out, y_absmax, rows, D, eps, stream);
}

extern "C" int bcos_layernorm_stats(const float* x, const float* weight, const float* bias, float* rstd_out, float* zsumsq_out,
                                    uint32_t* x_absmax, int64_t rows, int D, float eps, void* stream) {
    if (!x || !rstd_out || rows <= 0 || D <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_layernorm_stats: bad argument");
    if (vec_ok(D, {x, weight, bias})) {
        int64_t nb = (rows + 15) / 16;           // 16 rows per workgroup and pass
        if (nb > 256 * 32) nb = 256 * 32;
        const dim3 grid((unsigned)nb), block(TPB);
        hipStream_t st = STREAM(stream);
        switch ((D + 63) / 64) {
            case 1: hipLaunchKernelGGL(layernorm_stats16_kernel<1>, grid, block, 0, st, x, weight, bias, rstd_out, zsumsq_out, x_absmax, rows, D, eps); break;
            case 2: hipLaunchKernelGGL(layernorm_stats16_kernel<2>, grid, block, 0, st, x, weight, bias, rstd_out, zsumsq_out, x_absmax, rows, D, eps); break;
            case 3: hipLaunchKernelGGL(layernorm_stats16_kernel<3>, grid, block, 0, st, x, weight, bias, rstd_out, zsumsq_out, x_absmax, rows, D, eps); break;
            default: hipLaunchKernelGGL(layernorm_stats16_kernel<4>, grid, block, 0, st, x, weight, bias, rstd_out, zsumsq_out, x_absmax, rows, D, eps); break;
        }
    } else
        hipLaunchKernelGGL(layernorm_stats_kernel, dim3(grid_rows(rows)), dim3(TPB), 0, STREAM(stream), x, weight, bias, rstd_out,
                           zsumsq_out, x_absmax, rows, D, eps);
    return check_launch("layernorm_stats_kernel");
}

extern "C" int bcos_layernorm_bwd_detached(const float* gy, const float* weight, const float* rstd, const float* addend,
                                           const float* mul2, float* out, float* out2, uint32_t* out2_absmax, int64_t rows, int D,
                                           void* stream) {
    return rows_bwd_detached<true>("bcos_layernorm_bwd_detached: bad argument", gy, weight, rstd, addend, mul2, out, out2, out2_absmax, rows,
                                   D, stream);
}

extern "C" int bcos_layernorm_bwd_add(const float* gy, const float* x, const float* weight, const float* rstd, const float* addend,
                                      float* gx, float* xhat_out, int64_t rows, int D, void* stream) {
    return rows_bwd_full<true>("bcos_layernorm_bwd: bad argument", gy, x, weight, rstd, addend, gx, xhat_out, rows, D, stream);
}

extern "C" int bcos_layernorm_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xhat_out,
                                  int64_t rows, int D, void* stream) {
    return bcos_layernorm_bwd_add(gy, x, weight, rstd, nullptr, gx, xhat_out, rows, D, stream);
}

extern "C" int bcos_groupnorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int N, int HW,
                                  int C, int G, float eps, void* stream) {
    return group_fwd<true>("bcos_groupnorm_fwd", x, weight, bias, y, rstd_out, N, HW, C, G, eps, stream);
}

extern "C" int bcos_groupnorm_bwd_detached(const float* gy, const float* weight, const float* rstd, float* gx, int N, int HW, int C,
                                           int G, void* stream) {
    return group_bwd_detached<true>("bcos_groupnorm_bwd_detached", gy, weight, rstd, gx, N, HW, C, G, stream);
}

extern "C" int bcos_groupnorm_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xhat_out,
                                  int N, int HW, int C, int G, void* stream) {
    return group_bwd_full<true>("bcos_groupnorm_bwd", gy, x, weight, rstd, gx, xhat_out, N, HW, C, G, stream);
}

// ---- uncentered: no row maxima in this ABI ------------------------------------------------------------------------------------------------
extern "C" int bcos_layernorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int64_t rows,
                                      int D, float eps, void* stream) {
    return rows_fwd<false>("bcos_layernorm_unc_fwd: NULL x / y, or rows / D <= 0", x, weight, bias, y, rstd_out, nullptr, rows, D, eps,
                           stream);
}

extern "C" int bcos_layernorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, const float* addend,
                                               const float* mul2, float* out, float* out2, int64_t rows, int D, void* stream) {
    return rows_bwd_detached<false>("bcos_layernorm_unc_bwd_detached: NULL gy / rstd, neither out nor out2, or rows / D <= 0", gy, weight,
                                    rstd, addend, mul2, out, out2, nullptr, rows, D, stream);
}

extern "C" int bcos_layernorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, const float* addend,
                                      float* gx, float* xr_out, int64_t rows, int D, void* stream) {
    return rows_bwd_full<false>("bcos_layernorm_unc_bwd: NULL gy / x / rstd / gx, or rows / D <= 0", gy, x, weight, rstd, addend, gx, xr_out,
                                rows, D, stream);
}

extern "C" int bcos_groupnorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int N, int HW,
                                      int C, int G, float eps, void* stream) {
    return group_fwd<false>("bcos_groupnorm_unc_fwd", x, weight, bias, y, rstd_out, N, HW, C, G, eps, stream);
}

extern "C" int bcos_groupnorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, float* gx, int N, int HW, int C,
                                               int G, void* stream) {
    return group_bwd_detached<false>("bcos_groupnorm_unc_bwd_detached", gy, weight, rstd, gx, N, HW, C, G, stream);
}

extern "C" int bcos_groupnorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xr_out,
                                      int N, int HW, int C, int G, void* stream) {
    return group_bwd_full<false>("bcos_groupnorm_unc_bwd", gy, x, weight, rstd, gx, xr_out, N, HW, C, G, stream);
}
