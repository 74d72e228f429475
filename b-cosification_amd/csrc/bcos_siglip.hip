// bcos_siglip.hip -- the SigLIP distillation objective of the CLIP B-cosification recipe (SigLipLoss, bcos/modules/losses.py:576-638 of
// the reference, as bcos/training/trainer.py:666-707 calls it: both sides L2-normalised, the attn_unpool head's location cosines raised
// to cos_power and averaged first), loss AND every gradient in one call.  The reference is two F.normalize, a batched matmul, pow / abs /
// mean, scale, bias, labels, logsigmoid, a sum and the autograd of all of it: some dozens of small launches.  Here: three launches,
//   1. siglip_cosines   one wavefront per student row (l, i) and slice of the teacher rows: the row divided by max(||s||, eps), then
//                       c[l,i,j] (four j per pass over the row; the teacher row's own max(||t||, eps) comes out of the same pass);
//   2. siglip_pairs     one wavefront per batch row i, lanes over j: the mean over locations, z, the stable logsigmoid, G, the
//                       coefficient of every location's cosine, and the row's partial sums;
//   3. siglip_grads     gs (one wavefront per 256 elements of a row), gt (one thread per element) and the three scalars, as block
//                       ranges of one grid.
// The normalisation's backward needs u . g; with g = sum_j dc_j ut_j that is sum_j dc_j c_j, so it is taken from the cosines (pass 1) and
// their coefficients (pass 2) and every output element is written once, by one thread, from a chain in a fixed order.  No atomics of any
// kind, no launch-shape dependence: two calls on the same data give the same bits.  Plain FMAs: 2 x 10^8 multiply-adds at the recipe's
// largest shape (L = 49, N = M = 64, D = 1024) -- the matrix pipe would not change what the step costs, the launch count does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int SL_TPB = 256;
constexpr int SL_WAVES = SL_TPB / 64;
constexpr int SL_JB = 4;                       // teacher rows per pass over a student row (pass 1)
constexpr int SL_LB = 8;                       // locations per batch of loads (pass 2)
constexpr int SL_DB = 4;                       // 64-float slices of a gradient row held in registers at once (pass 3)
constexpr float SL_NORM_EPS = 1e-12f;          // F.normalize's eps
constexpr int SL_MAX_P = 64;

struct SiglipArgs {
    const float* s;          // [L, N, D]
    const float* t;          // [M, D]
    const float* scale;      // device scalar
    const float* bias;       // device scalar
    float* loss;
    float* gs;               // NULL or [L, N, D]
    float* gt;               // NULL or [M, D]
    float* gscale;           // NULL or scalar
    float* gbias;            // NULL or scalar
    // workspace
    float* ns;               // [L*N]   max(||s_r||, eps), negated for a row below the clamp   (NORMALIZE only, as the next three)
    float* nt;               // [M]
    float* us;               // [L*N, D] s_r / max(||s_r||, eps)
    float* ut;               // [M, D]
    float* c;                // [L*N, M] cosines
    float* dc;               // [L*N, M] d loss / d c
    float* rdot;             // [N, M]   sum_l dc[l,i,j] c[l,i,j]
    float* part;             // [3, N]   per batch row: sum logsigmoid, sum G q, sum G
    int L, N, M, D, pos_offset, p, normalize, detach_pow;
};

// max(||x||, eps) from the sum of squares.  A row below the clamp gets it with a minus sign: the workspace carries that to the gradient
// pass, where such a row's norm is a constant (torch's clamp_min passes no gradient there).  Every normalised element is x / norm, an
// IEEE division as in F.normalize (x / x is exactly 1: a one-element row normalises to exactly +-1)
__device__ __forceinline__ float clamped_norm(float sumsq) {
    const float n = sqrtf(sumsq);
    return n < SL_NORM_EPS ? -SL_NORM_EPS : n;
}

// |c|^(p-1) for p >= 2 by p - 2 multiplications
__device__ __forceinline__ float abs_pow(float c, int p) {
    const float a = fabsf(c);
    float w = a;
    for (int k = 2; k < p; ++k) w *= a;
    return w;
}

// One wavefront per (student row r, slice of the teacher rows): `jsplit` slices of `jper` rows each (a multiple of SL_JB), so that a pooled
// batch of 64 rows still fills the device.  Every slice's wave takes the row's norm (the same chain: the same bits); slice 0 stores the
// normalised row for the gradient pass.  Which wave computes c[r, j] changes nothing about how it is computed.
__global__ __launch_bounds__(SL_TPB) void siglip_cosines(const SiglipArgs a, int jsplit, int jper) {
    const int lane = threadIdx.x & 63;
    const int64_t R = (int64_t)a.L * a.N;
    const int64_t w = (int64_t)blockIdx.x * SL_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= R * jsplit) return;
    const int64_t r = w / jsplit;
    const int slice = (int)(w % jsplit);
    const int D = a.D, M = a.M;
    const float* s = a.s + r * D;
    float ns = 1.0f;
    if (a.normalize) {
        float ss = 0.f;
#pragma unroll 4
        for (int d = lane; d < D; d += 64) ss = fmaf(s[d], s[d], ss);
        const float n = clamped_norm(wave_sum(ss));
        ns = fabsf(n);
        if (slice == 0) {
            if (lane == 0) a.ns[r] = n;
            float* us = a.us + r * D;
            for (int d = lane; d < D; d += 64) us[d] = s[d] / ns;
        }
    }
    // a wave that takes every teacher row reads the normalised elements back (each lane the ones it stored) instead of dividing again
    const float* u = a.normalize && jsplit == 1 ? a.us + r * D : nullptr;
    const int jend = (slice + 1) * jper < M ? (slice + 1) * jper : M;
    for (int j0 = slice * jper; j0 < jend; j0 += SL_JB) {
        const float* t[SL_JB];
        float acc[SL_JB], tt[SL_JB];
#pragma unroll
        for (int k = 0; k < SL_JB; ++k) {
            const int j = j0 + k < M ? j0 + k : M - 1;        // the tail repeats the last row; its result is not stored
            t[k] = a.t + (int64_t)j * D;
            acc[k] = 0.f;
            tt[k] = 0.f;
        }
#pragma unroll 4
        for (int d = lane; d < D; d += 64) {
            const float x = u ? u[d] : a.normalize ? s[d] / ns : s[d];
#pragma unroll
            for (int k = 0; k < SL_JB; ++k) {
                const float v = t[k][d];
                acc[k] = fmaf(x, v, acc[k]);
                tt[k] = fmaf(v, v, tt[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < SL_JB; ++k) {
            const int j = j0 + k;
            float c = wave_sum(acc[k]);
            float nt = 1.0f;
            if (a.normalize) {
                nt = clamped_norm(wave_sum(tt[k]));
                c /= fabsf(nt);
            }
            if (j >= M) continue;
            if (lane == 0) a.c[r * M + j] = c;
            if (a.normalize && j % R == r) {                  // every wave knows ||t_j||; the normalised row is written by ONE of them
                if (lane == 0) a.nt[j] = nt;
                float* ut = a.ut + (int64_t)j * D;
                for (int d = lane; d < D; d += 64) ut[d] = t[k][d] / fabsf(nt);
            }
        }
    }
}

__global__ __launch_bounds__(SL_TPB) void siglip_pairs(const SiglipArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * SL_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= a.N) return;
    const int L = a.L, N = a.N, M = a.M, p = a.p;
    const float scale = *a.scale, bias = *a.bias;
    const float fL = (float)L, fN = (float)N;
    const int pos = a.pos_offset >= 0 ? a.pos_offset + i : -1;
    float s_ls = 0.f, s_gq = 0.f, s_g = 0.f;
    for (int j = lane; j < M; j += 64) {
        float sum = 0.f;
#pragma unroll 8
        for (int l = 0; l < L; ++l) {
            const float c = a.c[((int64_t)l * N + i) * M + j];
            sum += p >= 2 ? c * abs_pow(c, p) : c;
        }
        const float q = sum / fL;                              // (exact for L = 1)
        const float z = fmaf(scale, q, bias);
        const float y = j == pos ? 1.0f : -1.0f;
        const float x = y * z;
        // logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)); sigmoid(-x) from the same exponential: e / (1 + e) for x >= 0, 1 / (1 + e) below
        const float e = expf(-fabsf(x));
        s_ls += fminf(x, 0.f) - log1pf(e);
        const float sg = (x >= 0.f ? e : 1.0f) / (1.0f + e);
        const float G = (-y * sg) / fN;
        s_g += G;
        s_gq = fmaf(G, q, s_gq);
        const float coef = (G * scale) / fL;                   // d loss / d f(c_l), the same for every location
        float rd = 0.f;
        for (int l0 = 0; l0 < L; l0 += SL_LB) {               // SL_LB cosines loaded ahead of the stores they could alias
            float cv[SL_LB];
#pragma unroll
            for (int k = 0; k < SL_LB; ++k) cv[k] = l0 + k < L ? a.c[((int64_t)(l0 + k) * N + i) * M + j] : 0.f;
#pragma unroll
            for (int k = 0; k < SL_LB; ++k) {
                if (l0 + k >= L) break;
                float d = coef;
                if (p >= 2) {
                    const float w = abs_pow(cv[k], p);
                    d = a.detach_pow ? coef * w : coef * ((float)p * w);
                }
                a.dc[((int64_t)(l0 + k) * N + i) * M + j] = d;
                rd = fmaf(d, cv[k], rd);
            }
        }
        a.rdot[(int64_t)i * M + j] = rd;
    }
    s_ls = wave_sum(s_ls);
    s_gq = wave_sum(s_gq);
    s_g = wave_sum(s_g);
    if (lane == 0) {
        a.part[i] = s_ls;
        a.part[N + i] = s_gq;
        a.part[2 * N + i] = s_g;
    }
}

__global__ __launch_bounds__(SL_TPB) void siglip_grads(const SiglipArgs a, int64_t gs_blocks, int64_t gt_blocks) {
    const int lane = threadIdx.x & 63;
    const int L = a.L, N = a.N, M = a.M, D = a.D;
    const int64_t R = (int64_t)L * N;
    const int64_t b = blockIdx.x;
    const float* us = a.normalize ? a.us : a.s;
    const float* ut = a.normalize ? a.ut : a.t;
    if (b < gs_blocks) {
        // gs[r, :] = (sum_j dc[r, j] ut_j - us_r (us_r . g)) / max(||s_r||, eps), j ascending; below the clamp the norm is a constant.
        // One wavefront per (row, 256 consecutive d): four per lane
        const int chunks = (D + 64 * SL_DB - 1) / (64 * SL_DB);
        const int64_t w = b * SL_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (w >= R * chunks) return;
        const int64_t r = w / chunks;
        const int d0 = (int)(w % chunks) * 64 * SL_DB;
        const float* dc = a.dc + r * M;
        const float ns = a.normalize ? a.ns[r] : 1.0f;
        const bool project = a.normalize && ns > 0.f;
        float rowdot = 0.f;
        if (project) {
            const float* c = a.c + r * M;
            for (int j = lane; j < M; j += 64) rowdot = fmaf(dc[j], c[j], rowdot);
            rowdot = wave_sum(rowdot);
        }
        const float* u = us + r * D;
        float* g = a.gs + r * D;
        float acc[SL_DB];
        int d[SL_DB];
#pragma unroll
        for (int k = 0; k < SL_DB; ++k) {
            acc[k] = 0.f;
            d[k] = d0 + 64 * k + lane;
            if (d[k] >= D) d[k] = -1;
        }
#pragma unroll 4
        for (int j = 0; j < M; ++j) {
            const float wj = dc[j];
            const float* t = ut + (int64_t)j * D;
#pragma unroll
            for (int k = 0; k < SL_DB; ++k)
                if (d[k] >= 0) acc[k] = fmaf(wj, t[d[k]], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < SL_DB; ++k) {
            if (d[k] < 0) continue;
            float v = acc[k];
            if (project) v = fmaf(-u[d[k]], rowdot, v);
            g[d[k]] = a.normalize ? v / fabsf(ns) : v;
        }
    } else if (b < gs_blocks + gt_blocks) {
        // gt[j, d] = (sum_{l, i} dc[l, i, j] us_{l, i}[d] - ut_j[d] (ut_j . g)) / max(||t_j||, eps), l outer, i inner
        const int64_t e = (b - gs_blocks) * SL_TPB + threadIdx.x;
        if (e >= (int64_t)M * D) return;
        const int j = (int)(e / D), d = (int)(e % D);
        const float nt = a.normalize ? a.nt[j] : 1.0f;
        const bool project = a.normalize && nt > 0.f;
        float coldot = 0.f;
        if (project)
            for (int i = 0; i < N; ++i) coldot += a.rdot[(int64_t)i * M + j];
        float acc = 0.f;
#pragma unroll 8
        for (int64_t r = 0; r < R; ++r) acc = fmaf(a.dc[r * M + j], us[r * D + d], acc);
        if (project) acc = fmaf(-ut[e], coldot, acc);
        a.gt[e] = a.normalize ? acc / fabsf(nt) : acc;
    } else if (threadIdx.x < 64) {
        // the scalars: per-lane chains over the batch rows in ascending order, then the butterfly
        float s_ls = 0.f, s_gq = 0.f, s_g = 0.f;
        for (int i = lane; i < N; i += 64) {
            s_ls += a.part[i];
            s_gq += a.part[N + i];
            s_g += a.part[2 * N + i];
        }
        s_ls = wave_sum(s_ls);
        s_gq = wave_sum(s_gq);
        s_g = wave_sum(s_g);
        if (lane == 0) {
            *a.loss = -s_ls / (float)N;
            if (a.gscale) *a.gscale = s_gq;
            if (a.gbias) *a.gbias = s_g;
        }
    }
}

// the sizes the kernels index with: everything that is multiplied fits int64 by construction (int x int x int), the grids must fit 2^31 - 1
int siglip_check_sizes(int L, int N, int M, int D, const char** why) {
    if (L <= 0 || N <= 0 || M <= 0 || D <= 0) {
        *why = "L, N, M and D must be positive";
        return BCOS_E_INVAL;
    }
    const int64_t R = (int64_t)L * N, cap = (int64_t)1 << 38;
    if (R > cap / M || R > cap / D || (int64_t)M * D > cap) {
        *why = "L * N * M, L * N * D or M * D too large";
        return BCOS_E_INVAL;
    }
    return BCOS_OK;
}

int64_t siglip_ws_floats(int L, int N, int M, int D) {
    const int64_t R = (int64_t)L * N;
    return R + M + (R + M) * D + 2 * R * M + (int64_t)N * M + 3 * (int64_t)N;
}

}  // namespace

extern "C" int bcos_siglip_loss_ws_floats(int L, int N, int M, int D, int64_t* floats) {
    const char* why = nullptr;
    if (!floats) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss_ws_floats: floats is NULL");
    if (siglip_check_sizes(L, N, M, D, &why) != BCOS_OK) return bcos_set_error(BCOS_E_INVAL, why);
    *floats = siglip_ws_floats(L, N, M, D);
    return BCOS_OK;
}

extern "C" int bcos_siglip_loss(const float* s, const float* t, const float* scale, const float* bias, float* loss, float* gs, float* gt,
                                float* gscale, float* gbias, float* ws, int64_t ws_floats, int L, int N, int M, int D, int pos_offset, int p,
                                int flags, void* stream) {
    // everything is checked before the first launch
    if (!s || !t || !loss) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: s, t and loss must not be NULL");
    if (!scale || !bias) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: scale and bias are device scalars, not NULL");
    const char* why = nullptr;
    if (siglip_check_sizes(L, N, M, D, &why) != BCOS_OK) return bcos_set_error(BCOS_E_INVAL, why);
    if (pos_offset >= 0 && (int64_t)pos_offset + N > M)
        return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: pos_offset + N exceeds M (a row's positive column does not exist)");
    if (p < 0 || p > SL_MAX_P) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: p must lie in [0, 64]");
    if (L > 1 && p == 0) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: p = 0 is the pooled form, it takes L = 1");
    if (flags & ~(BCOS_SIGLIP_NORMALIZE | BCOS_SIGLIP_DETACH_POW)) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: unknown flag");
    const int64_t need = siglip_ws_floats(L, N, M, D);
    if (!ws || ws_floats < need) return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: ws is NULL or smaller than bcos_siglip_loss_ws_floats");

    const int64_t R = (int64_t)L * N;
    SiglipArgs a;
    a.s = s; a.t = t; a.scale = scale; a.bias = bias;
    a.loss = loss; a.gs = gs; a.gt = gt; a.gscale = gscale; a.gbias = gbias;
    a.ns = ws;
    a.nt = a.ns + R;
    a.us = a.nt + M;
    a.ut = a.us + R * D;
    a.c = a.ut + (int64_t)M * D;
    a.dc = a.c + R * M;
    a.rdot = a.dc + R * M;
    a.part = a.rdot + (int64_t)N * M;
    a.L = L; a.N = N; a.M = M; a.D = D; a.pos_offset = pos_offset < 0 ? -1 : pos_offset; a.p = p;
    a.normalize = (flags & BCOS_SIGLIP_NORMALIZE) != 0;
    a.detach_pow = (flags & BCOS_SIGLIP_DETACH_POW) != 0;

    // pass 1: the teacher rows in jsplit slices of jper (a multiple of SL_JB) so that about 2048 waves run; pass 3: 256 d per wave
    const int jblocks = (M + SL_JB - 1) / SL_JB;
    int64_t jsplit = R >= 2048 ? 1 : (2048 + R - 1) / R;
    if (jsplit > jblocks) jsplit = jblocks;
    const int jper = (int)((jblocks + jsplit - 1) / jsplit) * SL_JB;
    jsplit = (M + jper - 1) / jper;
    const int64_t chunks = (D + 64 * SL_DB - 1) / (64 * SL_DB);
    const int64_t row_blocks = (R * jsplit + SL_WAVES - 1) / SL_WAVES;
    const int64_t gs_blocks = gs ? (R * chunks + SL_WAVES - 1) / SL_WAVES : 0;
    const int64_t gt_blocks = gt ? ((int64_t)M * D + SL_TPB - 1) / SL_TPB : 0;
    if (row_blocks > INT32_MAX || gs_blocks + gt_blocks + 1 > INT32_MAX)
        return bcos_set_error(BCOS_E_INVAL, "bcos_siglip_loss: the problem needs more than 2^31 - 1 workgroups");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(siglip_cosines, dim3((unsigned)row_blocks), dim3(SL_TPB), 0, st, a, (int)jsplit, jper);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("siglip_cosines", err);
    hipLaunchKernelGGL(siglip_pairs, dim3((unsigned)((N + SL_WAVES - 1) / SL_WAVES)), dim3(SL_TPB), 0, st, a);
    err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("siglip_pairs", err);
    hipLaunchKernelGGL(siglip_grads, dim3((unsigned)(gs_blocks + gt_blocks + 1)), dim3(SL_TPB), 0, st, a, gs_blocks, gt_blocks);
    err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("siglip_grads", err);
    return BCOS_OK;
}
