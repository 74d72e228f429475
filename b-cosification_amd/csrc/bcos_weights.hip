// bcos_weights.hip -- the pre-split weight images the tapconv loops read (bcos_tapconv.hip): the bf16x3 image (bcos_split_weights), the
// scaled f16x2 image with its inverse row scales (bcos_split_weights_f16x2*), and banks + images of many layers from one call
// (bcos_weight_prep_batch).  The image sizes (split_bytes, h2_tiles, h2_image_bytes) are shared with the dispatcher: bcos_tapconv_plan.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"
#include "bcos_tapconv_plan.h"

namespace {

// wt [rows][Ktot] fp32 -> wt3 [32-row tile][16-k step][plane h|m|l][lane][8 bf16]: lane = (row % 32) + 32 * ((k % 16) / 8),
// i.e. the B operand of v_mfma_f32_32x32x16_bf16 for that (tile, step); rows are padded to a multiple of 128 and k to a
// multiple of 16 with zeros.  Same truncating split as tile_body_x3::split_store (bit-identical products).
__global__ __launch_bounds__(256) void split_weights_kernel(const float* __restrict__ wt, uint4* __restrict__ wt3, int rows,
                                                            int Ktot, int nk, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // (tile, ks, lane)
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const int64_t ts = i >> 6;
    const int ks = (int)(ts % nk);
    const int tile = (int)(ts / nk);
    const int row = tile * 32 + (lane & 31);
    const int k0 = ks * 16 + 8 * (lane >> 5);
    unsigned h[8], m[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (row < rows && k0 + e < Ktot) ? wt[(int64_t)row * Ktot + k0 + e] : 0.f;
        h[e] = __float_as_uint(x) & 0xffff0000u;
        const float r1 = x - __uint_as_float(h[e]);
        m[e] = __float_as_uint(r1) & 0xffff0000u;
        l[e] = __float_as_uint(r1 - __uint_as_float(m[e])) & 0xffff0000u;
    }
    auto pack = [](const unsigned (&v)[8]) {
        return uint4{(v[0] >> 16) | v[1], (v[2] >> 16) | v[3], (v[4] >> 16) | v[5], (v[6] >> 16) | v[7]};
    };
    uint4* dst = wt3 + (ts * 3) * 64 + lane;
    dst[0] = pack(h);
    dst[64] = pack(m);
    dst[128] = pack(l);
}

}  // namespace

extern "C" int bcos_split_weights_bytes(int rows, int Ktot, int64_t* bytes) {
    if (rows <= 0 || Ktot <= 0 || !bytes) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights_bytes: bad argument");
    *bytes = split_bytes(rows, Ktot);
    return BCOS_OK;
}

extern "C" int bcos_split_weights(const float* wt, void* wt3, int rows, int Ktot, void* stream) {
    if (!wt || !wt3 || rows <= 0 || Ktot <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights: bad argument");
    if (reinterpret_cast<uintptr_t>(wt3) & 15) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights: wt3 must be 16-byte aligned");
    const int nk = (Ktot + 15) / 16;
    const int64_t total = split_bytes(rows, Ktot) / (3 * 16);
    hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), wt, reinterpret_cast<uint4*>(wt3), rows, Ktot, nk, total);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("split_weights launch", err);
    return BCOS_OK;
}

namespace {

// f16x2 image of wt [rows][Ktot]: [32-row tile][16-k step][plane h|l][lane][8 f16] (B fragments of v_mfma_f32_32x32x16_f16,
// rows padded to a multiple of 128, k to a multiple of 16) followed by the inverse row scales float[padded rows].
// Row r is scaled by 2^e_r so that its max |w| lands in [2^14, 2^15) before the split (exact), cinv[r] = 2^-e_r.
__global__ __launch_bounds__(256) void weight_rowscale_kernel(const float* __restrict__ wt, float* __restrict__ cinv, int rows,
                                                              int rows_pad, int Ktot) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows_pad) return;
    unsigned m = 0u;
    if (row < rows)
        for (int k = lane; k < Ktot; k += 64) m = max(m, absbits(wt[(int64_t)row * Ktot + k]));
    m = wave_max_u32(m);
    if (lane == 0) cinv[row] = f16x2_inv(f16x2_exp(m));
}

__global__ __launch_bounds__(256) void split_weights_h2_kernel(const float* __restrict__ wt, uint4* __restrict__ wt2,
                                                               const float* __restrict__ cinv, int rows, int Ktot, int nk,
                                                               int64_t total, int taps, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // (tile, ks, lane)
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const int64_t ts = i >> 6;
    const int ks = (int)(ts % nk);
    const int tile = (int)(ts / nk);
    const int row = tile * 32 + (lane & 31);
    // k of the 8 elements: plain order, or (taps > 1) channel-chunk-major: step ks = tap ks % taps of 16-channel chunk ks / taps
    const int k0 = taps > 1 ? (ks % taps) * C + (ks / taps) * 16 + 8 * (lane >> 5) : ks * 16 + 8 * (lane >> 5);
    const float scale = 1.0f / cinv[row];                             // exact: a power of two
    f16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (row < rows && k0 + e < Ktot) ? wt[(int64_t)row * Ktot + k0 + e] * scale : 0.f;
        const _Float16 hh = (_Float16)x;
        h[e] = hh;
        l[e] = (_Float16)(x - (float)hh);
    }
    uint4* dst = wt2 + (ts * 2) * 64 + lane;
    dst[0] = __builtin_bit_cast(uint4, h);
    dst[64] = __builtin_bit_cast(uint4, l);
}

// both steps in one launch for small weight tensors (one workgroup per 32-row tile: row maxima, then its fragments) -- a training step
// re-splits every weight twice (the forward and the transposed input-gradient image), ~100 images of 37-400 K elements for ViT-Ti:
// half the launches of that for the block weights.  Same arithmetic as the two kernels above.
__global__ __launch_bounds__(256) void split_weights_h2_fused_kernel(const float* __restrict__ wt, uint4* __restrict__ wt2,
                                                                     float* __restrict__ cinv, int rows, int Ktot, int nk, int taps, int C) {
    // grid (32-row tile, K part): every workgroup takes the maxima of its tile's rows (coalesced 16-byte loads, the rows meet in LDS
    // atomics; redundant across the K parts: the tensors are L2-sized) and writes the fragments of its share of the 16-k steps
    __shared__ unsigned s_max[32];
    __shared__ float s_scale[32];
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tid < 32) s_max[tid] = 0u;
    __syncthreads();
    const int row0 = tile * 32;
    const int live = rows - row0 < 32 ? rows - row0 : 32;
    const float* base = wt + (int64_t)row0 * Ktot;
    if ((Ktot & 3) == 0 && !(reinterpret_cast<uintptr_t>(wt) & 15)) {
        const int per_row = Ktot >> 2, n4 = live * per_row;
        for (int i = tid; i < n4; i += 256) {
            const f32x4 v = reinterpret_cast<const f32x4*>(base)[i];
            unsigned m = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) m = max(m, __float_as_uint(v[q]) & 0x7fffffffu);
            atomicMax(&s_max[i / per_row], m);
        }
    } else {
        const int n = live * Ktot;
        for (int i = tid; i < n; i += 256) atomicMax(&s_max[i / Ktot], __float_as_uint(base[i]) & 0x7fffffffu);
    }
    __syncthreads();
    if (tid < 32) {
        const float ci = f16x2_inv(f16x2_exp(s_max[tid]));
        if (blockIdx.y == 0) cinv[row0 + tid] = ci;
        s_scale[tid] = 1.0f / ci;                                     // exact: a power of two
    }
    __syncthreads();
    const int lane = tid & 63;
    const int row = row0 + (lane & 31);
    const float scale = s_scale[lane & 31];
    for (int ks = (int)blockIdx.y * 4 + (tid >> 6); ks < nk; ks += 4 * (int)gridDim.y) {
        const int k0 = taps > 1 ? (ks % taps) * C + (ks / taps) * 16 + 8 * (lane >> 5) : ks * 16 + 8 * (lane >> 5);
        f16x8 h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = (row < rows && k0 + e < Ktot) ? wt[(int64_t)row * Ktot + k0 + e] * scale : 0.f;
            const _Float16 hh = (_Float16)x;
            h[e] = hh;
            l[e] = (_Float16)(x - (float)hh);
        }
        uint4* dst = wt2 + ((int64_t)tile * nk + ks) * 2 * 64 + lane;
        dst[0] = __builtin_bit_cast(uint4, h);
        dst[64] = __builtin_bit_cast(uint4, l);
    }
}

}  // namespace

extern "C" int bcos_split_weights_f16x2_bytes(int rows, int Ktot, int64_t* bytes) {
    if (rows <= 0 || Ktot <= 0 || !bytes) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights_f16x2_bytes: bad argument");
    *bytes = h2_image_bytes(rows, Ktot) + h2_tiles(rows) * 32 * 4;
    return BCOS_OK;
}

extern "C" int bcos_split_weights_f16x2(const float* wt, void* wt2, int rows, int Ktot, void* stream) {
    return bcos_split_weights_f16x2_conv(wt, wt2, rows, 1, Ktot, stream);
}

extern "C" int bcos_split_weights_f16x2_conv(const float* wt, void* wt2, int rows, int taps, int C, void* stream) {
    if (taps <= 0 || C <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights_f16x2: bad argument");
    const int Ktot = taps * C;
    // the kernel walks K channel-chunk-major exactly when this holds (tile_body_h2: kmajor)
    const int ktaps = (taps > 1 && taps <= H2_MAX_TAPS && C % 16 == 0) ? taps : 1;
    if (!wt || !wt2 || rows <= 0 || Ktot <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights_f16x2: bad argument");
    if (reinterpret_cast<uintptr_t>(wt2) & 15) return bcos_set_error(BCOS_E_INVAL, "bcos_split_weights_f16x2: image must be 16-byte aligned");
    const int nk = (Ktot + 15) / 16;
    const int rows_pad = (int)h2_tiles(rows) * 32;
    float* cinv = reinterpret_cast<float*>(static_cast<char*>(wt2) + h2_image_bytes(rows, Ktot));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (one workgroup per 32 rows walks its whole K: beyond ~150 K elements or K > 1024 the two wide launches are faster -- at 2^20
    //  elements the one-launch form cost a ResNet-50 training step 43 us per image, 4.6 ms per step)
    if ((int64_t)rows_pad * Ktot <= 160 * 1024 && Ktot <= 1024) {
        int parts = nk / 8;                                   // two 16-k steps per wave and workgroup
        parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
        hipLaunchKernelGGL(split_weights_h2_fused_kernel, dim3((unsigned)h2_tiles(rows), (unsigned)parts), dim3(256), 0, s, wt,
                           reinterpret_cast<uint4*>(wt2), cinv, rows, Ktot, nk, ktaps, C);
    } else {
        hipLaunchKernelGGL(weight_rowscale_kernel, dim3((unsigned)((rows_pad + 3) / 4)), dim3(256), 0, s, wt, cinv, rows, rows_pad, Ktot);
        const int64_t total = h2_tiles(rows) * nk * 64;
        hipLaunchKernelGGL(split_weights_h2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wt,
                           reinterpret_cast<uint4*>(wt2), cinv, rows, Ktot, nk, total, ktaps, C);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("split_weights_f16x2 launch", err);
    return BCOS_OK;
}

// ---- banks + images of many layers from one call (bcos_weight_prep_batch) ---------------------------------------------------------------
namespace {
constexpr int PREP_KCH = 1024;          // bank elements of a row per workgroup of the gather
// (1) grid (32-row tile x K part, jobs): gather the part's elements of the tile's rows from the strided source into the bank (coalesced
//     along K) and fold their maxima into row_max[job.row_offset + row] (zero-filled by the caller): per thread, per wave, then ONE atomic per
//     row and workgroup.
__global__ __launch_bounds__(256) void weight_prep_gather_kernel(const bcos_weight_prep_job* __restrict__ jobs, unsigned* __restrict__ row_max) {
    const bcos_weight_prep_job& jb = jobs[blockIdx.y];
    const int rows = jb.rows, Cp = jb.Cp, channels = jb.channels;
    const int Ktot = jb.taps * Cp;
    const int kparts = (Ktot + PREP_KCH - 1) / PREP_KCH;
    const int tile = (int)blockIdx.x / kparts, kpart = (int)blockIdx.x - tile * kparts;
    const int row0 = tile * 32;
    if (row0 >= rows) return;
    const int live = rows - row0 < 32 ? rows - row0 : 32;
    const int k_lo = kpart * PREP_KCH, k_hi = k_lo + PREP_KCH < Ktot ? k_lo + PREP_KCH : Ktot;
    const float* __restrict__ src = jb.src;
    float* __restrict__ bank = jb.bank;
    const int tid = threadIdx.x;
    // (t, c) of this thread's elements do not depend on the row: decoded once
    int off[PREP_KCH / 256];
    bool in[PREP_KCH / 256];
#pragma unroll
    for (int q = 0; q < PREP_KCH / 256; ++q) {
        const int k = k_lo + q * 256 + tid;
        const int t = k / Cp, c = k - t * Cp;
        in[q] = k < k_hi && c < channels && t < jb.taps;
        off[q] = in[q] ? c * jb.ch_stride + jb.tap_offset[t] : 0;
    }
    // rows in groups of eight: eight independent loads in flight per thread and K part, then the stores and the rows' maxima
#pragma unroll
    for (int q = 0; q < PREP_KCH / 256; ++q) {
        const int k = k_lo + q * 256 + tid;
        if (k_lo + q * 256 >= k_hi) break;
        for (int r0 = 0; r0 < live; r0 += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = (in[q] && r0 + u < live) ? src[(int64_t)(row0 + r0 + u) * jb.row_stride + off[q]] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (r0 + u < live) {            // (uniform over the workgroup)
                    if (k < k_hi) bank[(int64_t)(row0 + r0 + u) * Ktot + k] = v[u];
                    const unsigned m = wave_max_u32(k < k_hi ? absbits(v[u]) : 0u);
                    if ((tid & 63) == 0 && m) atomicMax(row_max + jb.row_offset + row0 + r0 + u, m);
                }
            }
        }
    }
}

// (2) grid (32-row tile x group of 16-k steps, jobs): the image of the bank -- the arithmetic of weight_rowscale_kernel + split_weights_h2_kernel
//     on the bank's values and the rows' maxima: that pair's image bit for bit.
__global__ __launch_bounds__(256) void weight_prep_split_kernel(const bcos_weight_prep_job* __restrict__ jobs, const unsigned* __restrict__ row_max) {
    const bcos_weight_prep_job& jb = jobs[blockIdx.y];
    if (jb.image == nullptr) return;
    const int rows = jb.rows, taps = jb.taps, Cp = jb.Cp;
    const int Ktot = taps * Cp;
    const int nk = (Ktot + 15) / 16;
    constexpr int KS_PER_WG = PREP_KCH / 16;                    // 64 steps (16 per wave)
    const int kgroups = (nk + KS_PER_WG - 1) / KS_PER_WG;
    const int tiles = (int)h2_tiles(rows);                       // (the image is padded to a multiple of 128 rows: empty tiles hold zeros)
    const int tile = (int)blockIdx.x / kgroups, kgroup = (int)blockIdx.x - tile * kgroups;
    if (tile >= tiles) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = tile * 32 + (lane & 31);
    const float ci = f16x2_inv(f16x2_exp(row < rows ? row_max[jb.row_offset + row] : 0u));
    const float scale = 1.0f / ci;                                // exact: a power of two
    uint4* wt2 = reinterpret_cast<uint4*>(jb.image);
    if (kgroup == 0 && tid < 32) reinterpret_cast<float*>(static_cast<char*>(jb.image) + h2_image_bytes(rows, Ktot))[tile * 32 + tid] = ci;
    const float* __restrict__ bank = jb.bank;
    const int ktaps = (taps > 1 && taps <= H2_MAX_TAPS && Cp % 16 == 0) ? taps : 1;      // (bcos_split_weights_f16x2_conv: channel-chunk-major K)
    const int ks_hi = (kgroup + 1) * KS_PER_WG < nk ? (kgroup + 1) * KS_PER_WG : nk;
    for (int ks = kgroup * KS_PER_WG + (tid >> 6); ks < ks_hi; ks += 4) {
        const int k0 = ktaps > 1 ? (ks % ktaps) * Cp + (ks / ktaps) * 16 + 8 * (lane >> 5) : ks * 16 + 8 * (lane >> 5);
        f16x8 h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = (row < rows && k0 + e < Ktot) ? bank[(int64_t)row * Ktot + k0 + e] * scale : 0.f;
            const _Float16 hh = (_Float16)x;
            h[e] = hh;
            l[e] = (_Float16)(x - (float)hh);
        }
        uint4* dst = wt2 + ((int64_t)tile * nk + ks) * 2 * 64 + lane;
        dst[0] = __builtin_bit_cast(uint4, h);
        dst[64] = __builtin_bit_cast(uint4, l);
    }
}
}  // namespace

extern "C" int bcos_weight_prep_batch(const bcos_weight_prep_job* jobs, int njobs, int max_rows, int max_ktot, uint32_t* row_max, void* stream) {
    if (!jobs || !row_max || njobs <= 0 || njobs > 65535 || max_rows <= 0 || max_ktot <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_weight_prep_batch: bad argument");
    if (reinterpret_cast<uintptr_t>(jobs) & 7) return bcos_set_error(BCOS_E_INVAL, "bcos_weight_prep_batch: job table must be 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t tiles = h2_tiles(max_rows);
    const int64_t kparts = ((int64_t)max_ktot + PREP_KCH - 1) / PREP_KCH;
    if (tiles * kparts > 0x7fffffff) return bcos_set_error(BCOS_E_NOSUP, "bcos_weight_prep_batch: too large");
    hipLaunchKernelGGL(weight_prep_gather_kernel, dim3((unsigned)(tiles * kparts), (unsigned)njobs), dim3(256), 0, s, jobs, row_max);
    hipLaunchKernelGGL(weight_prep_split_kernel, dim3((unsigned)(tiles * kparts), (unsigned)njobs), dim3(256), 0, s, jobs, row_max);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("weight_prep_batch launch", err);
    return BCOS_OK;
}
