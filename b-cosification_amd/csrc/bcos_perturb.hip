// bcos_perturb.hip -- the device side of the pixel-perturbation (deletion) analysis: an image's pixels are ranked by their attribution, the
// first k of the ranking are removed (all six channels of the [r,g,b,1-r,1-g,1-b] input set to 0, as an Occlusion mask does) and the
// explained class's score is recorded for K removal counts.  The ranking semantics -- key32, key64, thr(k) -- are stated once, in
// include/bcos_hip.h; everything here refers to them.
//   bcos_perturb_select        thr(k) of every image for K counts: an exact radix select on key32 (four 8-bit passes, integer
//                              histograms) and one ordered scan that breaks the tie among equal key32 by ascending pixel index;
//   bcos_prep_input_perturbed  the PREPARED network input of copies [first, first + n) of the B * K perturbed copies straight from the
//                              B source images -- the masked batch never exists in input layout;
//   bcos_class_scores          the explained class's logit / sigmoid / softmax of every copy, from logits that never left the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_K = 64;                      // BCOS_PERTURB_MAX_COUNTS
constexpr int KC = 16;                         // targets per workgroup of a histogram pass: 16 x 256 bins of LDS
constexpr unsigned ALL = 0xFFFFFFFFu;          // rank of a target with k = HW: thr = UINT64_MAX, it takes no part in the passes

struct Counts {
    int32_t k[MAX_K];
};

__device__ __forceinline__ unsigned key32_of(float s, unsigned flip) {
    const unsigned b = __float_as_uint(s);
    return (b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u)) ^ flip;      // flip = 0xFFFFFFFF for "most important first"
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------
// Workspace (32-bit words): hist0 [B][256] | hist [B][K][256] | prefix [B][K] | rank [B][K].
//   zero     clears hist0 and hist (the call never relies on what the workspace held);
//   pass 0   one histogram of the top byte per image (every target starts with the empty prefix);
//   resolve  one wavefront per target: the 256 bins as 4 per lane, an inclusive scan over the lanes, the bin in which the running count
//            passes the target's rank -> prefix = prefix << 8 | bin, rank -= pixels below the bin.  It clears the row it read.
//   pass p   per target the histogram of byte 3 - p over the pixels whose higher bytes equal the target's prefix;
//   tie      one workgroup per (target, image) walks the pixels in ascending order and takes the rank-th whose key32 equals the prefix.
// Histograms are integer counts (LDS atomics per workgroup, flushed with global integer atomics): exact whatever the launch shape.
__global__ __launch_bounds__(TPB) void perturb_zero_kernel(unsigned* __restrict__ ws, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < words; i += stride) ws[i] = 0u;
}

__global__ __launch_bounds__(TPB) void perturb_hist0_kernel(const float* __restrict__ scores, unsigned* __restrict__ hist0, int HW,
                                                            unsigned flip) {
    __shared__ unsigned s_h[256];
    const int b = blockIdx.y;
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const float* s = scores + (int64_t)b * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += stride) atomicAdd(&s_h[key32_of(s[p], flip) >> 24], 1u);
    __syncthreads();
    const unsigned c = s_h[threadIdx.x];
    if (c) atomicAdd(&hist0[(int64_t)b * 256 + threadIdx.x], c);
}

__global__ __launch_bounds__(TPB) void perturb_hist_kernel(const float* __restrict__ scores, const unsigned* __restrict__ prefix,
                                                           const unsigned* __restrict__ rank, unsigned* __restrict__ hist, int HW, int K,
                                                           int pass, unsigned flip) {
    __shared__ unsigned s_h[KC * 256];
    __shared__ unsigned s_pre[KC];
    __shared__ int s_on[KC];
    const int b = blockIdx.y, k0 = blockIdx.z * KC;
    const int nk = min(KC, K - k0);
    for (int i = threadIdx.x; i < KC * 256; i += TPB) s_h[i] = 0u;
    if (threadIdx.x < KC) {
        const bool on = (int)threadIdx.x < nk && rank[(int64_t)b * K + k0 + threadIdx.x] != ALL;
        s_on[threadIdx.x] = on ? 1 : 0;
        s_pre[threadIdx.x] = on ? prefix[(int64_t)b * K + k0 + threadIdx.x] : 0u;
    }
    __syncthreads();
    const int hi_shift = 32 - 8 * pass, byte_shift = 24 - 8 * pass;       // pass in 1..3
    const float* s = scores + (int64_t)b * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += stride) {
        const unsigned key = key32_of(s[p], flip);
        const unsigned hi = key >> hi_shift, byte = (key >> byte_shift) & 255u;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (s_on[j] && s_pre[j] == hi) atomicAdd(&s_h[j * 256 + byte], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nk * 256; i += TPB) {
        const unsigned c = s_h[i];
        if (c) atomicAdd(&hist[((int64_t)b * K + k0) * 256 + i], c);
    }
}

__global__ __launch_bounds__(TPB) void perturb_resolve_kernel(const unsigned* __restrict__ hist0, unsigned* __restrict__ hist,
                                                              unsigned* __restrict__ prefix, unsigned* __restrict__ rank, Counts counts,
                                                              int HW, int K, int pass) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int k = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (k >= K) return;                                                    // (a whole wavefront: no barrier below)
    const int64_t slot = (int64_t)b * K + k;
    unsigned pre = 0u, r;
    if (pass == 0) {
        r = counts.k[k] >= HW ? ALL : (unsigned)counts.k[k];
    } else {
        pre = prefix[slot];
        r = rank[slot];
    }
    if (r == ALL) {
        if (pass == 0 && lane == 0) { prefix[slot] = 0u; rank[slot] = ALL; }
        return;
    }
    unsigned* row = pass == 0 ? nullptr : hist + slot * 256;
    const unsigned* src = (pass == 0 ? hist0 + (int64_t)b * 256 : row) + 4 * lane;      // (the workspace is 8-byte aligned: no 16-byte access)
    const unsigned h[4] = {src[0], src[1], src[2], src[3]};
    if (row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) row[4 * lane + j] = 0u;
    }
    const unsigned mine = h[0] + h[1] + h[2] + h[3];
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    unsigned below = incl - mine;                                          // pixels in the bins of lower lanes
    // exactly one lane holds the bin: below <= r < below + mine (the rank is below the row's total by construction)
    if (below <= r && r < incl) {
        int bin = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (bin == j && r >= below + h[j]) { below += h[j]; bin = j + 1; }
        prefix[slot] = (pre << 8) | (unsigned)(4 * lane + bin);
        rank[slot] = r - below;
    }
}

__global__ __launch_bounds__(TPB) void perturb_tie_kernel(const float* __restrict__ scores, const unsigned* __restrict__ prefix,
                                                          const unsigned* __restrict__ rank, unsigned long long* __restrict__ thr, int HW,
                                                          int K, unsigned flip) {
    __shared__ unsigned s_w[2][TPB / 64];
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t slot = (int64_t)b * K + k;
    const unsigned r = rank[slot], target = prefix[slot];
    if (r == ALL) {                                                        // (uniform)
        if (threadIdx.x == 0) thr[slot] = 0xFFFFFFFFFFFFFFFFull;
        return;
    }
    const float* s = scores + (int64_t)b * HW;
    unsigned seen = 0u;                                                    // pixels with key32 == target below `base`
    int par = 0;
    for (int64_t base = 0; base < HW; base += TPB) {
        const int64_t p = base + threadIdx.x;
        const bool hit = p < HW && key32_of(s[p], flip) == target;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_w[par][wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned offs = seen, tot = 0u;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            const unsigned c = s_w[par][w];
            if (w < wave) offs += c;
            tot += c;
        }
        par ^= 1;
        if (hit && offs + (unsigned)__popcll(bal & ((1ull << lane) - 1ull)) == r) thr[slot] = ((unsigned long long)target << 32) | (unsigned long long)p;
        seen += tot;
        if (seen > r) break;                                               // (uniform: every thread sees the same counts)
    }
}

// ---- prepared input of the perturbed copies ----------------------------------------------------------------------------------------------
// One thread per output pixel, as prep_input_kernel (bcos_elementwise.hip) and with its arithmetic: o = (v - mean) / std with v = 0 for a
// removed pixel and the source value otherwise, so the bits are those of bcos_prep_input on the materialised copy.  Source pixel and score
// are re-read per copy out of L2.
__global__ __launch_bounds__(TPB) void prep_input_perturbed_kernel(const float* __restrict__ x, const float* __restrict__ scores,
                                                                   const unsigned long long* __restrict__ thr, float* __restrict__ out,
                                                                   const float* __restrict__ mean6, const float* __restrict__ std6,
                                                                   unsigned* __restrict__ absmax, int K, int first, int n, int HW, int Cpad,
                                                                   unsigned flip) {
    const int64_t total = (int64_t)n * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    float mu[6], sd[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { mu[c] = mean6[c]; sd[c] = std6[c]; }
    const bool wide = Cpad == 8 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / HW;
        const int hw = (int)(i - m * HW);
        const int64_t copy = first + m;
        const int64_t b = copy / K;
        const unsigned long long key = ((unsigned long long)key32_of(scores[b * HW + hw], flip) << 32) | (unsigned)hw;
        const bool removed = key < thr[copy];
        const float* src = x + b * 6 * HW + hw;
        float* dst = out + i * Cpad;
        unsigned mx = 0u;
        float o[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float v = removed ? 0.0f : src[(int64_t)c * HW];
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

// ---- score of the explained class ----------------------------------------------------------------------------------------------------------
// One wavefront per row.  Softmax: lane l takes the classes l, l + 64, ... in ascending order (max, then the sum of expf(x - max) as one
// fp32 chain per lane); the 64 lane values are combined by the butterfly xor 32, 16, 8, 4, 2, 1 -- a fixed tree, the same on every lane.
__global__ __launch_bounds__(TPB) void class_scores_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                           float* __restrict__ out, int64_t R, int CL, int group, int mode) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    const int t = targets[r / group];
    const float* row = logits + r * CL;
    float res;
    if (t < 0 || t >= CL) {
        res = __uint_as_float(0x7fc00000u);                                  // a class outside the logits: NaN, never an out-of-bounds read
    } else if (mode == 0) {
        res = row[t];
    } else if (mode == 1) {
        res = 1.0f / (1.0f + expf(-row[t]));
    } else {
        float mx = -INFINITY;
        for (int c = lane; c < CL; c += 64) mx = fmaxf(mx, row[c]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
        float sum = 0.f;
        for (int c = lane; c < CL; c += 64) sum += expf(row[c] - mx);
        sum = wave_sum(sum);
        res = expf(row[t] - mx) / sum;
    }
    if (lane == 0) out[r] = res;
}

inline int64_t select_words(int64_t B, int64_t K) { return B * 256 + B * K * 256 + 2 * B * K; }

inline bool select_shape_ok(int B, int64_t HW, int K) {
    return B >= 1 && B <= 65535 && HW >= 1 && HW <= INT32_MAX && K >= 1 && K <= MAX_K;      // (B <= 65535: grid.y; it bounds the workspace too)
}

}  // namespace

extern "C" int bcos_perturb_select_ws_bytes(int B, int64_t HW, int K, int64_t* bytes) {
    if (!bytes) return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select_ws_bytes: NULL pointer");
    if (!select_shape_ok(B, HW, K))
        return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select_ws_bytes: need 1 <= B <= 65535, 1 <= HW <= 2^31 - 1, 1 <= K <= 64");
    *bytes = 4 * select_words(B, K);
    return BCOS_OK;
}

extern "C" int bcos_perturb_select(const float* scores, const int32_t* counts_host, int descending, uint64_t* thr_out, void* ws,
                                   int64_t ws_bytes, int B, int64_t HW, int K, void* stream) {
    if (!scores || !counts_host || !thr_out || !ws) return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select: NULL pointer");
    if (!select_shape_ok(B, HW, K))
        return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select: need 1 <= B <= 65535, 1 <= HW <= 2^31 - 1, 1 <= K <= 64");
    Counts counts;
    for (int k = 0; k < MAX_K; ++k) counts.k[k] = 0;
    for (int k = 0; k < K; ++k) {
        if (counts_host[k] < 0 || counts_host[k] > HW) return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select: a count outside [0, HW]");
        counts.k[k] = counts_host[k];
    }
    const int64_t words = select_words(B, K);
    if (ws_bytes < 4 * words) return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select: ws_bytes is below bcos_perturb_select_ws_bytes");
    if ((reinterpret_cast<uintptr_t>(thr_out) & 7) || (reinterpret_cast<uintptr_t>(ws) & 7))
        return bcos_set_error(BCOS_E_INVAL, "bcos_perturb_select: thr_out and ws must be 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned* hist0 = static_cast<unsigned*>(ws);
    unsigned* hist = hist0 + (int64_t)B * 256;
    unsigned* prefix = hist + (int64_t)B * K * 256;
    unsigned* rank = prefix + (int64_t)B * K;
    const int hw = (int)HW;
    const unsigned flip = descending ? 0xFFFFFFFFu : 0u;
    const int64_t zero_words = (int64_t)B * 256 * (K + 1);
    int64_t zb = (zero_words + TPB - 1) / TPB;
    if (zb > 4096) zb = 4096;
    hipLaunchKernelGGL(perturb_zero_kernel, dim3((unsigned)zb), dim3(TPB), 0, st, hist0, zero_words);
    int64_t wgs = (HW + 4 * TPB - 1) / (4 * TPB);                           // pixel workgroups per image (counts do not depend on it)
    if (wgs > 128) wgs = 128;
    const dim3 res_grid((unsigned)((K + TPB / 64 - 1) / (TPB / 64)), (unsigned)B);
    hipLaunchKernelGGL(perturb_hist0_kernel, dim3((unsigned)wgs, (unsigned)B), dim3(TPB), 0, st, scores, hist0, hw, flip);
    hipLaunchKernelGGL(perturb_resolve_kernel, res_grid, dim3(TPB), 0, st, hist0, hist, prefix, rank, counts, hw, K, 0);
    for (int pass = 1; pass < 4; ++pass) {
        hipLaunchKernelGGL(perturb_hist_kernel, dim3((unsigned)wgs, (unsigned)B, (unsigned)((K + KC - 1) / KC)), dim3(TPB), 0, st, scores,
                           prefix, rank, hist, hw, K, pass, flip);
        hipLaunchKernelGGL(perturb_resolve_kernel, res_grid, dim3(TPB), 0, st, hist0, hist, prefix, rank, counts, hw, K, pass);
    }
    hipLaunchKernelGGL(perturb_tie_kernel, dim3((unsigned)K, (unsigned)B), dim3(TPB), 0, st, scores, prefix, rank,
                       reinterpret_cast<unsigned long long*>(thr_out), hw, K, flip);
    return check_launch("bcos_perturb_select kernels");
}

extern "C" int bcos_prep_input_perturbed(const float* x, const float* scores, const uint64_t* thr, int descending, float* out,
                                         const float* mean6, const float* std6, uint32_t* absmax_out, int B, int K, int first, int n, int Cx,
                                         int H, int W, int Cpad, int add_inverse, void* stream) {
    if (!x || !scores || !thr || !out || !mean6 || !std6) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: NULL pointer");
    if (B <= 0 || K <= 0 || H <= 0 || W <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: B, K, H and W must be positive");
    if (add_inverse || Cx != 6)
        return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: only the 6-channel input (masking before AddInverse is another operator)");
    if (Cpad < 6) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: Cpad < 6");
    if ((int64_t)H * W > INT32_MAX) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: H * W exceeds 2^31 - 1");
    if (first < 0 || n <= 0 || (int64_t)first + n > (int64_t)B * K)
        return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: copies [first, first + n) leave the B * K copies");
    if ((int64_t)n > INT64_MAX / ((int64_t)H * W) / Cpad || (int64_t)B > INT64_MAX / ((int64_t)H * W) / 6)
        return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: n * H * W * Cpad or B * 6 * H * W overflows");
    if (reinterpret_cast<uintptr_t>(thr) & 7) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_perturbed: thr must be 8-byte aligned");
    const int64_t total = (int64_t)n * H * W;
    int64_t blocks = (total + TPB - 1) / TPB;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(prep_input_perturbed_kernel, dim3((unsigned)blocks), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), x, scores,
                       reinterpret_cast<const unsigned long long*>(thr), out, mean6, std6, absmax_out, K, first, n, H * W, Cpad,
                       descending ? 0xFFFFFFFFu : 0u);
    return check_launch("prep_input_perturbed_kernel");
}

extern "C" int bcos_class_scores(const float* logits, const int32_t* targets, int group, int mode, float* out, int64_t R, int CL,
                                 void* stream) {
    if (!logits || !targets || !out) return bcos_set_error(BCOS_E_INVAL, "bcos_class_scores: NULL pointer");
    if (R <= 0 || CL <= 0 || group <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_class_scores: R, CL and group must be positive");
    if (R % group) return bcos_set_error(BCOS_E_INVAL, "bcos_class_scores: R is not a multiple of group");
    if (mode < 0 || mode > 2) return bcos_set_error(BCOS_E_INVAL, "bcos_class_scores: mode must be 0 (logit), 1 (sigmoid) or 2 (softmax)");
    if (R > INT64_MAX / CL || (R + TPB / 64 - 1) / (TPB / 64) > INT32_MAX)
        return bcos_set_error(BCOS_E_INVAL, "bcos_class_scores: R * CL overflows or R exceeds 2^33");
    hipLaunchKernelGGL(class_scores_kernel, dim3((unsigned)((R + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0,
                       reinterpret_cast<hipStream_t>(stream), logits, targets, out, R, CL, group, mode);
    return check_launch("class_scores_kernel");
}
