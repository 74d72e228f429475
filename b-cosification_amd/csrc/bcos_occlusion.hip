// bcos_occlusion.hip -- the two device halves of the Occlusion baseline explainer (interpretability/explanation_methods/explainers/
// occlusion.py of the reference).  The reference multiplies one image by a bank of 0/1 masks ([n_masks, 6, H, W], occlusion.py:80), runs
// the network on the copies, moves every logit row to the host and builds `participated * diff / n_part` as [n_masks, classes, H, W] there
// before summing over the masks (occlusion.py:93-108).  Its masks are rectangles (occlusion.py:46-49), so here a mask is four integers:
//   bcos_prep_input_occluded   writes the PREPARED network input of n occluded copies straight from the one source image -- the masked
//                              batch never exists in input layout;
//   bcos_occlusion_accumulate  sums, per output pixel and class, the logit drops of the masks that cover the pixel, in ascending mask order,
//                              from logits that never left the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TPB = 256;

// ---- prepared input of n occluded copies of one 6-channel image ---------------------------------------------------------------------
// One thread per output pixel, as prep_input_kernel (bcos_elementwise.hip) and with its arithmetic: o = (v - mean) / std on v = x * keep,
// keep = 0 inside the copy's rectangle and 1 outside -- the product the reference forms before the network normalises it, so the bits
// are those of bcos_prep_input on the materialised copy.  The source image (6 * H * W floats) is re-read per copy out of L2.
__global__ __launch_bounds__(TPB) void prep_input_occluded_kernel(const float* __restrict__ x, const i32x4* __restrict__ rects,
                                                                  float* __restrict__ out, const float* __restrict__ mean6,
                                                                  const float* __restrict__ std6, unsigned* __restrict__ absmax,
                                                                  int n, int HW, int W, int Cpad) {
    const int64_t total = (int64_t)n * HW;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    float mu[6], sd[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { mu[c] = mean6[c]; sd[c] = std6[c]; }
    const bool wide = Cpad == 8 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / HW;
        const int hw = (int)(i - m * HW);
        const int h = hw / W, w = hw - h * W;
        const i32x4 r = rects[m];
        const float keep = (h >= r[0] && h < r[1] && w >= r[2] && w < r[3]) ? 0.0f : 1.0f;
        const float* src = x + hw;
        float* dst = out + i * Cpad;
        unsigned mx = 0u;
        float o[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float v = src[(int64_t)c * HW] * keep;
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

// ---- per-pixel sum over the masks ----------------------------------------------------------------------------------------------------
// A workgroup owns a tile of ACC_TH x ACC_TW pixels (one pixel per thread; a wavefront covers 2 rows x 32 columns, so a store of one class
// is two full 128-byte lines) and a slice of the classes, which it walks in chunks of ACC_TC held in registers.
//   fill     the bank is scanned ONCE in ascending order, 256 rectangles per step (four steps' loads in flight); those that touch the
//            tile are compacted -- in order: ballot + prefix counts -- into an LDS list (rectangle, mask index, area).  For the named
//            configurations a tile meets ~160 of 12,544 rectangles, so the list (ACC_LCAP) holds them all and serves every class chunk;
//            when a bank overfills it, the list is consumed and the scan resumes behind the last block taken, per class chunk.
//   consume  ACC_SUB list entries at a time: their terms d / n_part for the chunk's classes are formed once, cooperatively (coalesced
//            along the classes), into LDS; every thread then walks the entries in list order and adds an entry's ACC_TC terms if the
//            rectangle holds its pixel (a wavefront whose pixels all lie outside skips the entry).
// Every output element is therefore one fp32 chain over its covering masks in ascending m, whatever T, the grid or the list capacity.
constexpr int ACC_TH = 8, ACC_TW = 32;
constexpr int ACC_TC = 32;
constexpr int ACC_LCAP = 768;
constexpr int ACC_SUB = 128;
constexpr int ACC_AHEAD = 4;

struct AccEntry {
    int r0, r1, c0, c1;
};

__global__ __launch_bounds__(TPB) void occlusion_accumulate_kernel(const float* __restrict__ org, const float* __restrict__ pert,
                                                                   const i32x4* __restrict__ rects, const int32_t* __restrict__ targets,
                                                                   float* __restrict__ out, int n, int CL, int T, int H, int W,
                                                                   int chunks_per_slice, int only_positive) {
    __shared__ AccEntry s_rect[ACC_LCAP];
    __shared__ int s_m[ACC_LCAP];
    __shared__ float s_area[ACC_LCAP];
    __shared__ __attribute__((aligned(16))) float s_d[ACC_SUB][ACC_TC];      // (read as 16-byte vectors)
    __shared__ int s_wtot[2][TPB / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int th0 = blockIdx.y * ACC_TH, tw0 = blockIdx.x * ACC_TW;
    const int h = th0 + wave * 2 + (lane >> 5), w = tw0 + (lane & 31);
    const bool live = h < H && w < W;
    const int nchunks = (T + ACC_TC - 1) / ACC_TC;
    const int chunk_lo = blockIdx.z * chunks_per_slice;
    const int chunk_hi = min(nchunks, chunk_lo + chunks_per_slice);

    int cnt = 0;                     // entries in the list
    bool whole = false;              // the list holds every rectangle of the bank that touches the tile: no further scan
    for (int chunk = chunk_lo; chunk < chunk_hi; ++chunk) {
        const int t0 = chunk * ACC_TC;
        float acc[ACC_TC];
#pragma unroll
        for (int k = 0; k < ACC_TC; ++k) acc[k] = 0.f;
        int pos = 0;
        bool done;
        do {
            if (!whole) {            // ---- fill from `pos` (a whole list from an earlier chunk is consumed again as it stands)
                const int start = pos;
                cnt = 0;
                int par = 0;
                bool full = false;
                while (pos < n && !full) {
                    i32x4 r[ACC_AHEAD];
#pragma unroll
                    for (int u = 0; u < ACC_AHEAD; ++u) {
                        const int idx = pos + u * TPB + tid;
                        r[u] = idx < n ? rects[idx] : i32x4{0, 0, 0, 0};
                    }
                    const int pos0 = pos;
#pragma unroll
                    for (int u = 0; u < ACC_AHEAD; ++u) {
                        const int base = pos0 + u * TPB;
                        if (base >= n) break;
                        const int idx = base + tid;
                        const bool hit = idx < n && r[u][0] < r[u][1] && r[u][2] < r[u][3] && r[u][0] < th0 + ACC_TH && r[u][1] > th0 &&
                                         r[u][2] < tw0 + ACC_TW && r[u][3] > tw0;
                        const unsigned long long bal = __ballot(hit);
                        if (lane == 0) s_wtot[par][wave] = __popcll(bal);
                        __syncthreads();
                        int offs = cnt, tot = 0;
#pragma unroll
                        for (int k = 0; k < TPB / 64; ++k) {
                            const int c = s_wtot[par][k];
                            if (k < wave) offs += c;
                            tot += c;
                        }
                        par ^= 1;
                        if (cnt + tot > ACC_LCAP) {          // (uniform: every thread sees the same counts); cnt > 0 here, ACC_LCAP >= TPB
                            full = true;
                            break;
                        }
                        if (hit) {
                            const int slot = offs + __popcll(bal & ((1ull << lane) - 1ull));
                            s_rect[slot] = AccEntry{r[u][0], r[u][1], r[u][2], r[u][3]};
                            s_m[slot] = idx;
                            s_area[slot] = (float)(r[u][1] - r[u][0]) * (float)(r[u][3] - r[u][2]);
                        }
                        cnt += tot;
                        pos = base + TPB;
                    }
                }
                whole = start == 0 && pos >= n;
            }
            done = whole || pos >= n;
            // ---- consume the list
            for (int jb = 0; jb < cnt; jb += ACC_SUB) {
                const int nj = min(ACC_SUB, cnt - jb);
                __syncthreads();                                   // the list is written; the previous sub-batch's terms are read
                for (int jj = tid >> 5; jj < nj; jj += TPB / 32) {
                    const int tc = tid & 31, t = t0 + tc;
                    float v = 0.f;
                    if (t < T) {
                        const int cls = targets ? targets[t] : t;
                        if (cls < 0 || cls >= CL) {
                            v = __uint_as_float(0x7fc00000u);      // a class outside the logits: NaN, never an out-of-bounds read
                        } else {
                            float d = org[cls] - pert[(int64_t)s_m[jb + jj] * CL + cls];
                            if (only_positive) d = d < 0.f ? 0.f : d;      // clamp(0) as torch's: a NaN stays NaN
                            v = d / s_area[jb + jj];
                        }
                    }
                    s_d[jj][tc] = v;
                }
                __syncthreads();
                for (int jj = 0; jj < nj; ++jj) {
                    const AccEntry e = s_rect[jb + jj];
                    if (h >= e.r0 && h < e.r1 && w >= e.c0 && w < e.c1) {
#pragma unroll
                        for (int k = 0; k < ACC_TC; k += 4) {
                            const f32x4 d4 = *reinterpret_cast<const f32x4*>(&s_d[jj][k]);
                            acc[k] += d4[0];
                            acc[k + 1] += d4[1];
                            acc[k + 2] += d4[2];
                            acc[k + 3] += d4[3];
                        }
                    }
                }
            }
            __syncthreads();                                       // before the list or the terms are overwritten
        } while (!done);
        if (live) {
#pragma unroll
            for (int k = 0; k < ACC_TC; ++k)
                if (t0 + k < T) out[((int64_t)(t0 + k) * H + h) * W + w] = acc[k];
        }
    }
}

}  // namespace

extern "C" int bcos_prep_input_occluded(const float* x, const int32_t* rects, float* out, const float* mean6, const float* std6,
                                        uint32_t* absmax_out, int n, int Cx, int H, int W, int Cpad, int add_inverse, void* stream) {
    if (!x || !rects || !out || !mean6 || !std6) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: NULL pointer");
    if (n <= 0 || H <= 0 || W <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: n, H and W must be positive");
    if (add_inverse || Cx != 6)
        return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: only the 6-channel input (masking before AddInverse is another operator)");
    if (Cpad < 6) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: Cpad < 6");
    if ((int64_t)H * W > INT32_MAX) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: H * W exceeds 2^31 - 1");
    if ((int64_t)n > INT64_MAX / ((int64_t)H * W) / Cpad) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: n * H * W * Cpad overflows");
    if (reinterpret_cast<uintptr_t>(rects) & 15) return bcos_set_error(BCOS_E_INVAL, "bcos_prep_input_occluded: rects must be 16-byte aligned");
    const int64_t total = (int64_t)n * H * W;
    int64_t blocks = (total + TPB - 1) / TPB;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(prep_input_occluded_kernel, dim3((unsigned)blocks), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), x,
                       reinterpret_cast<const i32x4*>(rects), out, mean6, std6, absmax_out, n, H * W, W, Cpad);
    return check_launch("prep_input_occluded_kernel");
}

extern "C" int bcos_occlusion_accumulate(const float* org, const float* pert, const int32_t* rects, const int32_t* rects_host,
                                         const int32_t* targets, float* out, int n, int CL, int T, int H, int W, int only_positive,
                                         void* stream) {
    if (!org || !pert || !rects || !out) return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: NULL pointer");
    if (n <= 0 || CL <= 0 || T <= 0 || H <= 0 || W <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: n, CL, T, H and W must be positive");
    if (!targets && T != CL) return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: without targets T must equal CL");
    if (reinterpret_cast<uintptr_t>(rects) & 15) return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: rects must be 16-byte aligned");
    if ((int64_t)T > INT64_MAX / H / W || (int64_t)n > INT64_MAX / CL || n > INT32_MAX - ACC_AHEAD * TPB)
        return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: T * H * W or n * CL overflows, or n exceeds 2^31 - 1025");
    if (rects_host) {
        for (int m = 0; m < n; ++m) {
            const int32_t* r = rects_host + 4 * (int64_t)m;
            if (r[0] >= r[1] || r[2] >= r[3])
                return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: a rectangle with an empty side (the reference divides 0 by 0)");
            if (r[0] < 0 || r[2] < 0 || r[1] > H || r[3] > W)
                return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: a rectangle that is not clipped to the image");
        }
    }
    const int tiles_w = (W + ACC_TW - 1) / ACC_TW, tiles_h = (H + ACC_TH - 1) / ACC_TH;
    if (tiles_h > 65535) return bcos_set_error(BCOS_E_INVAL, "bcos_occlusion_accumulate: H exceeds 65535 * 8");
    // class slices: enough workgroups for 256 CUs x 8, never more slices than class chunks (the bank scan is per workgroup)
    const int nchunks = (T + ACC_TC - 1) / ACC_TC;
    int64_t slices = (2048 + (int64_t)tiles_w * tiles_h - 1) / ((int64_t)tiles_w * tiles_h);
    if (slices > nchunks) slices = nchunks;
    if (slices < 1) slices = 1;
    const int per = (int)((nchunks + slices - 1) / slices);
    slices = (nchunks + per - 1) / per;
    hipLaunchKernelGGL(occlusion_accumulate_kernel, dim3((unsigned)tiles_w, (unsigned)tiles_h, (unsigned)slices), dim3(TPB), 0,
                       reinterpret_cast<hipStream_t>(stream), org, pert, reinterpret_cast<const i32x4*>(rects), targets, out, n, CL, T, H, W,
                       per, only_positive ? 1 : 0);
    return check_launch("occlusion_accumulate_kernel");
}
