// bcos_dwconv_train.hip -- training-mode gradients of the depthwise 7x7 B-cos convolution of csrc/bcos_dwconv.hip (stride 1, zero padding
// 3, NHWC fp32, gfx950): the input gradient with the B-cos scale differentiated (bcos_dwconv7_train_bwd, one launch) and the gradient of
// the effective filter bank (bcos_dwconv7_wgrad, two launches, no atomics).  include/bcos_hip.h states the arithmetic and every order.
//
// bcos_dwconv7_train_bwd.  The workgroup of the forward kernel: 256 threads, an 8 x 8 tile of one image, a slice of 64 channels, lane =
// (channel lane cl = tid & 15, slot = tid >> 4), a slot owns 4 neighbouring outputs of one tile row and walks the tap rows with a register
// sliding window.  The kernel needs two 14 x 14 patches per slice, glin = 2 scale gy and r = -(gy y) / norm^2; two of them at 64 channels
// are 100352 bytes, more than the 64 KB of static LDS.  Of the two ways out this file takes TWO PASSES OVER ONE PATCH BUFFER: the glin
// patch is staged, the weighted 49-tap sum runs; a barrier; the r patch is staged into the same buffer, the unweighted box sum (adds
// only) runs.  Why not a 32-channel slice: a pixel of 128 bytes is half a bank row, so the four 16-lane groups of a ds_read_b128
// ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32) would each hold lanes of four different slots, two of which share their
// sixteen banks whenever their pixels have the same parity -- conflict-free only under an odd row pitch and a slot order chosen for it --
// and a workgroup would cover half the channels per staged halo.  The second pass costs one more barrier and re-reads gy (L2-resident:
// the same workgroup read it a few microseconds earlier); nothing per element goes to HBM in between.
// LDS banks, redone for this layout: a pixel stays 64 channels x 4 bytes = 256 bytes = one bank row, lane cl reads the 16 bytes at
// 16 cl of its pixel, i.e. banks 4 cl .. 4 cl + 3 whatever the pixel.  Every 16-lane group listed above holds each value of cl = lane & 15
// exactly once (0-3, 12-15, 4-11;  4-11, 0-3, 12-15), so its 16 lanes cover all 64 banks once whichever slots (pixels) they belong to:
// no conflicts in either pass, no padding.  The staging stores (ds_write_b128) are the same addresses lane for lane.
// LDS: 14 * 14 * 256 + 49 * 256 = 62720 bytes, static.
//
// bcos_dwconv7_wgrad.  Stage 1: a workgroup of 224 threads owns a 64-channel slice and a fixed run of (image, 6 x 8 spatial tile) pairs.
// lane = (cl, slot), slot = (tap row r = 0..6, part = 0..1): the thread accumulates gw[r, 0..6, 4 cl..4 cl + 3] (28 registers) over tile
// rows 3 part .. 3 part + 2 of every pair, from the LDS-resident 12 x 14 x patch and 6 x 8 glin tile (43008 + 12288 = 55296 bytes; an
// 8 x 8 tile with its 14 x 14 patch would be 66560).  Both images keep the 256-byte pixel, so the bank argument above holds as it
// stands (the threads of a group that share a glin pixel read the same address: a broadcast).  Each thread writes its 28 sums to the
// workspace [G][2][49][C]; stage 2 adds the 2 G partials of every (tap, channel) in ascending index.  Which pairs a workgroup owns, and
// with it the order of every sum, is a function of (N, H, W, C) alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int K = 7, PAD = 3;
constexpr int CL = 16;                     // channel lanes (float4 each): 64 channels per workgroup
constexpr int SLICE = CL * 4;

// ---- input gradient ---------------------------------------------------------------------------------------------------------------
constexpr int TPB = 256;
constexpr int TILE = 8;
constexpr int PATCH = TILE + K - 1;        // 14
constexpr int OUTS = 4;                    // outputs per thread, along W
constexpr int SLOTS_W = TILE / OUTS;
static_assert(TPB / CL == SLOTS_W * TILE, "one slot per tile row and group of OUTS columns");

struct TrainArgs {
    const float *gy, *x, *y, *scale, *norm, *w, *addend;
    float* gx;
    int H, W, C, tiles_w, tiles_h, slices;
    int plain;               // B == 1: glin = gy, no norm term
};

// the operand of both gradients, rounded the same way in both kernels: one product mul * gy, then the gain (2: exact)
__device__ __forceinline__ f32x4 glin_of(const f32x4 g, const f32x4 m, const float gain) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gain * (m[e] * g[e]);
    return v;
}

__global__ __launch_bounds__(TPB) void dwconv7_train_bwd_kernel(const TrainArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 sP[PATCH * PATCH * CL];
    __shared__ __attribute__((aligned(16))) f32x4 sW[K * K * CL];
    const int tid = threadIdx.x;
    const int cl = tid & (CL - 1);
    const int slot = tid >> 4;
    unsigned blk = blockIdx.x;
    const int slice = blk % a.slices;  blk /= a.slices;
    const int tw = blk % a.tiles_w;    blk /= a.tiles_w;
    const int th = blk % a.tiles_h;
    const int n = blk / a.tiles_h;
    const int c = slice * SLICE + cl * 4;
    const int h0 = th * TILE, w0 = tw * TILE;
    const int64_t img = (int64_t)n * a.H * a.W;
    const int ty = slot / SLOTS_W, tx = (slot - ty * SLOTS_W) * OUTS;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // filter taps of the slice, flipped: the walk below is the forward's
    for (int i = tid; i < K * K * CL; i += TPB) {
        const int t = i / CL, l = i - t * CL;
        const int cc = slice * SLICE + l * 4;
        sW[i] = cc < a.C ? *reinterpret_cast<const f32x4*>(a.w + (int64_t)(K * K - 1 - t) * a.C + cc) : zero;
    }
    // pass 1: glin = 2 (scale gy) with halo, zeros outside the image and behind the last channel
    for (int i = tid; i < PATCH * PATCH * CL; i += TPB) {
        const int p = i / CL, l = i - p * CL;
        const int ph = p / PATCH, pw = p - ph * PATCH;
        const int h = h0 - PAD + ph, w = w0 - PAD + pw;
        const int cc = slice * SLICE + l * 4;
        f32x4 v = zero;
        if (cc < a.C && h >= 0 && h < a.H && w >= 0 && w < a.W) {
            const int64_t off = (img + (int64_t)h * a.W + w) * a.C + cc;
            v = *reinterpret_cast<const f32x4*>(a.gy + off);
            if (!a.plain) v = glin_of(v, *reinterpret_cast<const f32x4*>(a.scale + off), 2.0f);
        }
        sP[i] = v;
    }
    __syncthreads();

    f32x4 acc[OUTS], box[OUTS];
#pragma unroll
    for (int j = 0; j < OUTS; ++j) { acc[j] = zero; box[j] = zero; }
    // (the tap rows stay a loop, as in the forward kernel: unrolled, the LDS reads are hoisted and spill)
#pragma unroll 1
    for (int r = 0; r < K; ++r) {
        f32x4 xr[OUTS + K - 1], wr[K];
        const f32x4* row = sP + ((ty + r) * PATCH + tx) * CL + cl;
#pragma unroll
        for (int q = 0; q < OUTS + K - 1; ++q) xr[q] = row[q * CL];
#pragma unroll
        for (int s = 0; s < K; ++s) wr[s] = sW[(r * K + s) * CL + cl];
#pragma unroll
        for (int s = 0; s < K; ++s) {
#pragma unroll
            for (int j = 0; j < OUTS; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(wr[s][e], xr[j + s][e], acc[j][e]);
            }
        }
    }

    if (!a.plain) {
        __syncthreads();                   // every slot is done with the glin patch
        // pass 2: r = -(gy y) / (norm norm) into the same buffer
        for (int i = tid; i < PATCH * PATCH * CL; i += TPB) {
            const int p = i / CL, l = i - p * CL;
            const int ph = p / PATCH, pw = p - ph * PATCH;
            const int h = h0 - PAD + ph, w = w0 - PAD + pw;
            const int cc = slice * SLICE + l * 4;
            f32x4 v = zero;
            if (cc < a.C && h >= 0 && h < a.H && w >= 0 && w < a.W) {
                const int64_t off = (img + (int64_t)h * a.W + w) * a.C + cc;
                const f32x4 g = *reinterpret_cast<const f32x4*>(a.gy + off);
                const f32x4 yy = *reinterpret_cast<const f32x4*>(a.y + off);
                const f32x4 nr = *reinterpret_cast<const f32x4*>(a.norm + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = -(g[e] * yy[e]) / (nr[e] * nr[e]);
            }
            sP[i] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < K; ++r) {
            f32x4 xr[OUTS + K - 1];
            const f32x4* row = sP + ((ty + r) * PATCH + tx) * CL + cl;
#pragma unroll
            for (int q = 0; q < OUTS + K - 1; ++q) xr[q] = row[q * CL];
#pragma unroll
            for (int s = 0; s < K; ++s) {
#pragma unroll
                for (int j = 0; j < OUTS; ++j) box[j] += xr[j + s];
            }
        }
    }

    const int h = h0 + ty;
    if (c >= a.C || h >= a.H) return;
#pragma unroll
    for (int j = 0; j < OUTS; ++j) {
        const int w = w0 + tx + j;
        if (w >= a.W) break;
        const int64_t off = (img + (int64_t)h * a.W + w) * a.C + c;
        f32x4 g = acc[j];
        if (!a.plain) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = fmaf(xv[e], box[j][e], g[e]);
        }
        if (a.addend) g = *reinterpret_cast<const f32x4*>(a.addend + off) + g;
        *reinterpret_cast<f32x4*>(a.gx + off) = g;
    }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------
constexpr int WTH = 6, WTW = 8;            // spatial tile of stage 1
constexpr int WPH = WTH + K - 1;           // 12
constexpr int WPW = WTW + K - 1;           // 14
constexpr int PARTS = 2;                   // a part owns WTH / PARTS tile rows
constexpr int PROWS = WTH / PARTS;
constexpr int WTPB = CL * K * PARTS;       // 224
constexpr int WG_MAX = 256;                // workgroups per channel slice at the most
constexpr int HALF = WTW / 2;

struct WgradShape {
    int tiles_h, tiles_w, slices;
    int64_t pairs;           // N tiles_h tiles_w
    int64_t per_wg;          // pairs a workgroup owns: ceil(pairs / WG_MAX)
    int groups;              // G = ceil(pairs / per_wg) <= WG_MAX
};

WgradShape wgrad_shape(int N, int H, int W, int C) {
    WgradShape s;
    s.tiles_h = (H + WTH - 1) / WTH;
    s.tiles_w = (W + WTW - 1) / WTW;
    s.slices = (C + SLICE - 1) / SLICE;
    s.pairs = (int64_t)N * s.tiles_h * s.tiles_w;
    s.per_wg = (s.pairs + WG_MAX - 1) / WG_MAX;
    s.groups = (int)((s.pairs + s.per_wg - 1) / s.per_wg);
    return s;
}

int64_t wgrad_bytes(const WgradShape& s, int C) { return (int64_t)s.groups * PARTS * (K * K) * C * (int64_t)sizeof(float); }

struct WgradArgs {
    const float *gy, *mul, *x;
    float* ws;
    int H, W, C, tiles_w, tiles_h, slices;
    int64_t pairs, per_wg;
    float gain;
};

__global__ __launch_bounds__(WTPB) void dwconv7_wgrad_partial_kernel(const WgradArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 sX[WPH * WPW * CL];
    __shared__ __attribute__((aligned(16))) f32x4 sG[WTH * WTW * CL];
    const int tid = threadIdx.x;
    const int cl = tid & (CL - 1);
    const int slot = tid >> 4;             // 0 .. 13
    const int r = slot >> 1, part = slot & 1;
    const int slice = blockIdx.x % a.slices;
    const int grp = blockIdx.x / a.slices;
    const int c = slice * SLICE + cl * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 acc[K];
#pragma unroll
    for (int s = 0; s < K; ++s) acc[s] = zero;

    const int64_t first = (int64_t)grp * a.per_wg;
    const int64_t last = first + a.per_wg < a.pairs ? first + a.per_wg : a.pairs;
    for (int64_t pair = first; pair < last; ++pair) {
        const int tw = (int)(pair % a.tiles_w);
        const int th = (int)((pair / a.tiles_w) % a.tiles_h);
        const int64_t n = pair / ((int64_t)a.tiles_w * a.tiles_h);
        const int h0 = th * WTH, w0 = tw * WTW;
        const int64_t img = n * a.H * a.W;
        if (pair != first) __syncthreads();          // the previous pair's reads are over
        for (int i = tid; i < WPH * WPW * CL; i += WTPB) {
            const int p = i / CL, l = i - p * CL;
            const int ph = p / WPW, pw = p - ph * WPW;
            const int h = h0 - PAD + ph, w = w0 - PAD + pw;
            const int cc = slice * SLICE + l * 4;
            f32x4 v = zero;
            if (cc < a.C && h >= 0 && h < a.H && w >= 0 && w < a.W)
                v = *reinterpret_cast<const f32x4*>(a.x + (img + (int64_t)h * a.W + w) * a.C + cc);
            sX[i] = v;
        }
        for (int i = tid; i < WTH * WTW * CL; i += WTPB) {
            const int p = i / CL, l = i - p * CL;
            const int ph = p / WTW, pw = p - ph * WTW;
            const int h = h0 + ph, w = w0 + pw;
            const int cc = slice * SLICE + l * 4;
            f32x4 v = zero;
            if (cc < a.C && h < a.H && w < a.W) {
                const int64_t off = (img + (int64_t)h * a.W + w) * a.C + cc;
                v = *reinterpret_cast<const f32x4*>(a.gy + off);
                if (a.mul) v = glin_of(v, *reinterpret_cast<const f32x4*>(a.mul + off), a.gain);
                else if (a.gain != 1.0f) v *= a.gain;
            }
            sG[i] = v;
        }
        __syncthreads();
        // tile rows of this part ascending, columns ascending: one FMA chain per (tap, channel)
#pragma unroll 1
        for (int q = 0; q < PROWS * 2; ++q) {
            const int row = part * PROWS + (q >> 1), col = (q & 1) * HALF;
            f32x4 xr[HALF + K - 1], gl[HALF];
            const f32x4* xrow = sX + ((row + r) * WPW + col) * CL + cl;
            const f32x4* grow = sG + (row * WTW + col) * CL + cl;
#pragma unroll
            for (int j = 0; j < HALF + K - 1; ++j) xr[j] = xrow[j * CL];
#pragma unroll
            for (int j = 0; j < HALF; ++j) gl[j] = grow[j * CL];
#pragma unroll
            for (int j = 0; j < HALF; ++j) {
#pragma unroll
                for (int s = 0; s < K; ++s) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[s][e] = fmaf(gl[j][e], xr[j + s][e], acc[s][e]);
                }
            }
        }
    }
    if (c >= a.C) return;
    float* dst = a.ws + ((int64_t)(grp * PARTS + part) * (K * K) + r * K) * a.C + c;
#pragma unroll
    for (int s = 0; s < K; ++s) *reinterpret_cast<f32x4*>(dst + (int64_t)s * a.C) = acc[s];
}

// gw[i] = sum over the partials 0 .. parts - 1, ascending, of ws[part][i]; one thread per float4
__global__ __launch_bounds__(256) void dwconv7_wgrad_sum_kernel(const float* ws, float* gw, int quads, int parts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(ws) + i;
    f32x4 s = src[0];
    for (int p = 1; p < parts; ++p) s += src[(int64_t)p * quads];
    reinterpret_cast<f32x4*>(gw)[i] = s;
}

thread_local char msg[192];
int fail(const char* who, const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return bcos_set_error(BCOS_E_INVAL, msg);
}

}  // namespace

extern "C" int bcos_dwconv7_train_bwd(const float* gy, const float* x, const float* y, const float* scale, const float* norm, const float* w,
                                      const float* addend, float* gx, int N, int H, int W, int C, float b, void* stream) {
    const char* who = "bcos_dwconv7_train_bwd";
    if (b != 1.0f && b != 2.0f) return fail(who, "only B = 2 and B = 1 are differentiated");
    if (!gy || !w || !gx) return fail(who, "NULL output gradient, filter bank or input gradient");
    if (b == 2.0f && (!x || !y || !scale || !norm)) return fail(who, "B = 2 needs x, y, scale and norm of the forward pass");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(who, "sizes must be positive");
    if (C % 4 != 0) return fail(who, "C % 4 != 0 (lanes move four channels)");
    if (misaligned16(gy) || misaligned16(x) || misaligned16(y) || misaligned16(scale) || misaligned16(norm) || misaligned16(w) ||
        misaligned16(addend) || misaligned16(gx))
        return fail(who, "every pointer must be 16-byte aligned");
    TrainArgs a{};
    a.gy = gy; a.x = x; a.y = y; a.scale = scale; a.norm = norm; a.w = w; a.addend = addend; a.gx = gx;
    a.H = H; a.W = W; a.C = C; a.plain = b == 1.0f;
    a.tiles_h = (H + TILE - 1) / TILE;
    a.tiles_w = (W + TILE - 1) / TILE;
    a.slices = (C + SLICE - 1) / SLICE;
    const int64_t blocks = (int64_t)N * a.tiles_h * a.tiles_w * a.slices;
    if (blocks > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(dwconv7_train_bwd_kernel, dim3((unsigned)blocks), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), a);
    return check_launch("dwconv7_train_bwd_kernel");
}

extern "C" int bcos_dwconv7_wgrad_workspace(int N, int H, int W, int C) {
    const char* who = "bcos_dwconv7_wgrad_workspace";
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return fail(who, "sizes must be positive and C % 4 == 0");
    const int64_t bytes = wgrad_bytes(wgrad_shape(N, H, W, C), C);
    if (bytes > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 bytes of workspace");
    return (int)bytes;
}

extern "C" int bcos_dwconv7_wgrad(const float* gy, const float* mul, float gain, const float* x, float* gw, void* ws, int64_t ws_bytes, int N,
                                  int H, int W, int C, void* stream) {
    const char* who = "bcos_dwconv7_wgrad";
    if (!gy || !x || !gw || !ws) return fail(who, "NULL output gradient, input, weight gradient or workspace");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(who, "sizes must be positive");
    if (C % 4 != 0) return fail(who, "C % 4 != 0 (lanes move four channels)");
    if (misaligned16(gy) || misaligned16(mul) || misaligned16(x) || misaligned16(gw) || misaligned16(ws))
        return fail(who, "every pointer must be 16-byte aligned");
    if (!(gain == gain) || gain - gain != 0.0f) return fail(who, "gain must be finite");
    const WgradShape s = wgrad_shape(N, H, W, C);
    const int64_t need = wgrad_bytes(s, C);
    if (need > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 bytes of workspace");
    if (ws_bytes < need) return fail(who, "workspace smaller than bcos_dwconv7_wgrad_workspace(N, H, W, C)");
    if ((int64_t)s.groups * s.slices > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 workgroups");
    WgradArgs a{};
    a.gy = gy; a.mul = mul; a.x = x; a.ws = static_cast<float*>(ws); a.gain = gain;
    a.H = H; a.W = W; a.C = C; a.tiles_h = s.tiles_h; a.tiles_w = s.tiles_w; a.slices = s.slices; a.pairs = s.pairs; a.per_wg = s.per_wg;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dwconv7_wgrad_partial_kernel, dim3((unsigned)(s.groups * s.slices)), dim3(WTPB), 0, st, a);
    if (int rc = check_launch("dwconv7_wgrad_partial_kernel")) return rc;
    const int quads = K * K * C / 4;
    hipLaunchKernelGGL(dwconv7_wgrad_sum_kernel, dim3((quads + 255) / 256), dim3(256), 0, st, a.ws, gw, quads, s.groups * PARTS);
    return check_launch("dwconv7_wgrad_sum_kernel");
}
