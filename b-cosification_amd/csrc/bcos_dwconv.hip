// bcos_dwconv.hip -- depthwise 7x7 B-cos convolution (stride 1, zero padding 3) on NHWC fp32 for gfx950: the first layer of a ConvNeXt
// block (bcos/models/convnext.py), forward and explanation-mode input gradient.  include/bcos_hip.h states the arithmetic.
//
// One filter per channel leaves the matrix pipe nothing to contract, so this is a vector kernel.  A workgroup of 256 threads owns an
// 8 x 8 spatial tile of one image and a slice of 64 channels:
//   * lanes run along channels: thread = (channel lane cl = tid & 15: channels 4 cl .. 4 cl + 3 of the slice, pixel slot = tid >> 4),
//     every global and LDS access is a float4;
//   * the 14 x 14 x 64 input patch (tile + halo of 3, zeros outside the image and behind the last channel) is staged in LDS once,
//     the slice's 49 x 64 filter taps next to it (backward: taps flipped, patch = mul * gy);
//   * a slot computes 4 neighbouring outputs of one tile row: per tap row it reads 10 patch values and 7 taps from LDS and issues
//     4 x 7 x 8 FMAs on them (a register sliding window: 17 LDS reads per 224 FMAs instead of 98);
//   * a pixel of the patch is 256 bytes = one LDS bank row, so the 16 lanes of every ds_read_b128 lane group cover 64 distinct banks
//     whichever slots they belong to: no bank conflicts, no padding.
// LDS: 14 * 14 * 256 + 49 * 256 = 62720 bytes, static (16-byte aligned by declaration).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int TPB = 256;
constexpr int K = 7, PAD = 3;
constexpr int TILE = 8;                    // output tile, both directions
constexpr int PATCH = TILE + K - 1;        // 14
constexpr int CL = 16;                     // channel lanes (float4 each): 64 channels per workgroup
constexpr int OUTS = 4;                    // outputs per thread, along W
constexpr int SLOTS_W = TILE / OUTS;       // 2 slots across, TPB / CL / SLOTS_W = 8 down
static_assert(TPB / CL == SLOTS_W * TILE, "one slot per tile row and group of OUTS columns");

struct DwArgs {
    const float* in;         // x (forward) / gy (backward)
    const float* w;          // [49, C]
    const float* mul;        // backward: NULL or [N,H,W,C]
    const float* addend;     // backward: NULL or [N,H,W,C]
    float* out;              // y / gx
    float* scale_out;        // forward: NULL or [N,H,W,C]
    float* norm_out;         // forward: NULL or [N,H,W,C]
    int H, W, C, tiles_w, tiles_h, slices;
    float b;
    int plain;               // forward: B == 1, y = lin
};

template <bool BWD>
__global__ __launch_bounds__(TPB) void dwconv7_kernel(const DwArgs a) {
    __shared__ __attribute__((aligned(16))) f32x4 sX[PATCH * PATCH * CL];
    __shared__ __attribute__((aligned(16))) f32x4 sW[K * K * CL];
    const int tid = threadIdx.x;
    const int cl = tid & (CL - 1);
    const int slot = tid >> 4;
    // workgroup -> (image, tile row, tile column, channel slice), slice fastest
    unsigned blk = blockIdx.x;
    const int slice = blk % a.slices;  blk /= a.slices;
    const int tw = blk % a.tiles_w;    blk /= a.tiles_w;
    const int th = blk % a.tiles_h;
    const int n = blk / a.tiles_h;
    const int c = slice * (CL * 4) + cl * 4;
    const bool c_ok = c < a.C;
    const int h0 = th * TILE, w0 = tw * TILE;
    const int64_t img = (int64_t)n * a.H * a.W;

    // filter taps of the slice, read once; the backward walks them flipped, so its body is the forward's
    for (int i = tid; i < K * K * CL; i += TPB) {
        const int t = i / CL, l = i - t * CL;
        const int cc = slice * (CL * 4) + l * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (cc < a.C) v = *reinterpret_cast<const f32x4*>(a.w + (int64_t)(BWD ? K * K - 1 - t : t) * a.C + cc);
        sW[i] = v;
    }
    // input patch with halo
    for (int i = tid; i < PATCH * PATCH * CL; i += TPB) {
        const int p = i / CL, l = i - p * CL;
        const int ph = p / PATCH, pw = p - ph * PATCH;
        const int h = h0 - PAD + ph, w = w0 - PAD + pw;
        const int cc = slice * (CL * 4) + l * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (cc < a.C && h >= 0 && h < a.H && w >= 0 && w < a.W) {
            const int64_t off = (img + (int64_t)h * a.W + w) * a.C + cc;
            v = *reinterpret_cast<const f32x4*>(a.in + off);
            if (BWD && a.mul) v *= *reinterpret_cast<const f32x4*>(a.mul + off);
        }
        sX[i] = v;
    }
    __syncthreads();

    const int ty = slot / SLOTS_W, tx = (slot - ty * SLOTS_W) * OUTS;
    f32x4 lin[OUTS], ss[OUTS];
#pragma unroll
    for (int j = 0; j < OUTS; ++j) { lin[j] = f32x4{0.f, 0.f, 0.f, 0.f}; ss[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // taps in row-major ascending order: one FMA chain per output element and sum.  The tap rows stay a loop: unrolled, the compiler
    // hoists all 7 x 17 LDS reads ahead of the arithmetic and spills
#pragma unroll 1
    for (int r = 0; r < K; ++r) {
        f32x4 xr[OUTS + K - 1], wr[K];
        const f32x4* row = sX + ((ty + r) * PATCH + tx) * CL + cl;
#pragma unroll
        for (int q = 0; q < OUTS + K - 1; ++q) xr[q] = row[q * CL];
#pragma unroll
        for (int s = 0; s < K; ++s) wr[s] = sW[(r * K + s) * CL + cl];
#pragma unroll
        for (int s = 0; s < K; ++s) {
#pragma unroll
            for (int j = 0; j < OUTS; ++j) {
                const f32x4 xv = xr[j + s];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lin[j][e] = fmaf(wr[s][e], xv[e], lin[j][e]);
                    if (!BWD) ss[j][e] = fmaf(xv[e], xv[e], ss[j][e]);
                }
            }
        }
    }

    const int h = h0 + ty;
    if (!c_ok || h >= a.H) return;
#pragma unroll
    for (int j = 0; j < OUTS; ++j) {
        const int w = w0 + tx + j;
        if (w >= a.W) break;
        const int64_t off = (img + (int64_t)h * a.W + w) * a.C + c;
        if (BWD) {
            f32x4 g = lin[j];
            if (a.addend) g = *reinterpret_cast<const f32x4*>(a.addend + off) + g;
            *reinterpret_cast<f32x4*>(a.out + off) = g;
        } else {
            f32x4 y, sc, nr;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                nr[e] = sqrtf(ss[j][e] + 1e-6f);
                sc[e] = a.plain ? 1.f : bcos_scale_of(lin[j][e], nr[e], a.b);
                y[e] = a.plain ? lin[j][e] : sc[e] * lin[j][e];
            }
            *reinterpret_cast<f32x4*>(a.out + off) = y;
            if (a.scale_out) *reinterpret_cast<f32x4*>(a.scale_out + off) = sc;
            if (a.norm_out) *reinterpret_cast<f32x4*>(a.norm_out + off) = nr;
        }
    }
}

// the checks both entry points share (all of them ahead of any HIP call) and the launch shape
int dw_plan(const char* who, const void* in, const void* w, const void* out, const void* opt1, const void* opt2, int N, int H, int W, int C,
            DwArgs& a, unsigned& grid) {
    static thread_local char msg[160];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return bcos_set_error(BCOS_E_INVAL, msg);
    };
    if (!in || !w || !out) return fail("NULL input, filter bank or output");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail("sizes must be positive");
    if (C % 4 != 0) return fail("C % 4 != 0 (lanes move four channels)");
    if (misaligned16(in) || misaligned16(w) || misaligned16(out) || misaligned16(opt1) || misaligned16(opt2))
        return fail("every pointer must be 16-byte aligned");
    a.H = H; a.W = W; a.C = C;
    a.tiles_h = (H + TILE - 1) / TILE;
    a.tiles_w = (W + TILE - 1) / TILE;
    a.slices = (C + CL * 4 - 1) / (CL * 4);
    const int64_t blocks = (int64_t)N * a.tiles_h * a.tiles_w * a.slices;
    if (blocks > 0x7fffffffLL) return fail("more than 2^31 - 1 workgroups");
    grid = (unsigned)blocks;
    return BCOS_OK;
}

}  // namespace

extern "C" int bcos_dwconv7_fwd(const float* x, const float* w, float* y, float* scale_out, float* norm_out, int N, int H, int W, int C,
                                float b, void* stream) {
    DwArgs a{};
    unsigned grid = 0;
    if (int rc = dw_plan("bcos_dwconv7_fwd", x, w, y, scale_out, norm_out, N, H, W, C, a, grid)) return rc;
    if (b == 1.0f && scale_out) return bcos_set_error(BCOS_E_INVAL, "bcos_dwconv7_fwd: B = 1 has no scale to keep (scale_out must be NULL)");
    a.in = x; a.w = w; a.out = y; a.scale_out = scale_out; a.norm_out = norm_out; a.b = b; a.plain = b == 1.0f;
    hipLaunchKernelGGL(dwconv7_kernel<false>, dim3(grid), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), a);
    return check_launch("dwconv7_kernel<fwd>");
}

extern "C" int bcos_dwconv7_bwd(const float* gy, const float* w, const float* mul, const float* addend, float* gx, int N, int H, int W, int C,
                                void* stream) {
    DwArgs a{};
    unsigned grid = 0;
    if (int rc = dw_plan("bcos_dwconv7_bwd", gy, w, gx, mul, addend, N, H, W, C, a, grid)) return rc;
    a.in = gy; a.w = w; a.mul = mul; a.addend = addend; a.out = gx;
    hipLaunchKernelGGL(dwconv7_kernel<true>, dim3(grid), dim3(TPB), 0, reinterpret_cast<hipStream_t>(stream), a);
    return check_launch("dwconv7_kernel<bwd>");
}
