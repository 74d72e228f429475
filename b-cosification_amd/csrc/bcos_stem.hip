// bcos_stem.hip -- the 7 x 7 / stride 2 stem convolution of a ResNet straight from the raw NCHW image (include/bcos_hip.h:
// bcos_stem_conv_fwd).  In the forward pass bcos_prep_input writes the normalised, channel-padded NHWC copy of the image (and its per-pixel
// maxima) and the very next launch, the stem on the LDS-DMA loop of bcos_tapconv.hip (route d_256x64, C = 8: two taps per 16-k step),
// gathers every pixel of that copy about twelve times, 16 bytes per lane, behind one barrier, one counted wait and one DMA issue per step.
// Nothing else reads the copy.  Here a workgroup owns a 16 x 16 block of output pixels of ONE image: it loads the raw pixels of the block's
// (2 * 16 + 5)^2 input patch once (coalesced along the image rows), applies AddInverse and the normalisation of prep_input_kernel in
// registers -- (v - mean) / std, the same expression -- and keeps the fp32 patch in LDS; the K loop then has no barrier and no global A
// traffic, its weight fragments come out of L2 (the pre-split image is 100 KB), prefetched one step ahead.
//
// The result is bit for bit what bcos_prep_input followed by the stem's bcos_tapconv_ops launch gives (tests/test_stem_kernel_gpu.py): a
// row's bits depend on its own window only -- per accumulator the same 25 16-k steps in the same order (step ks = taps 2 ks | 2 ks + 1 in
// the lower | upper half of the wave, tap 49 of the last step all zeros) with the same three products per step (l_a h_b, h_a l_b, h_a h_b),
// the same operand-scale rule (the maximum over the row's 49 taps of the per-pixel maxima, or the image's maximum where the caller hands
// in the per-image range and the image qualifies: tile_body_d's rule), the same split, the patch norm summed as tile_body_d sums it (per
// lane one fma chain over the first and one over the second 16-byte piece of every step, the two added, then the two halves of the wave) and
// the forward epilogue's expressions in its order ([RELU |] [SCALE_OUT]), under contraction off with the two fused operations written as
// explicit fmas, as bcos_shortcut.hip does.  The split, the scale rule and the lane-group maximum are the shared definitions of
// bcos_f16x2.h.
//
// Shape: 256 threads = 4 waves; a wave owns 4 output rows x 16 output columns = two 32-row MFMA blocks (block row r = output row r >> 4,
// column r & 15) x 64 output channels = 4 accumulator tiles.  LDS: the patch as four planes [column parity][channel half] of
// [37 rows][20] 16-byte pieces (a fragment read is two ds_read_b128 whose 16-lane groups each cover 256 contiguous bytes: conflict free)
// + the per-pixel maxima [37][40] = 53 280 bytes: three workgroups fit a CU (130 VGPRs: three waves per SIMD).  Epilogue in ACCUMULATOR layout (register r of a tile is one row,
// the 32 lanes of a half are 32 consecutive channels = 128 contiguous bytes per instruction); t is stored non-temporally, y with the
// default policy (the pool reads it next).
// Measured at batch 256 (profiles/stem_kernel_ab.txt): 635 us with multipliers kept where prep_input + the stem launch (+ the range pass
// over the copy's maxima) took 1 111 us, 562 against 975 us without; 130 VGPRs, no scratch.  What keeps it above its matrix bound
// (0.23 ms) is vector work: the split of every fragment in the wave that multiplies it and the 4-byte stores of the epilogue.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int NT = 256;
constexpr int TP = 16, TQ = 16;             // output pixels of a tile: rows x columns
constexpr int PR = 2 * TP + 5;              // patch rows (37)
constexpr int PC = 2 * TQ + 5;              // patch columns (37)
constexpr int PI = 20;                      // 16-byte pieces per plane row: TQ + 3 used, padded
constexpr int PLANE = PR * PI * 16;         // bytes of one plane
constexpr int PM_LD = 40;                   // words per row of the maxima
constexpr int NK = 25;                      // 16-k steps: K = 49 taps x 8 channels = 392, the last step half empty
constexpr int COUT = 64;
constexpr unsigned OOB = 0x80000000u;       // byte offset beyond every tensor (< 2 GiB): the store is dropped
constexpr unsigned IMG_RANGE_STEP = 16;     // tile_body_d: an image whose nonzero pixel maxima lie within 2^16 of its maximum takes ONE scale

struct StemArgs {
    const float* x; const float* mean6; const float* std6;
    const char* w; const float* cinv; const float* csc; const float* csh;
    float* y; float* t; float* norm_out; unsigned* y_absmax;
    const unsigned* x_imgmax; const unsigned* x_imgmin;
    int N, Cx, H, W, P, Q, tiles_q, relu;
    unsigned lsb;
};

// byte offset of tap t = th * 7 + tw inside the patch planes, relative to the fragment row's base (output pixel (pl, ql): patch row
// 2 pl + th, patch column 2 ql + tw = plane parity tw & 1, piece ql + (tw >> 1))
__device__ __forceinline__ constexpr int tap_off(int t) {
    const int th = t / 7, tw = t % 7;
    return (tw & 1) * 2 * PLANE + (th * PI + (tw >> 1)) * 16;
}

template <bool KEEP>
__global__ __launch_bounds__(NT, 2) void stem_conv_kernel(const StemArgs p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) char lds[4 * PLANE + PR * PM_LD * 4];
    unsigned* pm = reinterpret_cast<unsigned*>(lds + 4 * PLANE);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fhalf = lane >> 5;
    const int n = (int)blockIdx.y;
    const int tile_p = (int)blockIdx.x / p.tiles_q, tile_q = (int)blockIdx.x - tile_p * p.tiles_q;
    const int p0 = tile_p * TP, q0 = tile_q * TQ;
    const int H = p.H, W = p.W, HW = H * W;

    // ---- the patch: raw pixels -> AddInverse, (v - mean) / std -> LDS (pixels outside the image are zeros) ---------------------------
    {
        float mu[6], sd[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) { mu[c] = p.mean6[c]; sd[c] = p.std6[c]; }
        const int ih0 = 2 * p0 - 3, iw0 = 2 * q0 - 3;
        const float* src = p.x + (int64_t)n * p.Cx * HW;
        const bool add_inverse = p.Cx == 3;
        constexpr int NPIX = PR * PC, NIT = (NPIX + NT - 1) / NT;
        float v[NIT][6];
        bool ok[NIT];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = tid + k * NT;
            const int r = i / PC, c = i - r * PC;
            const int ih = ih0 + r, iw = iw0 + c;
            ok[k] = i < NPIX && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
            const float* s = src + (ok[k] ? ih * W + iw : 0);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[k][ch] = ok[k] ? s[ch * HW] : 0.f;
            if (!add_inverse) {
#pragma unroll
                for (int ch = 3; ch < 6; ++ch) v[k][ch] = ok[k] ? s[ch * HW] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = tid + k * NT;
            if (i >= NPIX) break;
            const int r = i / PC, c = i - r * PC;
            if (add_inverse) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[k][ch + 3] = 1.0f - v[k][ch];
            }
            float o[6];
            unsigned m = 0u;
#pragma unroll
            for (int ch = 0; ch < 6; ++ch) {
                o[ch] = (v[k][ch] - mu[ch]) / sd[ch];
                o[ch] = ok[k] ? o[ch] : 0.f;
                m = max(m, absbits(o[ch]));
            }
            char* dst = lds + (c & 1) * 2 * PLANE + (r * PI + (c >> 1)) * 16;
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(dst + PLANE) = f32x4{o[4], o[5], 0.f, 0.f};
            pm[r * PM_LD + c] = m;
        }
    }
    __syncthreads();

    // ---- the rows of this lane's two fragments, their operand scales -----------------------------------------------------------------
    // fragment row frow of block i of this wave = output pixel (4 wave + 2 i + (frow >> 4), frow & 15) of the tile
    bool img_rule = false;
    unsigned img_max = 0u;
    if (p.x_imgmax != nullptr) {
        const unsigned mx = p.x_imgmax[n], mn = p.x_imgmin[n];
        const unsigned Ei = max(mx >> 23, 15u);
        img_rule = Ei - min(mn >> 23, Ei) <= IMG_RANGE_STEP;
        img_max = mx;
    }
    int a_base[2];
    float sc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pl = 4 * wave + 2 * i + (frow >> 4), ql = frow & 15;
        a_base[i] = (2 * pl * PI + ql) * 16;
        unsigned mx = img_max;
        if (!img_rule) {
            mx = 0u;
            const unsigned* w0 = pm + 2 * pl * PM_LD + 2 * ql;
#pragma unroll
            for (int th = 0; th < 7; ++th)
#pragma unroll
                for (int tw = 0; tw < 7; ++tw) mx = max(mx, w0[th * PM_LD + tw]);
        }
        sc[i] = row_scale_of(mx);
    }

    // ---- K loop: no barrier, A fragments from the patch, weight fragments from the image (a step ahead) ------------------------------
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float pa[2] = {0.f, 0.f}, pb[2] = {0.f, 0.f};
    const char* wb = p.w + lane * 16;
    auto read_a = [&](auto ks_c, f32x4 (&x0)[2], f32x4 (&x1)[2]) {
        constexpr int ks = decltype(ks_c)::value;
        constexpr int off_lo = tap_off(2 * ks), off_hi = 2 * ks + 1 < 49 ? tap_off(2 * ks + 1) : tap_off(2 * ks);
        const int off = fhalf ? off_hi : off_lo;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            x0[i] = *reinterpret_cast<const f32x4*>(lds + a_base[i] + off);
            x1[i] = *reinterpret_cast<const f32x4*>(lds + a_base[i] + off + PLANE);
            if constexpr (2 * ks + 1 >= 49) {          // the upper half's tap of the last step does not exist: zeros
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                x0[i] = fhalf ? z : x0[i];
                x1[i] = fhalf ? z : x1[i];
            }
        }
    };
    auto read_b = [&](int ks, f16x8 (&bh)[2], f16x8 (&bl)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            bh[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK + ks) * 2048);
            bl[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK + ks) * 2048 + 1024);
        }
    };
    f32x4 x0[2], x1[2];
    f16x8 bh[2], bl[2];
    read_b(0, bh, bl);
    read_a(std::integral_constant<int, 0>{}, x0, x1);
    auto step = [&](auto ks_c) {
        constexpr int ks = decltype(ks_c)::value;
        f32x4 n0[2], n1[2];
        f16x8 nh[2], nl[2];
        if constexpr (ks + 1 < NK) {
            read_b(ks + 1, nh, nl);
            read_a(std::integral_constant<int, (ks + 1 < NK ? ks + 1 : 0)>{}, n0, n1);
        }
        f16x8 ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            unsigned h01, h23, h45, h67, l01, l23, l45, l67;
            split4_f16<true>(x0[i], sc[i], h01, h23, l01, l23, pa[i]);
            split4_f16<true>(x1[i], sc[i], h45, h67, l45, l67, pb[i]);
            ah[i] = __builtin_bit_cast(f16x8, u32x4{h01, h23, h45, h67});
            al[i] = __builtin_bit_cast(f16x8, u32x4{l01, l23, l45, l67});
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        if constexpr (ks + 1 < NK) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { x0[i] = n0[i]; x1[i] = n1[i]; }
#pragma unroll
            for (int j = 0; j < 2; ++j) { bh[j] = nh[j]; bl[j] = nl[j]; }
        }
    };
    [&]<int... Ks>(std::integer_sequence<int, Ks...>) { (step(std::integral_constant<int, Ks>{}), ...); }(std::make_integer_sequence<int, NK>{});

    // ---- epilogue, in accumulator layout ---------------------------------------------------------------------------------------------
    const int P = p.P, Q = p.Q;
    const unsigned out_bytes = (unsigned)(p.N * P * Q) * (COUT * 4u);
    auto rsrc = [](const void* q, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q), 0, bytes, 0x00020000); };
    const __amdgpu_buffer_rsrc_t r_y = rsrc(p.y, out_bytes), r_t = rsrc(KEEP ? p.t : p.y, out_bytes);
    float cinv[2], csc[2], csh[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cinv[j] = p.cinv[j * 32 + frow];
        csc[j] = p.csc ? p.csc[j * 32 + frow] : 1.f;
        csh[j] = p.csh ? p.csh[j * 32 + frow] : 0.f;
    }
    const bool relu = p.relu != 0;
    const bool want_max = p.y_absmax != nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float ss = pa[i] + pb[i];
        const float tsum = ss + __shfl_xor(ss, 32);
        const float nrm = sqrtf(tsum + 1e-6f);          // BCOS_CONV_EPS
        const float rinv_l = 1.0f / nrm;
        if (p.norm_out != nullptr && fhalf == 0) {
            const int pp = p0 + 4 * wave + 2 * i + (frow >> 4), qq = q0 + (frow & 15);
            if (pp < P && qq < Q) p.norm_out[(n * P + pp) * Q + qq] = nrm;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // register r of a tile = block row (r & 3) + 8 (r >> 2) + 4 fhalf, channel = lane & 31 of the tile
            const int lrow = (r & 3) + 8 * (r >> 2) + 4 * fhalf;
            const int pp = p0 + 4 * wave + 2 * i + (lrow >> 4), qq = q0 + (lrow & 15);
            const bool live = pp < P && qq < Q;
            const int pix = (n * P + pp) * Q + qq;
            const unsigned roff = (live ? (unsigned)pix * (COUT * 4u) : OOB) + (unsigned)frow * 4u;
            const float ainv = inv_scale(__shfl(sc[i], lrow));            // lane l < 32 holds the values of fragment row l
            const float rinv = __shfl(rinv_l, lrow);
            unsigned mx = 0u;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float v = acc[i][j][r] * ainv;
                float val = __builtin_fmaf(v, cinv[j], 0.f);      // (operand scales, then the bias stage: one fma in bcos_tapconv.hip)
                float s = fabsf(val) * rinv;
                val = val * s;
                val = __builtin_fmaf(val, csc[j], csh[j]);
                s = s * csc[j];
                if (relu) {
                    const bool open_gate = val > 0.f;
                    s = open_gate ? __uint_as_float(__float_as_uint(s) | p.lsb) : 0.f;
                    val = open_gate ? val : 0.f;
                }
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), r_y, (int)(roff + j * 128u), 0, 0);
                if (KEEP) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), r_t, (int)(roff + j * 128u), 0, 2);
                mx = max(mx, absbits(val));
            }
            if (want_max) {
                const unsigned a = group_max_u32<32>(mx);         // the row's maximum over its 64 channels: the workgroup owns its pixels
                if (frow == group_max_lane<32>() && live) p.y_absmax[pix] = a;
            }
            __builtin_amdgcn_sched_barrier(0);      // (one row at a time, as in bcos_shortcut.hip)
        }
    }
}

// Per-image range of the per-pixel maxima of the PREPARED input, from the raw image: what bcos_image_absrange gives on the maxima
// bcos_prep_input emits (out_max[n]: the image's maximum; out_min[n]: the smallest nonzero pixel maximum, 0xffffffff where every pixel is
// zero).  One workgroup per image.
__global__ __launch_bounds__(1024) void stem_image_range_kernel(const float* __restrict__ x, const float* __restrict__ mean6,
                                                                const float* __restrict__ std6, unsigned* __restrict__ out_max,
                                                                unsigned* __restrict__ out_min, int Cx, int HW) {
#pragma clang fp contract(off)
    __shared__ unsigned s_max[16], s_min[16];
    float mu[6], sd[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { mu[c] = mean6[c]; sd[c] = std6[c]; }
    const float* src = x + (int64_t)blockIdx.x * Cx * HW;
    unsigned vmax = 0u, vmin = 0xffffffffu;
    for (int i = (int)threadIdx.x; i < HW; i += 1024) {
        float v[6];
        if (Cx == 3) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { v[c] = src[c * HW + i]; v[c + 3] = 1.0f - v[c]; }
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = src[c * HW + i];
        }
        unsigned m = 0u;
#pragma unroll
        for (int c = 0; c < 6; ++c) m = max(m, absbits((v[c] - mu[c]) / sd[c]));
        vmax = max(vmax, m);
        vmin = min(vmin, m - 1u);      // (0 - 1 wraps to the top: zero pixels never win)
    }
    vmax = wave_max_u32(vmax);
    vmin = ~wave_max_u32(~vmin);
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = vmax; s_min[threadIdx.x >> 6] = vmin; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = 0u, mn = 0xffffffffu;
        for (int k = 0; k < 16; ++k) { m = max(m, s_max[k]); mn = min(mn, s_min[k]); }
        out_max[blockIdx.x] = m;
        out_min[blockIdx.x] = mn == 0xffffffffu ? mn : mn + 1u;
    }
}

inline bool aligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

}  // namespace

extern "C" int bcos_stem_image_range(const float* x, const float* mean6, const float* std6, uint32_t* out_max, uint32_t* out_min, int N,
                                     int Cx, int H, int W, int add_inverse, void* stream) {
    if (!x || !mean6 || !std6 || !out_max || !out_min || N <= 0 || H <= 0 || W <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_stem_image_range: bad argument");
    if (Cx != (add_inverse ? 3 : 6)) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_image_range: Cx must be 3 (add_inverse) or 6");
    if ((int64_t)Cx * H * W > INT32_MAX) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_image_range: Cx * H * W exceeds 2^31 - 1");
    hipLaunchKernelGGL(stem_image_range_kernel, dim3((unsigned)N), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), x, mean6, std6,
                       out_max, out_min, Cx, H * W);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("bcos_stem_image_range launch", err);
    return BCOS_OK;
}

extern "C" int bcos_stem_conv_fwd(const bcos_stem_conv* a, void* stream) {
    if (!a) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: NULL argument block");
    if (!a->x || !a->mean6 || !a->std6 || !a->y) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: x, mean6, std6 and y are required");
    if (a->N <= 0 || a->H <= 0 || a->W <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: N, H and W must be positive");
    if (a->Cx != (a->add_inverse ? 3 : 6)) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: Cx must be 3 (add_inverse) or 6");
    if ((a->x_imgmax == nullptr) != (a->x_imgmin == nullptr)) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: x_imgmax and x_imgmin go together");
    if (a->flags & ~BCOS_EPI_SCALE_GATE_LSB) return bcos_set_error(BCOS_E_INVAL, "bcos_stem_conv_fwd: only BCOS_EPI_SCALE_GATE_LSB may be set in flags");
    if (a->kh != 7 || a->kw != 7 || a->stride != 2 || a->padding != 3 || a->Cout != COUT)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: only the 7 x 7 / stride 2 / padding 3 convolution to 64 channels");
    if (a->b != 2.0f) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: only B = 2");
    if (a->max_out != 1 || a->groups != 1) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: no MaxOut, no groups");
    if (a->bias) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: no bias");
    if (a->relu_gate) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: no replayed gate tensor");
    if (a->relu != 0 && a->relu != 1) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: relu must be 0 or 1");
    const bool f16x2 = a->contraction == BCOS_CONTRACT_F16X2 || (a->contraction == BCOS_CONTRACT_DEFAULT && bcos_get_contraction_mode() == 2);
    if (!f16x2 || !a->w_f16x2) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: needs the f16x2 contraction with the pre-split weight image");
    const int P = (a->H - 1) / 2 + 1, Q = (a->W - 1) / 2 + 1;
    const int64_t M = (int64_t)a->N * P * Q;
    if (M * COUT * 4 >= ((int64_t)1 << 31) || (int64_t)a->N * a->Cx * a->H * a->W * 4 >= ((int64_t)1 << 31) || a->N > 65535)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: tensors of 2 GiB and more");
    for (const void* q : {(const void*)a->w_f16x2, (const void*)a->y, (const void*)a->t})
        if (!aligned(q, 16)) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: y, t and the weight image must be 16-byte aligned");
    for (const void* q : {(const void*)a->x, (const void*)a->mean6, (const void*)a->std6, (const void*)a->csc, (const void*)a->csh, (const void*)a->norm_out,
                          (const void*)a->y_absmax, (const void*)a->x_imgmax, (const void*)a->x_imgmin})
        if (!aligned(q, 4)) return bcos_set_error(BCOS_E_NOSUP, "bcos_stem_conv_fwd: arrays must be 4-byte aligned");
    StemArgs k;
    k.x = a->x; k.mean6 = a->mean6; k.std6 = a->std6; k.csc = a->csc; k.csh = a->csh;
    k.y = a->y; k.t = a->t; k.norm_out = a->norm_out; k.y_absmax = a->y_absmax;
    // (the per-image range decides the scale rule only where the tapconv launch would use it: BCOS_OPT_PATCH = 0 scans every row's taps)
    const bool img = a->x_imgmax != nullptr && bcos_option(BCOS_OPT_PATCH) != 0;
    k.x_imgmax = img ? a->x_imgmax : nullptr; k.x_imgmin = img ? a->x_imgmin : nullptr;
    // the inverse row scales follow the fragments of the image (bcos_split_weights_f16x2: rows padded to 128, k to 16)
    k.w = static_cast<const char*>(a->w_f16x2); k.cinv = reinterpret_cast<const float*>(k.w + (size_t)4 * NK * 2048);
    k.N = a->N; k.Cx = a->Cx; k.H = a->H; k.W = a->W; k.P = P; k.Q = Q; k.tiles_q = (Q + TQ - 1) / TQ; k.relu = a->relu;
    k.lsb = (a->relu && a->t && (a->flags & BCOS_EPI_SCALE_GATE_LSB)) ? 1u : 0u;
    const dim3 grid((unsigned)(k.tiles_q * ((P + TP - 1) / TP)), (unsigned)a->N);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->t) hipLaunchKernelGGL((stem_conv_kernel<true>), grid, dim3(NT), 0, s, k);
    else hipLaunchKernelGGL((stem_conv_kernel<false>), grid, dim3(NT), 0, s, k);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("bcos_stem_conv_fwd launch", err);
    return BCOS_OK;
}
