// bcos_shortcut.hip -- the 1 x 1 downsample shortcut of a stage's first bottleneck fused into the forward launch of the conv3 beside it
// (include/bcos_hip.h: bcos_shortcut_conv3_fwd).  In the forward pass the shortcut launch writes idn [M, C4] (and, when multipliers are
// kept, td) and the very next launch, conv3 with addend = idn, reads it back; nothing else ever reads idn: at 56 x 56 and batch 256 that
// is 0.82 GB written and 0.82 GB read.  Here one workgroup carries a 64-row tile through both contractions and idn lives in registers only.
//
// The result is bit for bit what the two bcos_tapconv_ops launches give (tests/test_shortcut_fusion_gpu.py): per accumulator the same 16-k
// steps in the same order with the same three products per step (l_a h_b, h_a l_b, h_a h_b), the same operand-scale rule (a power of two
// from the pixel's max |A|), the same split into (h, l) f16, the patch norm summed as tile_body_d sums it from its A fragments (per lane
// one fma chain over the first and one over the second 16-byte piece of every step, the two added, then the two halves of the wave) and the
// forward epilogue expressions in the order of bcos_tapconv.hip's specialised kinds ([RELU |] [SCALE_OUT |] [ADDEND]).  That file is
// compiled with the compiler's default contraction of a * b + c into one fma; this one switches contraction off and writes the two fused
// operations of the epilogue (the bias stage and the channel affine) as explicit fmas.  The split, the scale rule and the lane-group maximum are the
// definitions both files share (bcos_f16x2.h); what is restated here is the order of the epilogue expressions (and the patch norm's
// summation order) and nothing else.
//
// Shape: 256 threads = 2 x 2 waves, one 64-row tile per workgroup and 256 output columns at a time (C4 = 512: two passes, the small A
// operands re-read from L2): a wave owns 32 rows x 128 columns = 4 accumulator tiles.
//   phase 1  the shortcut: x_sub [64 x Kd] x [Kd x 256].  A fragments come straight from global memory (a pixel of the stride grid is one
//            contiguous row of Kd floats), the pre-split weight fragments out of L2; no LDS.  Epilogue in ACCUMULATOR layout (register r of
//            a tile is one row, the 32 lanes of a half are 32 consecutive columns = 128 contiguous bytes per instruction) into 64 registers
//            of idn; td is stored non-temporally.
//   phase 2  conv3: h [64 x K3] x [K3 x 256] into the same accumulators, epilogue + idn, ReLU, gate bit; out with the default cache policy
//            (the next launch reads it), t3 non-temporally; the row maxima of |out| are folded over the tiles (registers), the lanes (DPP),
//            the column passes and the two column waves (LDS) and written with a plain store: the workgroup owns its pixels.
// Measured at batch 256 (profiles/shortcut_fusion_ab.txt): 64, 64 -> 256 at 56 x 56 runs 661 us where the pair took 926 us; 128, 256 -> 512
// at 28 x 28 runs 634 us against 568 us -- its 48 dependent steps per workgroup with nothing but the next A fragment prefetched (the
// registers are taken) leave it latency-bound --, so the engine keeps that site on the pair of launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int BM = 64;                      // rows of a tile
constexpr int BN = 256;                     // output columns of a pass
constexpr int NT = 256;
constexpr unsigned OOB = 0x80000000u;       // byte offset beyond every tensor (< 2 GiB): the load returns zeros, the store is dropped

struct SArgs {
    const float* x; const unsigned* x_absmax; const char* wd; const float* cinvd; const float* cscd; const float* cshd; float* td;
    const float* h; const unsigned* h_absmax; const char* w3; const float* cinv3; const float* csc3; const float* csh3;
    float* out; float* t3; unsigned* out_absmax;
    int M, PQ, Q, H, W, stride;
    unsigned lsb;
};

// One [32 x 16 NK] x [16 NK x 128] contraction of a wave: the A fragments of row `a_off` (byte offset of the lane's first piece: row base +
// 32 bytes for the upper half of the wave) through descriptor `ra`, split with the row's scale `sc`; the weight image `wb` (already at the
// wave's first 32-column tile and the lane's 16 bytes).  -> the accumulators and 1 / patch norm of the lane's fragment row.
template <int NK>
__device__ __forceinline__ float contract(const __amdgpu_buffer_rsrc_t ra, const unsigned a_off, const float sc, const char* wb, f32x16 (&acc)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float pa = 0.f, pb = 0.f;
    f32x4 n0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)a_off, 0, 0));
    f32x4 n1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)(a_off + 16u), 0, 0));
#pragma unroll 2
    for (int ks = 0; ks < NK; ++ks) {
        const f32x4 x0 = n0, x1 = n1;
        if (ks + 1 < NK) {
            n0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)(a_off + (ks + 1) * 64u), 0, 0));
            n1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)(a_off + (ks + 1) * 64u + 16u), 0, 0));
        }
        f16x8 ah, al, bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bh[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK + ks) * 2048);
            bl[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK + ks) * 2048 + 1024);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) pa = __builtin_fmaf(x0[q], x0[q], pa);
#pragma unroll
        for (int q = 0; q < 4; ++q) pb = __builtin_fmaf(x1[q], x1[q], pb);
        split_frag(x0, x1, sc, ah, al);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[j], 0, 0, 0);
    }
    const float ss = pa + pb;
    const float t = ss + __shfl_xor(ss, 32);
    const float nrm = sqrtf(t + 1e-6f);          // BCOS_CONV_EPS
    return 1.0f / nrm;
}

template <int NKD, int NK3, int NPART, bool KEEP>
__global__ __launch_bounds__(NT, 2) void shortcut_conv3_kernel(const SArgs p) {
#pragma clang fp contract(off)
    __shared__ unsigned sMax[2 * BM];                                      // [2 column waves][BM] row maxima of |out|
    constexpr int KD = NKD * 16, K3 = NK3 * 16, C4 = NPART * BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 31, fhalf = lane >> 5;
    const int m0 = (int)blockIdx.x * BM;
    const int M = p.M;

    auto rsrc = [](const void* q, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q), 0, bytes, 0x00020000); };
    const unsigned pix_in = (unsigned)(M / p.PQ) * (unsigned)(p.H * p.W);      // pixels of the block input
    const unsigned bytes4 = (unsigned)M * (C4 * 4u);
    const __amdgpu_buffer_rsrc_t r_x = rsrc(p.x, pix_in * (KD * 4u)), r_xm = rsrc(p.x_absmax, pix_in * 4u);
    const __amdgpu_buffer_rsrc_t r_h = rsrc(p.h, (unsigned)M * (K3 * 4u)), r_hm = rsrc(p.h_absmax, (unsigned)M * 4u);
    constexpr bool keep_d = KEEP, keep_3 = KEEP;      // the multipliers td and t3 are kept together (explanation pass) or not at all
    const __amdgpu_buffer_rsrc_t r_out = rsrc(p.out, bytes4), r_td = rsrc(keep_d ? p.td : p.out, bytes4), r_t3 = rsrc(keep_3 ? p.t3 : p.out, bytes4);

    // fragment row of this lane: tile row wm 32 + frow, k = 16 ks + 8 fhalf .. + 7; the shortcut reads the pixel on its stride grid
    const int mA = m0 + wm * 32 + frow;
    unsigned xd_off = OOB, xm_off = OOB, h_off = OOB, hm_off = OOB;
    if (mA < M) {
        const int n = mA / p.PQ;
        const int rem = mA - n * p.PQ;
        const int pp = rem / p.Q;
        const int qq = rem - pp * p.Q;
        const unsigned pix = (unsigned)((n * p.H + pp * p.stride) * p.W + qq * p.stride);
        xd_off = pix * (KD * 4u) + fhalf * 32u;
        xm_off = pix * 4u;
        h_off = (unsigned)mA * (K3 * 4u) + fhalf * 32u;
        hm_off = (unsigned)mA * 4u;
    }
    const float scd = row_scale_of((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_xm, (int)xm_off, 0, 0));
    const float sc3 = row_scale_of((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_hm, (int)hm_off, 0, 0));

    // accumulator layout: register r of a tile = tile row wm 32 + (r & 3) + 8 (r >> 2) + 4 fhalf, column = lane & 31 of the tile
    const bool want_max = p.out_absmax != nullptr;
#pragma unroll 1
    for (int part = 0; part < NPART; ++part) {
        const int col0 = part * BN + wn * 128 + frow;       // this lane's column of tile 0 (+ 32 per tile)
        f32x16 acc[4];
        float idn[4][16];
        // ---- phase 1: the shortcut --------------------------------------------------------------------------------------------------
        {
            const float rinv_l = contract<NKD>(r_x, xd_off, scd, p.wd + (size_t)((col0 - frow) >> 5) * NKD * 2048 + lane * 16, acc);
            float cinv[4], csc[4], csh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cinv[j] = p.cinvd[col0 + j * 32];
                csc[j] = p.cscd ? p.cscd[col0 + j * 32] : 1.f;
                csh[j] = p.cshd ? p.cshd[col0 + j * 32] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * fhalf;
                const int m = m0 + wm * 32 + lrow;
                const unsigned roff = (m < M ? (unsigned)m * (C4 * 4u) : OOB) + (unsigned)col0 * 4u;
                const float ainv = inv_scale(__shfl(scd, lrow));            // lane l < 32 holds the values of fragment row l
                const float rinv = __shfl(rinv_l, lrow);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[j][r] * ainv;
                    float val = __builtin_fmaf(v, cinv[j], 0.f);      // (operand scales, then the bias stage: one fma in bcos_tapconv.hip)
                    float s = fabsf(val) * rinv;
                    val = val * s;
                    val = __builtin_fmaf(val, csc[j], csh[j]);
                    s = s * csc[j];
                    asm volatile("" : "+v"(val));      // (idn is formed HERE: left alone the compiler carries val and s into phase 2 and forms it there)
                    idn[j][r] = val;
                    if (keep_d) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), r_td, (int)(roff + j * 128u), 0, 2);
                }
                __builtin_amdgcn_sched_barrier(0);      // (one row at a time: left alone the scheduler computes the whole tile ahead of its stores and spills)
            }
        }
        // ---- phase 2: conv3 ---------------------------------------------------------------------------------------------------------
        {
            const float rinv_l = contract<NK3>(r_h, h_off, sc3, p.w3 + (size_t)((col0 - frow) >> 5) * NK3 * 2048 + lane * 16, acc);
            float cinv[4], csc[4], csh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cinv[j] = p.cinv3[col0 + j * 32];
                csc[j] = p.csc3 ? p.csc3[col0 + j * 32] : 1.f;
                csh[j] = p.csh3 ? p.csh3[col0 + j * 32] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * fhalf;
                const int m = m0 + wm * 32 + lrow;
                unsigned roff = (m < M ? (unsigned)m * (C4 * 4u) : OOB) + (unsigned)col0 * 4u;
                asm volatile("" : "+v"(roff));              // (recomputed, not carried over from phase 1 in 64 registers)
                const float ainv = inv_scale(__shfl(sc3, lrow));
                const float rinv = __shfl(rinv_l, lrow);
                unsigned mx = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int voff = (int)(roff + j * 128u);
                    const float v = acc[j][r] * ainv;
                    float val = __builtin_fmaf(v, cinv[j], 0.f);
                    float s = fabsf(val) * rinv;
                    val = val * s;
                    val = __builtin_fmaf(val, csc[j], csh[j]);
                    s = s * csc[j];
                    val = val + idn[j][r];
                    const bool open_gate = val > 0.f;
                    s = open_gate ? __uint_as_float(__float_as_uint(s) | p.lsb) : 0.f;
                    val = open_gate ? val : 0.f;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), r_out, voff, 0, 0);
                    if (keep_3) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), r_t3, voff, 0, 2);
                    mx = max(mx, absbits(val));
                }
                if (want_max) {
                    // the row's maximum over this wave's 128 columns; over the column passes in LDS (the same lane owns the word in every pass)
                    const unsigned a = group_max_u32<32>(mx);
                    if (frow == 16) {
                        unsigned* w = sMax + wn * BM + wm * 32 + lrow;
                        *w = part == 0 ? a : max(*w, a);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (!want_max) return;
    __syncthreads();
    if (tid < BM && m0 + tid < M) p.out_absmax[m0 + tid] = max(sMax[tid], sMax[BM + tid]);
}

inline bool aligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

}  // namespace

extern "C" int bcos_shortcut_conv3_fwd(const bcos_shortcut_conv3* a, void* stream) {
    if (!a) return bcos_set_error(BCOS_E_INVAL, "bcos_shortcut_conv3_fwd: NULL argument block");
    if (!a->x || !a->h || !a->out) return bcos_set_error(BCOS_E_INVAL, "bcos_shortcut_conv3_fwd: x, h and out are required");
    if (a->N <= 0 || a->H <= 0 || a->W <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_shortcut_conv3_fwd: N, H and W must be positive");
    if ((a->td == nullptr) != (a->t3 == nullptr)) return bcos_set_error(BCOS_E_INVAL, "bcos_shortcut_conv3_fwd: td and t3 go together");
    if (a->flags & ~BCOS_EPI_SCALE_GATE_LSB) return bcos_set_error(BCOS_E_INVAL, "bcos_shortcut_conv3_fwd: only BCOS_EPI_SCALE_GATE_LSB may be set in flags");
    const bool cfg1 = a->K3 == 64 && a->Kd == 64 && a->stride == 1 && a->C4 == 256;
    const bool cfg2 = a->K3 == 128 && a->Kd == 256 && a->stride == 2 && a->C4 == 512;
    if (!cfg1 && !cfg2)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: only (K3, Kd, stride, C4) = (64, 64, 1, 256) and (128, 256, 2, 512)");
    if (a->kh != 1 || a->kw != 1) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: only 1 x 1 layers");
    if (a->b != 2.0f) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: only B = 2");
    if (a->max_out != 1 || a->groups != 1) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: no MaxOut, no groups");
    if (a->bias_d || a->bias_3) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: no bias");
    if (a->relu_gate) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: no replayed gate tensor");
    const bool f16x2 = a->contraction == BCOS_CONTRACT_F16X2 || (a->contraction == BCOS_CONTRACT_DEFAULT && bcos_get_contraction_mode() == 2);
    if (!f16x2 || !a->wd_f16x2 || !a->w3_f16x2 || !a->x_absmax || !a->h_absmax)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: needs the f16x2 contraction with both weight images and both operands' maxima");
    const int P = (a->H + a->stride - 1) / a->stride, Q = (a->W + a->stride - 1) / a->stride;
    const int64_t M = (int64_t)a->N * P * Q;
    if (M * a->C4 * 4 >= ((int64_t)1 << 31) || (int64_t)a->N * a->H * a->W * a->Kd * 4 >= ((int64_t)1 << 31))
        return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: tensors of 2 GiB and more");
    for (const void* q : {(const void*)a->x, (const void*)a->wd_f16x2, (const void*)a->csc_d, (const void*)a->csh_d, (const void*)a->td, (const void*)a->h,
                          (const void*)a->w3_f16x2, (const void*)a->csc_3, (const void*)a->csh_3, (const void*)a->out, (const void*)a->t3})
        if (!aligned(q, 16)) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: tensors must be 16-byte aligned");
    for (const void* q : {(const void*)a->x_absmax, (const void*)a->h_absmax, (const void*)a->out_absmax})
        if (!aligned(q, 4)) return bcos_set_error(BCOS_E_NOSUP, "bcos_shortcut_conv3_fwd: the maxima arrays must be 4-byte aligned");
    SArgs k;
    k.x = a->x; k.x_absmax = a->x_absmax; k.cscd = a->csc_d; k.cshd = a->csh_d; k.td = a->td;
    k.h = a->h; k.h_absmax = a->h_absmax; k.csc3 = a->csc_3; k.csh3 = a->csh_3;
    k.out = a->out; k.t3 = a->t3; k.out_absmax = a->out_absmax;
    // the inverse row scales follow the fragments of an image (bcos_split_weights_f16x2: rows padded to 128, k to 16)
    k.wd = static_cast<const char*>(a->wd_f16x2); k.cinvd = reinterpret_cast<const float*>(k.wd + (size_t)(a->C4 / 32) * (a->Kd / 16) * 2048);
    k.w3 = static_cast<const char*>(a->w3_f16x2); k.cinv3 = reinterpret_cast<const float*>(k.w3 + (size_t)(a->C4 / 32) * (a->K3 / 16) * 2048);
    k.M = (int)M; k.PQ = P * Q; k.Q = Q; k.H = a->H; k.W = a->W; k.stride = a->stride;
    k.lsb = (a->flags & BCOS_EPI_SCALE_GATE_LSB) ? 1u : 0u;
    const dim3 grid((unsigned)((M + BM - 1) / BM));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool keep = a->td != nullptr;
    if (cfg1 && keep) hipLaunchKernelGGL((shortcut_conv3_kernel<4, 4, 1, true>), grid, dim3(NT), 0, s, k);
    else if (cfg1) hipLaunchKernelGGL((shortcut_conv3_kernel<4, 4, 1, false>), grid, dim3(NT), 0, s, k);
    else if (keep) hipLaunchKernelGGL((shortcut_conv3_kernel<16, 8, 2, true>), grid, dim3(NT), 0, s, k);
    else hipLaunchKernelGGL((shortcut_conv3_kernel<16, 8, 2, false>), grid, dim3(NT), 0, s, k);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("bcos_shortcut_conv3_fwd launch", err);
    return BCOS_OK;
}
