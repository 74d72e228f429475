// bcos_boundary.hip -- the block-boundary gradient of an identity-shortcut bottleneck fused with the input gradient of the conv3 below it
// (include/bcos_hip.h: bcos_boundary_conv3_grad).  In the explanation pass of a ResNet-50 the boundary launch (input gradient of the upper
// block's conv1, 64 -> 256, epilogue mul / addend / out2) writes G = v * t3 [M, 256] and the very next launch (input gradient of the lower
// block's conv3, 256 -> 64) reads it back as its A operand and nothing else ever reads it: at 56 x 56 and batch 256 that is 0.82 GB written
// and 0.82 GB read.  Here one workgroup carries a 64-row tile through both contractions and G lives in LDS only.
//
// The result is bit for bit what the two bcos_tapconv_ops launches give (tests/test_boundary_fusion_gpu.py): per accumulator the same 16-k
// steps in the same order with the same three products per step (l_a h_b, h_a l_b, h_a h_b), the same operand-scale rule (a power of two
// from the row's max |A|: per-pixel maxima of g1, the row maximum of G), the same split into (h, l) f16 and the same epilogue expressions
// in the same order as the specialised epilogues of bcos_tapconv.hip (kinds MUL | ADDEND | OUT2 [| MUL2] and MUL [| MULACT]).  The split, the
// scale rule, the lane-group maximum and the rebuilt multiplier are the definitions both files share (bcos_f16x2.h); what is restated here
// is the order of the epilogue expressions and nothing else.
//
// Shape: 256 threads = 2 x 2 waves, one 64-row tile per workgroup, 67 KB of LDS (two workgroups per CU).
//   phase 1  [64 x 64] x [64 x 256]: a wave owns 32 rows x 128 columns (4 accumulator tiles).  A fragments (K = 64: 8 x 16 bytes per lane) and
//            the pre-split weight fragments come straight from global memory / L2 into registers; no LDS.  Epilogue in ACCUMULATOR layout:
//            register r of a tile is one row, the 32 lanes of a half are 32 consecutive columns = 128 contiguous bytes per instruction for
//            addend / t3 / out2.  G goes to LDS as fp32 [64][256] (+16 bytes per row: conflict-free fragment reads); the row maxima of
//            |G| and |out2| are folded over the lanes (DPP), over the four tiles (registers) and over the two column waves (LDS).
//   phase 2  [64 x 256] x [256 x 64]: a wave owns 32 x 32.  The A fragment of a step is read from G and split with the row's scale by the wave
//            that multiplies it -- as the LDS-DMA loop of bcos_tapconv.hip does with its fp32 ring --, the weight fragments (4 KB per step and
//            workgroup) come out of L2.  Epilogue in accumulator layout again (t2 / g3: 128 contiguous bytes per half), row maxima and the
//            per-image range of g3 as the conv3 launch leaves them.
//
// Where this departs from the shape the design first proposed, and why:
//   * G stays fp32 in LDS (65 KB) and is split by the wave that multiplies it, instead of being written as (h, l) f16 planes at the end of
//     phase 1.  The split needs the row's scale, i.e. the maximum of |G| over all 256 columns, and a row's columns belong to TWO waves: the
//     maximum is complete only behind the barrier between the phases, when the accumulators that held G are gone.  Splitting before the
//     barrier would take a second barrier and G held in 64 registers across it; fp32 in LDS costs the same 64-65 KB as the two planes, two
//     workgroups still fit a CU (68 608 B each), and the fragment read + split is what tile_body_d does with its fp32 ring anyway.  In
//     accumulator layout a lane also holds single columns, so packed f16 pairs would need 2-byte LDS stores or a lane exchange.
//   * A (16 KB per tile) and W1's image are not staged in LDS: every A element is used by one row group only (each of its two column waves
//     reads its 32 rows' fragments directly, 8 x 16 bytes per lane, whole 128-byte lines over the four steps) and the weight images (64 KB
//     each, shared by all 12 544 workgroups) stay in L2; staging would add a barrier and LDS traffic for no reuse.  Not A/B-measured against
//     a staged variant; measured as a whole, the launch runs 706 us where the pair it replaces took 703 + 243 us (profiles/boundary_fusion_ab.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int BM = 64;                      // rows of a tile
constexpr int C1 = 64, C4 = 256;            // the one supported pair of widths
constexpr int NT = 256;
constexpr int G_PITCH = C4 * 4 + 16;        // bytes of a row of G in LDS: 8 consecutive rows start in 8 distinct 16-byte bank groups
constexpr int LDS_BYTES = BM * G_PITCH + 8 * BM * 4;
constexpr unsigned OOB = 0x80000000u;       // byte offset beyond every tensor (< 2 GiB): the load returns zeros, the store is dropped
constexpr int NK1 = C1 / 16, NK3 = C4 / 16; // 16-k steps of the two contractions

struct BArgs {
    const float* g1; const unsigned* g1_absmax; const char* w1; const float* cinv1;
    const float* addend; const float* t3; const float* mul2; float* out2; unsigned* out2_absmax;
    const char* w3; const float* cinv3;
    const float* t2; const float* mul_norm; const float* mul_csc; const float* mul_csh;
    float* g3; unsigned* g3_absmax; unsigned* g3_imgmax; unsigned* g3_imgmin_c;
    int M, PQ;
};

__global__ __launch_bounds__(NT, 2) void boundary_conv3_kernel(const BArgs p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* sG = lds;                                                        // [BM] rows of G, fp32
    unsigned* sMaxG = reinterpret_cast<unsigned*>(lds + BM * G_PITCH);     // [2 column waves][BM] row maxima of |G|
    unsigned* sMax2 = sMaxG + 2 * BM;                                      // ... of |out2|
    unsigned* sMax3 = sMax2 + 2 * BM;                                      // ... of |g3|
    unsigned* sImg = sMax3 + 2 * BM;                                       // [BM] maxima, [BM] complemented minima of the images the tile touches
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 31, fhalf = lane >> 5;
    const int m0 = (int)blockIdx.x * BM;
    const int M = p.M;
    if (tid < 2 * BM) sImg[tid] = 0u;                                      // (published by the barrier between the phases)

    const unsigned bytes1 = (unsigned)M * (C1 * 4u), bytes4 = (unsigned)M * (C4 * 4u);
    auto rsrc = [](const void* q, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q), 0, bytes, 0x00020000); };
    const __amdgpu_buffer_rsrc_t r_g1 = rsrc(p.g1, bytes1), r_am = rsrc(p.g1_absmax, (unsigned)M * 4u);
    const __amdgpu_buffer_rsrc_t r_ad = rsrc(p.addend, bytes4), r_t3 = rsrc(p.t3, bytes4), r_o2 = rsrc(p.out2, bytes4);
    const __amdgpu_buffer_rsrc_t r_t2 = rsrc(p.t2, bytes1), r_g3 = rsrc(p.g3, bytes1);
    const bool has_m2 = p.mul2 != nullptr;
    const __amdgpu_buffer_rsrc_t r_m2 = rsrc(has_m2 ? p.mul2 : p.t3, bytes4);

    // ---- phase 1: v = g1 W1^T ------------------------------------------------------------------------------------------------------
    // fragment row of this lane: tile row wm 32 + frow, k = 16 ks + 8 fhalf .. + 7
    const int mA = m0 + wm * 32 + frow;
    const unsigned a_off = mA < M ? (unsigned)mA * (C1 * 4u) + fhalf * 32u : OOB;
    f32x4 x0[NK1], x1[NK1];
#pragma unroll
    for (int ks = 0; ks < NK1; ++ks) {
        x0[ks] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_g1, (int)(a_off + ks * 64u), 0, 0));
        x1[ks] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_g1, (int)(a_off + ks * 64u + 16u), 0, 0));
    }
    const float sc1 = row_scale_of((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_am, (int)(mA < M ? (unsigned)mA * 4u : OOB), 0, 0));
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    {
        const char* wb = p.w1 + (size_t)(wn * 4) * NK1 * 2048 + lane * 16;      // image: [32-row tile][step][plane h | l][lane][8 f16]
#pragma unroll
        for (int ks = 0; ks < NK1; ++ks) {
            f16x8 ah, al, bh[4], bl[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bh[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK1 + ks) * 2048);
                bl[j] = *reinterpret_cast<const f16x8*>(wb + (j * NK1 + ks) * 2048 + 1024);
            }
            split_frag(x0[ks], x1[ks], sc1, ah, al);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[j], 0, 0, 0);
        }
    }
    // epilogue in accumulator layout: register r of a tile = tile row wm 32 + (r & 3) + 8 (r >> 2) + 4 fhalf, column = lane & 31 of the tile
    const bool want2 = p.out2_absmax != nullptr;
    unsigned row_off[16];              // byte offset of the row in a [M, 256] tensor
    float ainv[16];
    unsigned mxg[16], mx2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lrow = (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        const int m = m0 + wm * 32 + lrow;
        row_off[r] = m < M ? (unsigned)m * (C4 * 4u) : OOB;
        ainv[r] = inv_scale(__shfl(sc1, lrow));           // lane l < 32 holds the scale of fragment row l
        mxg[r] = 0u; mx2[r] = 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = wn * 128 + j * 32 + frow;
        const float cinv = p.cinv1[col];
        float ad[16], tt[16], m2[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int voff = (int)(row_off[r] + (unsigned)col * 4u);
            ad[r] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_ad, voff, 0, 2));     // read once: non-temporal
            tt[r] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_t3, voff, 0, 2));
            if (has_m2) m2[r] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_m2, voff, 0, 2));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int voff = (int)(row_off[r] + (unsigned)col * 4u);
            float v = acc[j][r] * ainv[r];
            v = v * cinv;
            float val = v + 0.f;                          // (the bias stage of the epilogue: -0 becomes +0)
            val = val + ad[r];
            const float o1 = val * tt[r];
            float o2 = val;
            if (has_m2) o2 = o2 * m2[r];
            o2 = (__float_as_uint(tt[r]) & 1u) ? o2 : 0.f;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o2), r_o2, voff, 0, 0);
            const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
            *reinterpret_cast<float*>(sG + lrow * G_PITCH + col * 4) = o1;
            mxg[r] = max(mxg[r], absbits(o1));
            mx2[r] = max(mx2[r], absbits(o2));
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        const unsigned a = group_max_u32<32>(mxg[r]);
        const unsigned b = want2 ? group_max_u32<32>(mx2[r]) : 0u;
        if (frow == 16) { sMaxG[wn * BM + lrow] = a; sMax2[wn * BM + lrow] = b; }
    }
    __syncthreads();                   // G and the row maxima of both column waves are complete

    // ---- phase 2: g3 = (G W3^T) t2 -------------------------------------------------------------------------------------------------
    if (want2 && tid < BM && m0 + tid < M) p.out2_absmax[m0 + tid] = max(sMax2[tid], sMax2[BM + tid]);
    const int R = wm * 32 + frow;
    const float sc2 = row_scale_of(max(sMaxG[R], sMaxG[BM + R]));
    f32x16 acc3;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc3[r] = 0.f;
    {
        const char* ga = sG + R * G_PITCH + fhalf * 32;
        const char* wb = p.w3 + (size_t)wn * NK3 * 2048 + lane * 16;
#pragma unroll
        for (int ks = 0; ks < NK3; ++ks) {
            const f16x8 bh = *reinterpret_cast<const f16x8*>(wb + ks * 2048);
            const f16x8 bl = *reinterpret_cast<const f16x8*>(wb + ks * 2048 + 1024);
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(ga + ks * 64);
            const f32x4 g1v = *reinterpret_cast<const f32x4*>(ga + ks * 64 + 16);
            f16x8 ah, al;
            split_frag(g0, g1v, sc2, ah, al);
            acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc3, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc3, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc3, 0, 0, 0);
        }
    }
    const bool want3 = p.g3_absmax != nullptr;
    const bool rebuild = p.mul_norm != nullptr;
    {
        const int col = wn * 32 + frow;
        const float cinv = p.cinv3[col];
        const float mcsc = (rebuild && p.mul_csc) ? p.mul_csc[col] : 1.f;
        const float mcsh = (rebuild && p.mul_csh) ? p.mul_csh[col] : 0.f;
        float tt[16], mn[16];
        int voff[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
            const int m = m0 + lrow;
            voff[r] = (int)(m < M ? (unsigned)m * (C1 * 4u) + (unsigned)col * 4u : OOB);
            tt[r] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r_t2, voff[r], 0, 0));
            mn[r] = rebuild ? p.mul_norm[m < M ? m : 0] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
            const float ai = inv_scale(row_scale_of(max(sMaxG[lrow], sMaxG[BM + lrow])));
            float m1 = tt[r];
            if (rebuild) m1 = bcos_mul_from_act(tt[r], mn[r], mcsc, mcsh);      // t2 holds the kept activation (BCOS_EPI_MUL_FROM_ACT)
            float v = acc3[r] * ai;
            v = v * cinv;
            const float val = v + 0.f;
            const float o = val * m1;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), r_g3, voff[r], 0, 0);
            if (want3) {
                const unsigned a1 = group_max_u32<32>(absbits(o));
                if (frow == 16) sMax3[wn * BM + lrow] = a1;
            }
        }
    }
    if (!want3) return;
    __syncthreads();
    const bool img_on = p.g3_imgmax != nullptr;
    const int n_first = m0 / p.PQ;
    if (tid < BM && m0 + tid < M) {
        const unsigned a1 = max(sMax3[tid], sMax3[BM + tid]);
        p.g3_absmax[m0 + tid] = a1;
        if (img_on && a1) {
            const int slot = (m0 + tid) / p.PQ - n_first;
            atomicMax(sImg + slot, a1);
            atomicMax(sImg + BM + slot, ~a1);
        }
    }
    if (!img_on) return;
    __syncthreads();
    if (tid < 2 * BM) {
        const unsigned v = sImg[tid];
        if (v) atomicMax((tid < BM ? p.g3_imgmax : p.g3_imgmin_c) + n_first + (tid & (BM - 1)), v);
    }
}

inline bool aligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

std::atomic<size_t> g_lds_high_water{0};

}  // namespace

extern "C" int bcos_boundary_conv3_grad(const bcos_boundary_conv3* a, void* stream) {
    if (!a) return bcos_set_error(BCOS_E_INVAL, "bcos_boundary_conv3_grad: NULL argument block");
    if (!a->g1 || !a->addend || !a->t3 || !a->out2 || !a->t2 || !a->g3)
        return bcos_set_error(BCOS_E_INVAL, "bcos_boundary_conv3_grad: g1, addend, t3, out2, t2 and g3 are required");
    if (a->N <= 0 || a->PQ <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_boundary_conv3_grad: N and PQ must be positive");
    if ((a->g3_imgmax == nullptr) != (a->g3_imgmin_c == nullptr) || (a->g3_imgmax && !a->g3_absmax))
        return bcos_set_error(BCOS_E_INVAL, "bcos_boundary_conv3_grad: g3_imgmax, g3_imgmin_c and g3_absmax go together");
    if ((a->mul_csc || a->mul_csh) && !a->mul_norm)
        return bcos_set_error(BCOS_E_INVAL, "bcos_boundary_conv3_grad: mul_csc / mul_csh without mul_norm");
    if (a->C1 != C1 || a->C4 != C4) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: only the widths 64 / 256");
    if (a->kh != 1 || a->kw != 1 || a->stride != 1) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: only 1 x 1 / stride-1 layers");
    if (a->b != 2.0f) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: only B = 2");
    const bool f16x2 = a->contraction == BCOS_CONTRACT_F16X2 || (a->contraction == BCOS_CONTRACT_DEFAULT && bcos_get_contraction_mode() == 2);
    if (!f16x2 || !a->w1_f16x2 || !a->w3_f16x2 || !a->g1_absmax)
        return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: needs the f16x2 contraction with both weight images and g1_absmax");
    const int64_t M = (int64_t)a->N * a->PQ;
    if (M * C4 * 4 >= ((int64_t)1 << 31)) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: tensors of 2 GiB and more");
    for (const void* q : {(const void*)a->g1, (const void*)a->w1_f16x2, (const void*)a->addend, (const void*)a->t3, (const void*)a->mul2, (const void*)a->out2,
                          (const void*)a->w3_f16x2, (const void*)a->t2, (const void*)a->g3, (const void*)a->mul_csc, (const void*)a->mul_csh})
        if (!aligned(q, 16)) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: tensors must be 16-byte aligned");
    for (const void* q : {(const void*)a->g1_absmax, (const void*)a->out2_absmax, (const void*)a->mul_norm, (const void*)a->g3_absmax,
                          (const void*)a->g3_imgmax, (const void*)a->g3_imgmin_c})
        if (!aligned(q, 4)) return bcos_set_error(BCOS_E_NOSUP, "bcos_boundary_conv3_grad: the maxima arrays and mul_norm must be 4-byte aligned");
    BArgs k;
    k.g1 = a->g1; k.g1_absmax = a->g1_absmax;
    // the inverse row scales follow the fragments of an image (bcos_split_weights_f16x2: rows padded to 128, k to 16)
    k.w1 = static_cast<const char*>(a->w1_f16x2); k.cinv1 = reinterpret_cast<const float*>(k.w1 + (C4 / 32) * NK1 * 2048);
    k.w3 = static_cast<const char*>(a->w3_f16x2); k.cinv3 = reinterpret_cast<const float*>(k.w3 + (128 / 32) * NK3 * 2048);
    k.addend = a->addend; k.t3 = a->t3; k.mul2 = a->mul2; k.out2 = a->out2; k.out2_absmax = a->out2_absmax;
    k.t2 = a->t2; k.mul_norm = a->mul_norm; k.mul_csc = a->mul_csc; k.mul_csh = a->mul_csh;
    k.g3 = a->g3; k.g3_absmax = a->g3_absmax; k.g3_imgmax = a->g3_imgmax; k.g3_imgmin_c = a->g3_imgmin_c;
    k.M = (int)M; k.PQ = a->PQ;
    hipError_t err = bcos_ensure_dynamic_lds(reinterpret_cast<const void*>(boundary_conv3_kernel), LDS_BYTES, g_lds_high_water);
    if (err != hipSuccess) return bcos_set_hip_error("bcos_boundary_conv3_grad: LDS size", err);
    hipLaunchKernelGGL(boundary_conv3_kernel, dim3((unsigned)((M + BM - 1) / BM)), dim3(NT), LDS_BYTES, reinterpret_cast<hipStream_t>(stream), k);
    err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("bcos_boundary_conv3_grad launch", err);
    return BCOS_OK;
}
