// bcos_f16x2.h -- the device primitives of the split-f16 (f16x2) contraction, one definition for every kernel that uses them (not part of
// the ABI): the vector types, the (h, l) split, the operand-scale rule, the lane-group maximum, the |x| bit patterns, the multiplier rebuilt
// from a kept activation and the plain wavefront reductions.  Two launches that must agree bit for bit (a fused launch and the pair it
// replaces, bcos_boundary.hip / bcos_shortcut.hip against bcos_tapconv.hip) agree in these because they call the same function.
// No function here holds a multiply that feeds an add, so none depends on the floating-point contraction setting of the file that includes it;
// one that does must fix its own (#pragma clang fp contract(off) inside the function, or an explicit fmaf).
#ifndef BCOS_F16X2_H
#define BCOS_F16X2_H
#include <hip/hip_runtime.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- |x| as a bit pattern (unsigned maxima of these order as the values do) ----------------------------------------------------------
__device__ __forceinline__ unsigned absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned absbits4(const f32x4& v) {
    return max(max(__float_as_uint(v[0]) & 0x7fffffffu, __float_as_uint(v[1]) & 0x7fffffffu),
               max(__float_as_uint(v[2]) & 0x7fffffffu, __float_as_uint(v[3]) & 0x7fffffffu));
}

// ---- the operand-scale rule ----------------------------------------------------------------------------------------------------------
// An operand row (a pixel's channels, a weight row, an image) with max |x| of biased exponent E is multiplied by the power of two
// 2^(141 - E) before the split, so that max * scale lies in [2^14, 2^15); E is clamped at 15 from below (zero rows, denormals: the scale stays
// finite).  f16x2_exp: the clamped exponent of a max-|x| bit pattern (the bit patterns carry no sign); f16x2_scale_bexp: the biased exponent
// of the scale (the level ladder of the input-patch loop adds to it); f16x2_scale / f16x2_inv: the scale and its inverse from E;
// inv_scale: the inverse from the scale itself.
__device__ __forceinline__ unsigned f16x2_exp(unsigned maxbits) {
    const unsigned E = maxbits >> 23;
    return E < 15u ? 15u : E;
}
__device__ __forceinline__ unsigned f16x2_scale_bexp(unsigned E) { return 268u - E; }
__device__ __forceinline__ float f16x2_scale(unsigned E) { return __uint_as_float(f16x2_scale_bexp(E) << 23); }
__device__ __forceinline__ float f16x2_inv(unsigned E) { return __uint_as_float((E - 14u) << 23); }
__device__ __forceinline__ float row_scale_of(unsigned maxbits) { return f16x2_scale(f16x2_exp(maxbits)); }
__device__ __forceinline__ float inv_scale(float s) { return __uint_as_float((254u - (__float_as_uint(s) >> 23)) << 23); }

// ---- the (h, l) split ----------------------------------------------------------------------------------------------------------------
// (h, l) f16 split of fp32 values times a power of two `s`, two values into the two halves of one register each:
//   h = f16(x s),  l = f16(x s - h).
// x s and x s - h are exact in fp32 (s is a power of two, h holds the leading 11 bits of x s), so each result is rounded ONCE, to f16
// -- bit for bit what (_Float16)(x * s) and (_Float16)(x * s - (float)h) give.  Written as the instructions themselves: v_fma_mixlo_f16 /
// v_fma_mixhi_f16 take fp32 (or, per source, f16-half) operands, compute the fma in fp32 and write the f16 result into the low / high
// half of the destination -- two vector instructions per element and no packing.  Left to the compiler the same expressions become
// multiply / convert / convert back / subtract / convert / pack over register PAIRS (v_pk_mul_f32, v_pk_fma_f32 ...: ~6 instructions
// per element plus the moves that build the pairs, and packed fp32 instructions beside matrix instructions cost more than their issue slot).
// One 16-byte piece (four fp32 values) -> two registers of h halves and two of l halves; SUMSQ: acc += x^2 of the four values (one
// v_fmac_f32 each: the compiler pairs neighbouring chains into v_pk_fma_f32 behind two moves).  ONE asm statement, so that nothing is
// padded between its instructions; inside it every instruction that reads a register half written by a v_fma_mix{lo,hi}_f16 is at
// least two instructions behind that write (gfx940+: a result written with a destination half-select needs one wait state before a
// vector instruction reads it).
template <bool SUMSQ>
__device__ __forceinline__ void split4_f16(const f32x4& x, const float s, unsigned& h01, unsigned& h23, unsigned& l01, unsigned& l23, float& acc) {
    unsigned a, b, c, d;
    if constexpr (SUMSQ) {
        asm("v_fma_mixlo_f16 %0, %5, %9, 0\n\t"
            "v_fma_mixlo_f16 %1, %7, %9, 0\n\t"
            "v_fma_mixhi_f16 %0, %6, %9, 0\n\t"
            "v_fma_mixhi_f16 %1, %8, %9, 0\n\t"
            "v_fmac_f32 %4, %5, %5\n\t"
            "v_fma_mixlo_f16 %2, %5, %9, -%0 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixlo_f16 %3, %7, %9, -%1 op_sel_hi:[0,0,1]\n\t"
            "v_fmac_f32 %4, %6, %6\n\t"
            "v_fma_mixhi_f16 %2, %6, %9, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_fmac_f32 %4, %7, %7\n\t"
            "v_fma_mixhi_f16 %3, %8, %9, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_fmac_f32 %4, %8, %8"
            : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d), "+v"(acc)
            : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(s));
    } else {
        asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\t"
            "v_fma_mixlo_f16 %1, %6, %8, 0\n\t"
            "v_fma_mixhi_f16 %0, %5, %8, 0\n\t"
            "v_fma_mixhi_f16 %1, %7, %8, 0\n\t"
            "v_fma_mixlo_f16 %2, %4, %8, -%0 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixlo_f16 %3, %6, %8, -%1 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %2, %5, %8, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %3, %7, %8, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
            : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(s));
    }
    h01 = a; h23 = b; l01 = c; l23 = d;
}
// ... without the sum of squares
__device__ __forceinline__ void split4_f16(const f32x4& x, const float s, unsigned& h01, unsigned& h23, unsigned& l01, unsigned& l23) {
    float unused = 0.f;
    split4_f16<false>(x, s, h01, h23, l01, l23, unused);
}

// the eight k of a lane's fragment (two 16-byte pieces) -> its h and l fragments
__device__ __forceinline__ void split_frag(const f32x4& x0, const f32x4& x1, const float s, f16x8& h, f16x8& l) {
    unsigned h01, h23, h45, h67, l01, l23, l45, l67;
    split4_f16(x0, s, h01, h23, l01, l23);
    split4_f16(x1, s, h45, h67, l45, l67);
    h = __builtin_bit_cast(f16x8, u32x4{h01, h23, h45, h67});
    l = __builtin_bit_cast(f16x8, u32x4{l01, l23, l45, l67});
}

// ---- maxima over lanes ---------------------------------------------------------------------------------------------------------------
// max over groups of G consecutive lanes (G = 8, 16, 32; groups aligned to G) on the vector ALU (DPP), no LDS traffic.
// After the call the lanes with (lane % G) == group_max_lane<G>() hold the group's max.
template <int G>
__device__ __forceinline__ unsigned group_max_u32(unsigned v) {
    static_assert(G == 8 || G == 16 || G == 32, "group size");
    auto dpp = [](unsigned x, auto ctrl) { return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, decltype(ctrl)::value, 0xF, 0xF, false); };
    v = max(v, dpp(v, std::integral_constant<int, 0xB1>{}));       // quad_perm [1,0,3,2]
    v = max(v, dpp(v, std::integral_constant<int, 0x4E>{}));       // quad_perm [2,3,0,1]
    v = max(v, dpp(v, std::integral_constant<int, 0x141>{}));      // row_half_mirror: 8 lanes agree
    if (G >= 16) v = max(v, dpp(v, std::integral_constant<int, 0x140>{}));   // row_mirror: 16 lanes agree
    if (G == 32)                                                    // row_bcast15 into rows 1 and 3: lanes 16..31 of each half
        v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xA, 0xF, false));
    return v;
}
template <int G> constexpr int group_max_lane() { return G == 32 ? 16 : 0; }

// sum / max over the 64 lanes of a wavefront: the butterfly (distances 32, 16, ... 1) whose partners combine the same two values, so
// every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}

// ---- the multiplier rebuilt from a kept activation (BCOS_EPI_MUL_FROM_ACT) -----------------------------------------------------------
// `mul` given as the kept ACTIVATION a = relu(lin s csc + csh) of the layer below (B = 2, s = |lin| / norm) instead of its
// stored multiplier t = s csc gate: |lin|^2 = |a - csh| norm / |csc|, so t = csc sqrt(|a - csh| / (|csc| norm)) where a > 0.
// Hardware reciprocal / square root (1 ulp each): the IEEE division + sqrt sequences are ~20 instructions per element in an epilogue
// that is issue-bound, and t enters a product whose other factor carries fp32 rounding anyway.
__device__ __forceinline__ float bcos_mul_from_act(float a, float nrm, float csc, float csh) {
    const float z = fabsf(a - csh);
    const float den = fabsf(csc) * nrm;
    return (a > 0.f && den > 0.f) ? csc * __builtin_amdgcn_sqrtf(z * __builtin_amdgcn_rcpf(den)) : 0.f;
}

#endif
