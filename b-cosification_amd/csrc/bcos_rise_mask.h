// bcos_rise_mask.h -- the value of a RISE mask at one pixel, as include/bcos_hip.h defines it ("RISE baseline explainer"): ONE function
// for the three kernels of bcos_rise.hip, so that the dense masks, the prepared copies and the accumulated maps see the same bits.
// Plain fp32, every operation rounded on its own: contraction is switched off for everything that includes this header.
#ifndef BCOS_RISE_MASK_H
#define BCOS_RISE_MASK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

// One axis of the separable bilinear interpolation at upsampled position p = pixel + shift: the two grid indices, mirrored without
// repeating the edge (k -> |k|, then k >= s -> 2 (s - 1) - k), and the weight of the second.
struct RiseAxis {
    int k0, k1;
    float f;
};

__device__ __forceinline__ int rise_mirror(int k, int s) {
    k = k < 0 ? -k : k;
    return k >= s ? 2 * (s - 1) - k : k;
}

// p in [0, U), U = (s + 1) * cell, 2 <= s <= 8, 2 U < 2^24 (the launchers check): num and 2 U are integers fp32 holds exactly
__device__ __forceinline__ RiseAxis rise_axis(int p, int s, int U) {
    const int num = (2 * p + 1) * s - U, den = 2 * U;
    int i0 = num / den;
    if (num - i0 * den < 0) --i0;                                  // floor division: i0 = -1 for the first half cell
    RiseAxis a;
    a.f = (float)(num - i0 * den) / (float)den;
    a.k0 = rise_mirror(i0, s);
    a.k1 = rise_mirror(i0 + 1, s);
    return a;
}

// `bits`: the s x s grid, cell (a, b) in bit a * s + b.  ra0 / ra1: the two row indices ALREADY multiplied by s.
__device__ __forceinline__ float rise_blend(uint64_t bits, int ra0, int ra1, float fr, int b0, int b1, float fc) {
    const float g00 = (float)((bits >> (ra0 + b0)) & 1u), g01 = (float)((bits >> (ra0 + b1)) & 1u);
    const float g10 = (float)((bits >> (ra1 + b0)) & 1u), g11 = (float)((bits >> (ra1 + b1)) & 1u);
    const float top = g00 + fc * (g01 - g00);
    const float bot = g10 + fc * (g11 - g10);
    return top + fr * (bot - top);
}

__device__ __forceinline__ float rise_mask_value(uint64_t bits, int s, RiseAxis r, RiseAxis c) {
    return rise_blend(bits, r.k0 * s, r.k1 * s, r.f, c.k0, c.k1, c.f);
}

#endif  // BCOS_RISE_MASK_H
