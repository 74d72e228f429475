// bcos_agc.hip -- adaptive gradient clipping of a whole parameter list (bcos/training/agc.py:28-42 of the reference; the B-cosification
// recipes call it before every optimizer step, bcos/training/trainer.py:872-883).  The reference walks the list in Python: per tensor two
// norms and eight elementwise launches (1,070 launches for ResNet-50).  Here the list goes to the device in chunks of at most 64 tensors,
// each chunk's descriptors by value in the kernel arguments (no device table, no copy, no allocation, no synchronisation), one launch per
// chunk.  One wavefront per unit: it reads p and g once, reduces both sums of squares in a fixed order (per-lane chains, then a butterfly
// whose partners add the same two values, so every lane holds the same bits), decides, and rewrites g only when the unit clips -- that
// second read of g mostly hits the cache.  No atomics: two calls on the same data give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

namespace {

constexpr int AGC_TPB = 256;
constexpr int AGC_WAVES = AGC_TPB / 64;        // units in flight per workgroup
constexpr int AGC_CHUNK = 64;                  // tensors per launch (kernel-argument budget, as torch's multi_tensor_apply)
constexpr int64_t AGC_MAX_BLOCKS = 1 << 16;    // beyond that the waves loop over units
constexpr float AGC_GRAD_FLOOR = 1e-6f;        // grad_norm.clamp(min=1e-6): a constant of the reference (agc.py:39)

// 2,068 bytes of kernel arguments: read with scalar loads, indexed by the wave-uniform tensor number
struct AgcChunk {
    const float* p[AGC_CHUNK];
    float* g[AGC_CHUNK];
    int64_t unit_len[AGC_CHUNK];
    int64_t first[AGC_CHUNK + 1];   // tensor t owns the chunk's units [first[t], first[t+1])
    int ntensors;
    float clip_factor, eps;
};

// a unit as `head` scalars up to p's first 16-byte boundary, `n4` float4 and a scalar tail from `tail`; when g sits at another offset
// modulo 16 than p (parameters that are views into a flat buffer) the whole unit is scalar
struct UnitSplit {
    int64_t head, n4, tail;
};

__device__ inline UnitSplit split_unit(const float* p, const float* g, int64_t len) {
    const uintptr_t ap = reinterpret_cast<uintptr_t>(p), ag = reinterpret_cast<uintptr_t>(g);
    UnitSplit s;
    if (((ap ^ ag) & 15) != 0 || ((ap | ag) & 3) != 0) {
        s.head = len;
        s.n4 = 0;
    } else {
        const int64_t h = (int64_t)(((16 - (ap & 15)) & 15) >> 2);
        s.head = h < len ? h : len;
        s.n4 = (len - s.head) >> 2;
    }
    s.tail = s.head + 4 * s.n4;
    return s;
}

__device__ inline void acc4(float& s, const f32x4 v) {
    s = fmaf(v[0], v[0], s);
    s = fmaf(v[1], v[1], s);
    s = fmaf(v[2], v[2], s);
    s = fmaf(v[3], v[3], s);
}

__global__ __launch_bounds__(AGC_TPB) void agc_clip_kernel(const AgcChunk c, int64_t total_units) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * AGC_WAVES;
    for (int64_t w = (int64_t)blockIdx.x * AGC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); w < total_units; w += nwaves) {
        int lo = 0, hi = c.ntensors;                 // the last tensor with first[t] <= w
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (c.first[mid] <= w) lo = mid; else hi = mid;
        }
        const int64_t len = c.unit_len[lo];
        const int64_t off = (w - c.first[lo]) * len;
        const float* p = c.p[lo] + off;
        float* g = c.g[lo] + off;
        const UnitSplit s = split_unit(p, g, len);

        float sp = 0.f, sg = 0.f;
        for (int64_t i = lane; i < s.head; i += 64) {
            const float a = p[i], b = g[i];
            sp = fmaf(a, a, sp);
            sg = fmaf(b, b, sg);
        }
        const f32x4* p4 = reinterpret_cast<const f32x4*>(p + s.head);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(g + s.head);
        int64_t i = lane;
        for (; i + 3 * 64 < s.n4; i += 4 * 64) {      // four 16-byte loads of each tensor in flight per lane
            f32x4 a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] = __builtin_nontemporal_load(p4 + i + 64 * k);
                b[k] = g4[i + 64 * k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc4(sp, a[k]);
                acc4(sg, b[k]);
            }
        }
        for (; i < s.n4; i += 64) {
            acc4(sp, __builtin_nontemporal_load(p4 + i));
            acc4(sg, g4[i]);
        }
        for (int64_t j = s.tail + lane; j < len; j += 64) {
            const float a = p[j], b = g[j];
            sp = fmaf(a, a, sp);
            sg = fmaf(b, b, sg);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sp += __shfl_xor(sp, o);
            sg += __shfl_xor(sg, o);
        }
        const float pn = sqrtf(sp), gn = sqrtf(sg);
        // clamp(min=...) as torch's: a NaN stays NaN (fmaxf would return the bound)
        const float max_norm = (pn < c.eps ? c.eps : pn) * c.clip_factor;
        if (gn < max_norm) continue;                   // false for a NaN norm: torch.where then takes the clipped (NaN) gradient
        const float scale = max_norm / (gn < AGC_GRAD_FLOOR ? AGC_GRAD_FLOOR : gn);

        for (int64_t j = lane; j < s.head; j += 64) g[j] *= scale;
        f32x4* gw = reinterpret_cast<f32x4*>(g + s.head);
        i = lane;
        for (; i + 3 * 64 < s.n4; i += 4 * 64) {
            f32x4 b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = gw[i + 64 * k];
#pragma unroll
            for (int k = 0; k < 4; ++k) gw[i + 64 * k] = b[k] * scale;
        }
        for (; i < s.n4; i += 64) gw[i] = gw[i] * scale;
        for (int64_t j = s.tail + lane; j < len; j += 64) g[j] *= scale;
    }
}

}  // namespace

extern "C" int bcos_agc_clip(const bcos_agc_tensor* tensors, int ntensors, float clip_factor, float eps, void* stream) {
    if (!tensors || ntensors <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: NULL descriptor array or ntensors <= 0");
    if (!(isfinite(clip_factor) && clip_factor > 0.f) || !(isfinite(eps) && eps > 0.f))
        return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: clip_factor and eps must be finite and positive");
    // everything is checked before the first launch: a refused list leaves every gradient untouched
    int64_t chunk_units = 0;
    for (int t = 0; t < ntensors; ++t) {
        const bcos_agc_tensor& d = tensors[t];
        if (!d.p || !d.g) return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: NULL parameter or gradient");
        if (d.units <= 0 || d.unit_len <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: units and unit_len must be positive");
        if (d.units > INT64_MAX / d.unit_len) return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: units * unit_len overflows");
        if (t % AGC_CHUNK == 0) chunk_units = 0;
        if (__builtin_add_overflow(chunk_units, d.units, &chunk_units))
            return bcos_set_error(BCOS_E_INVAL, "bcos_agc_clip: the units of one chunk of 64 tensors overflow int64");
    }
    for (int base = 0; base < ntensors; base += AGC_CHUNK) {
        AgcChunk c;
        c.ntensors = ntensors - base < AGC_CHUNK ? ntensors - base : AGC_CHUNK;
        c.clip_factor = clip_factor;
        c.eps = eps;
        c.first[0] = 0;
        for (int t = 0; t < AGC_CHUNK; ++t) {
            if (t < c.ntensors) {
                const bcos_agc_tensor& d = tensors[base + t];
                c.p[t] = d.p;
                c.g[t] = d.g;
                c.unit_len[t] = d.unit_len;
                c.first[t + 1] = c.first[t] + d.units;      // (no overflow: checked above)
            } else {
                c.p[t] = nullptr;
                c.g[t] = nullptr;
                c.unit_len[t] = 0;
                c.first[t + 1] = c.first[t];
            }
        }
        const int64_t total = c.first[c.ntensors];
        int64_t blocks = (total + AGC_WAVES - 1) / AGC_WAVES;
        if (blocks > AGC_MAX_BLOCKS) blocks = AGC_MAX_BLOCKS;
        hipLaunchKernelGGL(agc_clip_kernel, dim3((unsigned)blocks), dim3(AGC_TPB), 0, reinterpret_cast<hipStream_t>(stream), c, total);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return bcos_set_hip_error("agc_clip_kernel", err);
    }
    return BCOS_OK;
}
