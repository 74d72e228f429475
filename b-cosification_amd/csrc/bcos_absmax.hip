// bcos_absmax.hip -- the operand maxima of the split-f16 contraction (bcos_operands.a_absmax / a_imgmax / a_imgmin / a_imgmin_c) for tensors
// whose producer did not emit them: per-pixel max |x| bit patterns (bcos_rows_absmax) and the per-image range of those
// (bcos_image_absmax, bcos_image_absrange, bcos_image_absrange_c).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_f16x2.h"

// per-pixel max |x| bit patterns of an NHWC tensor (for tensors whose producer is not a tapconv epilogue)
namespace {
__global__ __launch_bounds__(256) void rows_absmax_kernel(const float* __restrict__ x, unsigned* __restrict__ out, int64_t rows,
                                                          int C, int pitch) {
    // LPR lanes per row (power of two <= 64), float4 loads
    int lpr = 1;
    while (lpr < 64 && lpr * 4 < C) lpr <<= 1;
    const int rpw = 64 / lpr;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t row = wave * rpw + lane / lpr;
    const int sub = lane % lpr;
    unsigned m = 0u;
    if (row < rows) {
        const float* src = x + row * pitch;
        for (int c = sub * 4; c < C; c += lpr * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) m = max(m, __float_as_uint(v[q]) & 0x7fffffffu);
        }
    }
    for (int o = lpr >> 1; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if (row < rows && sub == 0) out[row] = m;
}
}  // namespace

namespace {
__global__ __launch_bounds__(1024) void image_absmax_kernel(const unsigned* __restrict__ absmax, unsigned* __restrict__ out,
                                                            unsigned* __restrict__ out_min, int hw) {
    // one workgroup of 16 waves per image, four independent loads in flight per thread: the kernel is one load latency long.
    // out_min (optional): the smallest NONZERO per-pixel maximum of the image (0xffffffff: every pixel is zero) -- with the
    // image maximum, the dynamic range of the pixels inside the image (bcos_operands.a_imgmin)
    __shared__ unsigned s_max[16], s_min[16];
    const unsigned* src = absmax + (size_t)blockIdx.x * hw;
    unsigned v = 0u, w = 0xffffffffu;
    for (int i0 = 0; i0 < hw; i0 += 4096) {
        unsigned u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * 1024 + (int)threadIdx.x;
            u[q] = i < hw ? src[i] : 0u;
        }
        v = max(max(v, u[0]), max(max(u[1], u[2]), u[3]));
#pragma unroll
        for (int q = 0; q < 4; ++q) w = min(w, u[q] - 1u);      // (0 - 1 wraps to the top: zero pixels never win)
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        v = max(v, (unsigned)__shfl_xor((int)v, o));
        w = min(w, (unsigned)__shfl_xor((int)w, o));
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = v; s_min[threadIdx.x >> 6] = w; }
    __syncthreads();
    if (threadIdx.x < 16) {
        unsigned m = s_max[threadIdx.x], mn = s_min[threadIdx.x];
#pragma unroll
        for (int o = 8; o; o >>= 1) {
            m = max(m, (unsigned)__shfl_xor((int)m, o));
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
        }
        if (threadIdx.x == 0) {
            out[blockIdx.x] = m;
            if (out_min) out_min[blockIdx.x] = mn == 0xffffffffu ? mn : mn + 1u;
        }
    }
}
}  // namespace

namespace {
// the same range from SEVERAL workgroups per image (grid: image x part), for images of many pixels or a device that is busy with
// another stream's launch: the parts meet by atomicMax in ZERO-FILLED words -- the minimum over the nonzero pixels as its complement
// (~v; 0 = no nonzero pixel), the form the producing epilogues leave (bcos_epilogue.out_imgmin_c)
__global__ __launch_bounds__(256) void image_absrange_c_kernel(const unsigned* __restrict__ absmax, unsigned* __restrict__ out_max,
                                                               unsigned* __restrict__ out_min_c, int hw, int per_part) {
    __shared__ unsigned s_max[4], s_min[4];
    const unsigned* src = absmax + (size_t)blockIdx.x * hw;
    const int lo = (int)blockIdx.y * per_part, hi = lo + per_part < hw ? lo + per_part : hw;
    unsigned v = 0u, w = 0xffffffffu;
    for (int i0 = lo; i0 < hi; i0 += 1024) {
        unsigned u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * 256 + (int)threadIdx.x;
            u[q] = i < hi ? src[i] : 0u;
        }
        v = max(max(v, u[0]), max(max(u[1], u[2]), u[3]));
#pragma unroll
        for (int q = 0; q < 4; ++q) w = min(w, u[q] - 1u);      // (0 - 1 wraps to the top: zero pixels never win)
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        v = max(v, (unsigned)__shfl_xor((int)v, o));
        w = min(w, (unsigned)__shfl_xor((int)w, o));
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = v; s_min[threadIdx.x >> 6] = w; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        const unsigned mn = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        if (m) atomicMax(out_max + blockIdx.x, m);
        if (mn != 0xffffffffu) atomicMax(out_min_c + blockIdx.x, ~(mn + 1u));
    }
}
}  // namespace

extern "C" int bcos_image_absrange_c(const uint32_t* absmax, uint32_t* out_max, uint32_t* out_min_c, int n_images, int pixels_per_image,
                                     void* stream) {
    if (!absmax || !out_max || !out_min_c || n_images <= 0 || pixels_per_image <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_image_absrange_c: bad argument");
    // parts of >= 2 048 pixels, as many as put ~1 024 workgroups on the device
    int parts = (pixels_per_image + 2047) / 2048;
    const int want = (1024 + n_images - 1) / n_images;
    parts = parts < 1 ? 1 : (parts > want ? want : parts);
    const int per_part = (((pixels_per_image + parts - 1) / parts) + 255) & ~255;
    parts = (pixels_per_image + per_part - 1) / per_part;
    hipLaunchKernelGGL(image_absrange_c_kernel, dim3((unsigned)n_images, (unsigned)parts), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       absmax, out_max, out_min_c, pixels_per_image, per_part);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("image_absrange_c launch", err);
    return BCOS_OK;
}

extern "C" int bcos_image_absmax(const uint32_t* absmax, uint32_t* out, int n_images, int pixels_per_image, void* stream) {
    return bcos_image_absrange(absmax, out, nullptr, n_images, pixels_per_image, stream);
}

extern "C" int bcos_image_absrange(const uint32_t* absmax, uint32_t* out_max, uint32_t* out_min, int n_images, int pixels_per_image,
                                   void* stream) {
    uint32_t* out = out_max;
    if (!absmax || !out || n_images <= 0 || pixels_per_image <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_image_absmax: bad argument");
    hipLaunchKernelGGL(image_absmax_kernel, dim3((unsigned)n_images), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), absmax, out,
                       out_min, pixels_per_image);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("image_absmax launch", err);
    return BCOS_OK;
}

extern "C" int bcos_rows_absmax(const float* x, uint32_t* out, int64_t rows, int C, int pitch, void* stream) {
    if (!x || !out || rows <= 0 || C <= 0 || C % 4 != 0) return bcos_set_error(BCOS_E_INVAL, "bcos_rows_absmax: bad argument");
    if (pitch == 0) pitch = C;
    if (pitch % 4 != 0 || pitch < C || (reinterpret_cast<uintptr_t>(x) & 15))
        return bcos_set_error(BCOS_E_INVAL, "bcos_rows_absmax: rows must be 16-byte addressable");
    int lpr = 1;
    while (lpr < 64 && lpr * 4 < C) lpr <<= 1;
    const int64_t rows_per_block = 4 * (64 / lpr);
    hipLaunchKernelGGL(rows_absmax_kernel, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, out, rows, C, pitch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return bcos_set_hip_error("rows_absmax launch", err);
    return BCOS_OK;
}
