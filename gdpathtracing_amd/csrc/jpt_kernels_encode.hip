// jpt_kernels_encode.hip -- jpt_encode: a float4 image packed into RGBA16F, RGB9E5 or RGBE8 texels (the arithmetic: jpt_encode.h,
// where encode_host restates the transform for the host).
//
// One streaming kernel, templated on the format, 256 threads per block.  A thread takes consecutive texels that make one 16-byte store:
// four for the 4-byte formats (four 16-byte loads), two for RGBA16F (two 16-byte loads); a thread whose texels run past the end takes
// them one by one with 4- or 8-byte stores.  The divisor is a kernel argument, 1 for every source but the running mean: the division is
// skipped when it is 1 (wave-uniform).  Memory-bound: 16 B in and 4 or 8 B out per texel.  No LDS, no atomics, no scratch; indices are
// 64-bit (the largest image is a whole reflection chain).
#include <hip/hip_runtime.h>

#include "jpt_encode.h"

namespace jpt {

namespace {

constexpr int kEncodeBlock = 256;

// One texel, as one 16-byte load.  RGB9E5 and RGBE8 drop alpha, and the compiler would narrow their loads to 12 bytes of every 16: naming
// alpha as an input of an empty statement keeps the load whole (the same lines are fetched either way; one instruction form, one VGPR).
template <int FORMAT>
__device__ __forceinline__ float4 load_texel(const float4* __restrict__ src, uint64_t i)
{
    const float4 v = src[i];
    if (FORMAT != kEncodeRgba16f) asm volatile("" ::"v"(v.w));
    return v;
}

template <int FORMAT>
__global__ __launch_bounds__(kEncodeBlock) void encode_kernel(const float4* __restrict__ src, uint64_t n, float divisor, int alpha_one, void* __restrict__ out)
{
    constexpr uint64_t kPer = FORMAT == kEncodeRgba16f ? 2u : 4u;   // texels of one 16-byte store
    const bool divide = divisor != 1.0f, one = alpha_one != 0;
    const uint64_t t = (uint64_t)blockIdx.x * (uint64_t)kEncodeBlock + threadIdx.x, first = t * kPer;
    if (first >= n) return;
    if (first + kPer <= n) {
        float4 v[kPer];
#pragma unroll
        for (int k = 0; k < (int)kPer; k++) v[k] = load_texel<FORMAT>(src, first + (uint64_t)k);
#pragma unroll
        for (int k = 0; k < (int)kPer; k++) v[k] = encode_source(v[k], divisor, divide, one);
        uint4 q;
        if (FORMAT == kEncodeRgba16f) {
            const uint2 a = encode_rgba16f(v[0]), b = encode_rgba16f(v[1]);
            q = make_uint4(a.x, a.y, b.x, b.y);
        } else if (FORMAT == kEncodeRgb9e5) {
            q = make_uint4(encode_rgb9e5(v[0]), encode_rgb9e5(v[1]), encode_rgb9e5(v[2]), encode_rgb9e5(v[3]));
        } else {
            q = make_uint4(encode_rgbe8(v[0]), encode_rgbe8(v[1]), encode_rgbe8(v[2]), encode_rgbe8(v[3]));
        }
        static_cast<uint4*>(out)[t] = q;
        return;
    }
    for (uint64_t i = first; i < n; i++) {   // the tail: at most kPer - 1 texels of one thread
        const float4 v = encode_source(load_texel<FORMAT>(src, i), divisor, divide, one);
        if (FORMAT == kEncodeRgba16f) static_cast<uint2*>(out)[i] = encode_rgba16f(v);
        else static_cast<uint32_t*>(out)[i] = FORMAT == kEncodeRgb9e5 ? encode_rgb9e5(v) : encode_rgbe8(v);
    }
}

template <int FORMAT>
void launch(hipStream_t stream, const float4* src, uint64_t n, float divisor, bool alpha_one, void* out)
{
    constexpr uint64_t kPer = FORMAT == kEncodeRgba16f ? 2u : 4u;
    const uint64_t threads = (n + kPer - 1u) / kPer;
    const unsigned blocks = (unsigned)((threads + (uint64_t)kEncodeBlock - 1u) / (uint64_t)kEncodeBlock);
    hipLaunchKernelGGL(encode_kernel<FORMAT>, dim3(blocks), dim3(kEncodeBlock), 0, stream, src, n, divisor, alpha_one ? 1 : 0, out);
}

}  // namespace

void launch_encode(hipStream_t stream, int32_t format, const float4* src, uint64_t n, float divisor, bool alpha_one, void* out)
{
    if (n == 0) return;
    if (format == kEncodeRgba16f) launch<kEncodeRgba16f>(stream, src, n, divisor, alpha_one, out);
    else if (format == kEncodeRgb9e5) launch<kEncodeRgb9e5>(stream, src, n, divisor, alpha_one, out);
    else launch<kEncodeRgbe8>(stream, src, n, divisor, alpha_one, out);
}

}  // namespace jpt
