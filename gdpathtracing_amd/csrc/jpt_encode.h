// jpt_encode.h -- the arithmetic of jpt_encode ("encoded outputs"): a float4 image the context holds, packed on
// the device into the format the engine stores it in -- half float (RGBA16F), shared-exponent RGB9E5 (VK_FORMAT_E5B9G9R9_UFLOAT_PACK32,
// GL_RGB9_E5, Godot's FORMAT_RGBE9995) or Ward's RGBE8 (a Radiance .hdr file's texels).  No reference counterpart: the reference hands
// its images to the engine as they are.  Every step is one binary32 operation, a compare and select, or an integer / bit operation, in
// source order: the device kernel (jpt_kernels_encode.hip) and the host form of jpt_debug_encode run these functions, and
// tests/np_encode.py restates them in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jpt {

constexpr int kEncodeRgba16f = 1, kEncodeRgb9e5 = 2, kEncodeRgbe8 = 3;   // JPT_ENCODE_*

__host__ __device__ __forceinline__ uint32_t encode_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__host__ __device__ __forceinline__ float encode_float(uint32_t u) { return __builtin_bit_cast(float, u); }
// a NaN gives +0, then two selects: lo for anything below it (-0 below +0 included: -0 > 0 is false), hi for anything above
__host__ __device__ __forceinline__ float encode_clamp(float x, float lo, float hi)
{
    const float z = x != x ? 0.0f : x;
    const float t = z > lo ? z : lo;
    return t < hi ? t : hi;
}
__host__ __device__ __forceinline__ float encode_max3(float a, float b, float c)
{
    const float t = a > b ? a : b;
    return t > c ? t : c;
}
// 2^k as a float, k in -126 .. 127
__host__ __device__ __forceinline__ float encode_pow2(int k) { return encode_float((uint32_t)(k + 127) << 23); }

// 1. the texel as the formats take it: rgb / divisor when the divisor is not 1 (one IEEE division per channel: the running mean of the
// accumulation, divisor = (float)frame_count); alpha as it is, or 1 (`alpha_one`: the accumulation's alpha is a sum nobody reads)
__host__ __device__ __forceinline__ float4 encode_source(const float4& s, float divisor, bool divide, bool alpha_one)
{
    float4 v = s;
    if (divide) {
        v.x = s.x / divisor;
        v.y = s.y / divisor;
        v.z = s.z / divisor;
    }
    if (alpha_one) v.w = 1.0f;
    return v;
}

// 2. RGBA16F.  One channel: NaN -> +0, clamp to [-65504, 65504] (so +-inf saturate), round to nearest even.  -0 stays -0 (NaN gives +0
// before the clamp, and the clamp's selects keep a -65504 <= x <= 65504 as it is).  |x| >= 2^-14 is a normal half: the exponent is
// rebiased and the 13 dropped bits rounded in integers (0xfff + the kept bit's parity: ties to even; a carry runs into the exponent, and
// 65504 is the largest input, so none reaches the infinity).  Below that the half is subnormal, a multiple of 2^-24: |x| + 0.5f is rounded
// by the adder to that grid (the ulp of [0.5, 1)), ties to even, and its low mantissa bits are the half's.  2^-25 gives 0, its successor 1.
__host__ __device__ __forceinline__ uint32_t encode_half(float x)
{
    const float c = encode_clamp(x, -65504.0f, 65504.0f);
    const uint32_t u = encode_bits(c), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    uint32_t h;
    if (a >= 0x38800000u) {
        const uint32_t r = a - 0x38000000u;
        h = (r + 0xfffu + ((r >> 13) & 1u)) >> 13;
    } else {
        h = encode_bits(encode_float(a) + 0.5f) - 0x3f000000u;
    }
    return sign | h;
}
// r g b a in ascending addresses: two little-endian words
__host__ __device__ __forceinline__ uint2 encode_rgba16f(const float4& v)
{
    return make_uint2(encode_half(v.x) | (encode_half(v.y) << 16), encode_half(v.z) | (encode_half(v.w) << 16));
}

// 3. RGB9E5: r | g << 9 | b << 18 | e << 27, alpha dropped.  Per channel NaN -> 0 and clamp to [0, 65408] (511 * 2^7, the largest value
// of the format).  With m the largest channel, e = max(biased exponent of m - 127, -16) + 16 from m's bits (m = 0 and the float32
// subnormals have biased exponent 0: e = 0), the mantissas are floorf(c * 2^(24 - e) + 0.5f) -- the product is exact, the sum is the one
// rounding -- unless m's own mantissa comes to 512: then e + 1 and half the scale.  e <= 31: 65408 gives e = 31 and a mantissa of 511.
__host__ __device__ __forceinline__ uint32_t encode_rgb9e5(const float4& v)
{
    const float r = encode_clamp(v.x, 0.0f, 65408.0f), g = encode_clamp(v.y, 0.0f, 65408.0f), b = encode_clamp(v.z, 0.0f, 65408.0f);
    const float m = encode_max3(r, g, b);
    const int eb = (int)(encode_bits(m) >> 23) - 127;
    int e = (eb > -16 ? eb : -16) + 16;
    if (__builtin_floorf(m * encode_pow2(24 - e) + 0.5f) == 512.0f) e = e + 1;
    const float scale = encode_pow2(24 - e);
    const uint32_t rm = (uint32_t)__builtin_floorf(r * scale + 0.5f), gm = (uint32_t)__builtin_floorf(g * scale + 0.5f),
                   bm = (uint32_t)__builtin_floorf(b * scale + 0.5f);
    return rm | (gm << 9) | (bm << 18) | ((uint32_t)e << 27);
}

// 4. RGBE8 (Ward's float2rgbe): r, g, b mantissas and the exponent byte in ascending addresses, alpha dropped.  Per channel NaN -> 0 and
// clamp to [0, the largest float below 2^127] (above it e + 128 does not fit a byte).  With v the largest channel: v >= 1e-32f gives
// e = biased exponent of v - 126 (frexp's: v = f * 2^e, f in [0.5, 1)), mantissas floorf(c * 2^(8 - e)) -- exact products below 256 --
// and the exponent byte e + 128; a smaller v gives four zero bytes.  (>= against the float32 constant: gdpathtracing_amd.hdrio compares
// > 1e-32 in binary64, and the float32 nearest to 1e-32 lies above that double.)
__host__ __device__ __forceinline__ uint32_t encode_rgbe8(const float4& v)
{
    const float top = encode_float(0x7effffffu);
    const float r = encode_clamp(v.x, 0.0f, top), g = encode_clamp(v.y, 0.0f, top), b = encode_clamp(v.z, 0.0f, top);
    const float m = encode_max3(r, g, b);
    if (!(m >= 1e-32f)) return 0u;
    const int e = (int)(encode_bits(m) >> 23) - 126;
    const float scale = encode_pow2(8 - e);
    const uint32_t rm = (uint32_t)__builtin_floorf(r * scale), gm = (uint32_t)__builtin_floorf(g * scale), bm = (uint32_t)__builtin_floorf(b * scale);
    return rm | (gm << 8) | (bm << 16) | ((uint32_t)(e + 128) << 24);
}

__host__ __device__ __forceinline__ bool encode_format_known(int32_t format) { return format >= kEncodeRgba16f && format <= kEncodeRgbe8; }
__host__ __device__ __forceinline__ size_t encode_texel_bytes(int32_t format) { return format == kEncodeRgba16f ? 8u : 4u; }

// the whole transform on the host (jpt_debug_encode with JPT_DEVICE_HOST_ONLY): n texels of src to n * encode_texel_bytes(format) bytes
inline void encode_host(int32_t format, const float4* src, uint64_t n, float divisor, bool alpha_one, void* out)
{
    const bool divide = divisor != 1.0f;
    for (uint64_t i = 0; i < n; i++) {
        const float4 v = encode_source(src[i], divisor, divide, alpha_one);
        if (format == kEncodeRgba16f) static_cast<uint2*>(out)[i] = encode_rgba16f(v);
        else static_cast<uint32_t*>(out)[i] = format == kEncodeRgb9e5 ? encode_rgb9e5(v) : encode_rgbe8(v);
    }
}

// jpt_encode's launch (jpt_kernels_encode.hip), on `stream`: n texels of `src` (16-byte aligned, as every float4 image of the context is)
// to `out` (16-byte aligned, n * encode_texel_bytes(format) bytes).  Nothing else is written; n = 0 launches nothing.
void launch_encode(hipStream_t stream, int32_t format, const float4* src, uint64_t n, float divisor, bool alpha_one, void* out);

}  // namespace jpt
