// jpt_denoise.h -- the arithmetic of jpt_denoise's filter ("the a-trous filter"): an edge-avoiding a-trous
// wavelet filter (Dammertz et al. 2010) over the demodulated running mean, guided by first-hit position, normal and albedo.
// No reference counterpart (the reference lists a denoiser among its wanted features).  Everything is + - * /, fabs, compares and
// selects, one binary32 operation each in source order: the device kernels (jpt_kernels_denoise.hip) and the host form of
// jpt_debug_atrous run these functions through the one pass body of jpt_atrous_pass.h, and tests/np_denoise.py restates them in
// float32 numpy bit for bit.
#pragma once

#include "../../include/jpt.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jpt {

constexpr int kAtrousMaxPasses = 6;
constexpr float kAlbedoFloor = 0.015625f;   // 2^-6: the least albedo a mean is divided by

struct AtrousParams {   // jpt_denoise_params
    int32_t passes = 5;
    int32_t normal_power_log2 = 6;
    float sigma_plane = 0.02f;
    float sigma_color = 4.0f;
};
// (null: the defaults) -- for jpt_set_denoise_params and the jpt_debug_* entries alike
inline AtrousParams denoise_params_of(const jpt_denoise_params* p)
{
    return p ? AtrousParams{p->passes, p->normal_power_log2, p->sigma_plane, p->sigma_color} : AtrousParams();
}

// what a filter pass holds of one pixel: colour i_k, position_t (xyz, hit distance; t < 0: a miss) and normal
struct AtrousPixel {
    float4 c, x, n;
};

__host__ __device__ __forceinline__ bool atrous_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e38f; }
__host__ __device__ __forceinline__ bool atrous_finite3(const float4& c) { return atrous_finite(c.x) && atrous_finite(c.y) && atrous_finite(c.z); }
__host__ __device__ __forceinline__ float atrous_pos(float v) { return v > 0.0f ? v : 0.0f; }   // max(0, v); a NaN gives 0

// the binomial kernel (1 4 6 4 1) / 16
__host__ __device__ __forceinline__ float atrous_h(int k)
{
    return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f);
}

// per-channel divisor of the demodulation: max(albedo, 2^-6); a NaN gives the floor
__host__ __device__ __forceinline__ float4 atrous_amod(const float4& albedo)
{
    return make_float4(albedo.x > kAlbedoFloor ? albedo.x : kAlbedoFloor, albedo.y > kAlbedoFloor ? albedo.y : kAlbedoFloor,
                       albedo.z > kAlbedoFloor ? albedo.z : kAlbedoFloor, 0.0f);
}
// i_0 = (sum / frame_count) / amod
__host__ __device__ __forceinline__ float4 atrous_demodulate(const float4& sum, float fc, const float4& albedo)
{
    const float4 a = atrous_amod(albedo);
    return make_float4((sum.x / fc) / a.x, (sum.y / fc) / a.y, (sum.z / fc) / a.z, 0.0f);
}

// the geometric weight e of tap q seen from centre p: misses see only misses; else the normal weight times the plane weight
__host__ __device__ __forceinline__ float atrous_geom_weight(const AtrousPixel& p, const AtrousPixel& q, int npow, float sigma_plane)
{
    const bool pm = p.x.w < 0.0f, qm = q.x.w < 0.0f;
    if (pm && qm) return 1.0f;
    if (pm || qm) return 0.0f;
    float wn = atrous_pos(p.n.x * q.n.x + p.n.y * q.n.y + p.n.z * q.n.z);
    for (int k = 0; k < npow; k++) wn = wn * wn;
    const float dx = q.x.x - p.x.x, dy = q.x.y - p.x.y, dz = q.x.z - p.x.z;
    const float rz = __builtin_fabsf(p.n.x * dx + p.n.y * dy + p.n.z * dz) / (sigma_plane * p.x.w);
    const float g = atrous_pos(1.0f - rz);
    return wn * (g * g);
}

// e * wc of tap q seen from centre p (not the centre tap itself, whose e * wc is 1 by definition); sc2 = sc * sc, sc = sigma_color
// halved once per pass
__host__ __device__ __forceinline__ float atrous_edge_weight(const AtrousPixel& p, const AtrousPixel& q, int npow, float sigma_plane, float sc2)
{
    const float e = atrous_geom_weight(p, q, npow, sigma_plane);
    const float cx = q.c.x - p.c.x, cy = q.c.y - p.c.y, cz = q.c.z - p.c.z;
    const float wc = 1.0f / (1.0f + (cx * cx + cy * cy + cz * cz) / sc2);
    return e * wc;
}

// One pixel of one pass, as a running sum the caller feeds taps in the pinned order (dy = -2..2 outer, dx = -2..2 inner; taps
// outside the image skipped)
struct AtrousSum {
    float r = 0.0f, g = 0.0f, b = 0.0f, w = 0.0f;
    __host__ __device__ __forceinline__ void tap(const AtrousPixel& p, const AtrousPixel& q, int dx, int dy, int npow, float sigma_plane, float sc2)
    {
        float ew = (dx == 0 && dy == 0) ? 1.0f : atrous_edge_weight(p, q, npow, sigma_plane, sc2);
        float wt = (atrous_h(dy + 2) * atrous_h(dx + 2)) * ew;
        if (!atrous_finite3(q.c) || ew != ew) wt = 0.0f;
        // (a tap of weight 0 adds nothing -- it is not multiplied: inf * 0 must not reach the sums)
        const bool use = wt != 0.0f;
        r = r + (use ? q.c.x * wt : 0.0f);
        g = g + (use ? q.c.y * wt : 0.0f);
        b = b + (use ? q.c.z * wt : 0.0f);
        w = w + wt;
    }
    __host__ __device__ __forceinline__ float4 result(const AtrousPixel& p) const
    {
        if (!atrous_finite3(p.c)) return make_float4(p.c.x, p.c.y, p.c.z, 0.0f);
        return make_float4(r / w, g / w, b / w, 0.0f);
    }
};

// ---- what the one pass body (jpt_atrous_pass.h: atrous_pass on the device, atrous_passes_host on the host) asks of a filter -----
// A filter's Taps holds the constants of one pass and names its Pixel, Sum and Prefilter (AtrousNoPrefilter: none).  skip(x): a
// centre with guide x is written as zeros; centre(s, pre): what the taps of one centre share, from the tap spacing and the fed
// prefilter; tap(): Sum::tap with it.
struct AtrousNoPrefilter {};

struct AtrousTaps {
    using Pixel = AtrousPixel;
    using Sum = AtrousSum;
    using Prefilter = AtrousNoPrefilter;
    int32_t npow;
    float sigma_plane, sc2;   // sc2 = sc * sc, sc = sigma_color halved once per pass
    __host__ __device__ __forceinline__ bool skip(const float4&) const { return false; }
    __host__ __device__ __forceinline__ float centre(int, const Prefilter&) const { return sc2; }
    __host__ __device__ __forceinline__ void tap(Sum& sum, const Pixel& p, const Pixel& q, int dx, int dy, float c) const
    {
        sum.tap(p, q, dx, dy, npow, sigma_plane, c);
    }
};

}  // namespace jpt
