// jpt_lightmap.h -- the arithmetic of jpt_bake_finish ("finishing a lightmap"): what turns the accumulation of a
// bake render into a lightmap an engine can sample -- a chart-aware a-trous filter guided by the bake's own texel images (no guide
// pass is traced: position4 / normal4 ARE the first hits), then a dilation that grows the charts outwards into the invalid texels.
// No reference counterpart.  Everything is + - * /, sqrt (the normal's length, once per texel), fabs, compares and selects, one
// binary32 operation each in source order: the device kernels (jpt_kernels_lightmap.hip) and the host form of jpt_debug_bake_finish
// run these functions (the filter through the one pass body of jpt_atrous_pass.h), and tests/np_lightmap.py restates them in float32
// numpy bit for bit.
//
// Corner cases, as settled here:
//   * an invalid texel's guides are (0, 0, 0, -1) and (0, 0, 0, 0) whatever its images hold (NaN included); its colour is (0, 0, 0, 0)
//     whatever the accumulation holds, before and after every filter pass.
//   * fp2 = 0 (no valid 4-neighbour, or one at the very same position): r2 = 0, so only taps AT the texel's position pass the distance
//     test, and their plane weight is max(0, 1 - 0/0) = 0 -- the texel keeps its own colour (the centre tap alone).
//   * a valid texel whose colour is not finite passes through every filter pass (state 1) and is never a tap; the dilation does not
//     read it either, so a texel whose only neighbours with state > 0 are non-finite stays untouched that pass.
//   * the distance test is `d2 <= sd2 * r2`, sd2 = sigma_distance * sigma_distance: a NaN fails it.
#pragma once

#include "jpt_denoise.h"

namespace jpt {

constexpr int kLightmapMaxPasses = 6;
constexpr int kLightmapMaxDilate = 64;

struct LightmapParams {   // jpt_bake_finish_params
    int32_t passes = 3;
    int32_t normal_power_log2 = 4;
    int32_t dilate = 4;
    float sigma_distance = 4.0f;
    float sigma_plane = 1.0f;
    float sigma_color = 4.0f;
};

// what a filter pass holds of one texel: colour (i_k.rgb, state), xg = (position, fp2; fp2 < 0: invalid) and ng = (unit normal, 0)
struct LightmapTexel {
    float4 c, x, n;
};

// dot(n.xyz, n.xyz) > 0, NaN failing: bake_texel_valid of jpt_bake.h, restated for host C++ (that header needs hipcc)
__host__ __device__ __forceinline__ bool lightmap_texel_valid(const float4& n) { return n.x * n.x + n.y * n.y + n.z * n.z > 0.0f; }

__host__ __device__ __forceinline__ float4 lightmap_invalid_x() { return make_float4(0.0f, 0.0f, 0.0f, -1.0f); }

__host__ __device__ __forceinline__ float lightmap_dist2(const float4& p, const float4& q)
{
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return dx * dx + dy * dy + dz * dz;
}

// ---- 1. prepare: the guides of texel (x, y) from the bake images -------------------------------------------------------------------
// fp2, the texel's squared world footprint: the least |x_q - x_p|^2 over its valid 4-neighbours in the order -x, +x, -y, +y (0: none).
// The MINIMUM: a chart-edge texel whose other neighbour belongs to a chart far away keeps the in-chart distance.
__host__ __device__ __forceinline__ void lightmap_guides(const float4* position4, const float4* normal4, int32_t width, int32_t height, int32_t x, int32_t y,
                                                         float4& xg, float4& ng)
{
    const size_t ip = (size_t)y * (size_t)width + (size_t)x;
    const float4 n = normal4[ip];
    if (!lightmap_texel_valid(n)) {
        xg = lightmap_invalid_x();
        ng = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 p = position4[ip];
    const int ox[4] = {-1, 1, 0, 0}, oy[4] = {0, 0, -1, 1};
    float fp2 = 0.0f;
    bool found = false;
    for (int k = 0; k < 4; k++) {
        const int32_t qx = x + ox[k], qy = y + oy[k];
        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
        const size_t iq = (size_t)qy * (size_t)width + (size_t)qx;
        if (!lightmap_texel_valid(normal4[iq])) continue;
        const float d2 = lightmap_dist2(p, position4[iq]);
        fp2 = found ? (d2 < fp2 ? d2 : fp2) : d2;
        found = true;
    }
    const float inv = 1.0f / __builtin_sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);   // normalize3 of jpt_device_math.h
    xg = make_float4(p.x, p.y, p.z, fp2);
    ng = make_float4(n.x * inv, n.y * inv, n.z * inv, 0.0f);
}

// i_0 = (sum.rgb / frame_count, 1) of a valid texel, (0, 0, 0, 0) of an invalid one (no albedo demodulation: a bake path carries
// throughput 1)
__host__ __device__ __forceinline__ float4 lightmap_colour0(const float4& sum, float fc, const float4& xg)
{
    if (xg.w < 0.0f) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4(sum.x / fc, sum.y / fc, sum.z / fc, 1.0f);
}

// ---- 2. filter -----------------------------------------------------------------------------------------------------------------------
// the constants of one pass
struct LightmapPass {
    int32_t step;      // s = 2^k
    int32_t npow;
    float sd2, sp2;    // sigma_distance^2, sigma_plane^2
    float sc2;         // sc * sc, sc = sigma_color halved once per pass
};

// the edge weight of tap q = p + s * (dx, dy) seen from a valid centre p (not the centre tap itself, whose weight is 1)
__host__ __device__ __forceinline__ float lightmap_edge_weight(const LightmapTexel& p, const LightmapTexel& q, int dx, int dy, const LightmapPass& ps)
{
    if (q.x.w < 0.0f) return 0.0f;
    const float ddx = q.x.x - p.x.x, ddy = q.x.y - p.x.y, ddz = q.x.z - p.x.z;
    const float d2 = ddx * ddx + ddy * ddy + ddz * ddz;
    const float r2 = (float)(ps.step * ps.step * (dx * dx + dy * dy)) * p.x.w;   // (the integer is at most 2^13: its float is exact)
    // world distance may exceed the atlas distance by at most sigma_distance: two charts that touch in the atlas do not mix
    if (!(d2 <= ps.sd2 * r2)) return 0.0f;
    float wn = atrous_pos(p.n.x * q.n.x + p.n.y * q.n.y + p.n.z * q.n.z);
    for (int k = 0; k < ps.npow; k++) wn = wn * wn;
    const float pd = p.n.x * ddx + p.n.y * ddy + p.n.z * ddz;
    const float g = atrous_pos(1.0f - (pd * pd) / (ps.sp2 * r2));   // (0 / 0: NaN, which gives 0)
    const float cx = q.c.x - p.c.x, cy = q.c.y - p.c.y, cz = q.c.z - p.c.z;
    const float wc = 1.0f / (1.0f + (cx * cx + cy * cy + cz * cz) / ps.sc2);
    return (wn * g) * wc;
}

// One valid texel of one pass, as a running sum the caller feeds taps in AtrousSum's order (dy = -2..2 outer, dx = -2..2 inner; taps
// outside the image skipped)
struct LightmapSum {
    float r = 0.0f, g = 0.0f, b = 0.0f, w = 0.0f;
    __host__ __device__ __forceinline__ void tap(const LightmapTexel& p, const LightmapTexel& q, int dx, int dy, const LightmapPass& ps)
    {
        float ew = (dx == 0 && dy == 0) ? 1.0f : lightmap_edge_weight(p, q, dx, dy, ps);
        float wt = (atrous_h(dy + 2) * atrous_h(dx + 2)) * ew;
        if (!atrous_finite3(q.c) || ew != ew) wt = 0.0f;
        const bool use = wt != 0.0f;   // (a tap of weight 0 is not multiplied: inf * 0 must not reach the sums)
        r = r + (use ? q.c.x * wt : 0.0f);
        g = g + (use ? q.c.y * wt : 0.0f);
        b = b + (use ? q.c.z * wt : 0.0f);
        w = w + wt;
    }
    __host__ __device__ __forceinline__ float4 result(const LightmapTexel& p) const
    {
        if (!atrous_finite3(p.c)) return make_float4(p.c.x, p.c.y, p.c.z, 1.0f);
        return make_float4(r / w, g / w, b / w, 1.0f);
    }
};

// what the pass body asks of this filter (AtrousTaps' members): an invalid centre is skipped, and the taps share the pass itself
struct LightmapTaps {
    using Pixel = LightmapTexel;
    using Sum = LightmapSum;
    using Prefilter = AtrousNoPrefilter;
    LightmapPass ps;   // (ps.step: read by the gathered form alone; centre() sets the spacing the taps are at)
    __host__ __device__ __forceinline__ bool skip(const float4& xg) const { return xg.w < 0.0f; }
    __host__ __device__ __forceinline__ LightmapPass centre(int s, const Prefilter&) const
    {
        LightmapPass p = ps;
        p.step = s;
        return p;
    }
    __host__ __device__ __forceinline__ void tap(Sum& sum, const Pixel& p, const Pixel& q, int dx, int dy, const LightmapPass& c) const
    {
        sum.tap(p, q, dx, dy, c);
    }
};

// ---- 3. dilate: one texel of one pass, reading only the previous pass's image ------------------------------------------------------------
// A texel of state 0 with a neighbour of state > 0 and finite colour among its 8 takes their weighted mean (2 for the four edge
// neighbours, 1 for the diagonals; dy = -1..1 outer, dx inner) and state 0.5; every other texel is copied.
__host__ __device__ __forceinline__ float4 lightmap_dilate(const float4* in, int32_t width, int32_t height, int32_t x, int32_t y)
{
    const float4 c = in[(size_t)y * (size_t)width + (size_t)x];
    if (c.w != 0.0f) return c;
    float r = 0.0f, g = 0.0f, b = 0.0f, w = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            const float4 q = in[(size_t)qy * (size_t)width + (size_t)qx];
            if (!(q.w > 0.0f) || !atrous_finite3(q)) continue;
            const float wt = (dx == 0 || dy == 0) ? 2.0f : 1.0f;
            r = r + q.x * wt;
            g = g + q.y * wt;
            b = b + q.z * wt;
            w = w + wt;
        }
    if (!(w > 0.0f)) return c;
    return make_float4(r / w, g / w, b / w, 0.5f);
}

}  // namespace jpt
