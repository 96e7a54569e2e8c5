// jpt_reflection.h -- reflection probes, the mip chain (jpt_reflection_prefilter): every probe's strip of six faces (jpt_cube.h) becomes
// a cubemap whose level l holds the radiance convolved with the GGX lobe of roughness l / (n_levels - 1) -- what a ReflectionProbe of
// Godot is read with, mip = roughness * (n_levels - 1).  The radiance is linear and not pre-multiplied by any BRDF term.
//
// Two images, both the call's own (16 B texels):
//   the SOURCE chain, per probe: levels 0 .. log2 S, each 6 faces of s_m x s_m texels (s_m = S >> m), (r, g, b, 0).  Level 0 is
//     accum.rgb / (float)frame_count; texel (i, j) of level m + 1 is ((a + b) + (c + d)) * 0.25 of the block a = (2i, 2j), b = (2i + 1,
//     2j), c = (2i, 2j + 1), d = (2i + 1, 2j + 1) of level m.  Level m of probe p starts at texel p * (8 S^2 - 2) + 8 (S^2 - s_m^2).
//   the OUTPUT chain, level-major: level l holds n * 6 * s_l^2 texels (probe, face, j, i), (r, g, b, 1), and starts at texel
//     n * 8 (S^2 - s_l^2).
//
// Output level 0 is source level 0 with alpha 1.  Output level l >= 1 has roughness r_l = l / (n_levels - 1) and alpha = r_l (the
// renderer's convention: sample_ggx_vndf and evaluate_brdf use roughness^2 as alpha^2; the NDF here is the standard GGX one, the
// reference's un-squared n.h in D is not reproduced).  Its sample table is made on the host in double and rounded to float
// (reflection_sample_table, jpt_primary.cpp): for k = 0 .. K - 1, u1 = (k + 0.5) / K, u2 the base-2 radical inverse of k,
//     cos t = sqrt((1 - u1) / (1 + (alpha^2 - 1) u1)),  phi = 2 pi u2,  h = (sin t cos phi, sin t sin phi, cos t),
//     L = (2 h_z h_x, 2 h_z h_y, 2 h_z^2 - 1)           (view = normal = the texel's direction: the usual split-sum assumption)
// samples with L_z <= 0 are dropped; the weight is w = L_z / sum L_z; the sample reads source level
//     m = clamp(floor(0.5 log2(O_s / O_0) + 0.5) + 1, 0, log2 S),  O_s = 4 / (K D(h_z)),  O_0 = 4 pi / (6 S^2)
// (filtered importance sampling: the level whose texels are about as wide as the sample).  An entry is (L_x, L_y, L_z, w) and the level;
// the kept entries stand first, k ascending.
//
// Output texel (f, i, j) of a level of size s (pinned: a fixed sequence of binary32 operations, tests/np_reflection.py):
//     N = normalize3(face table at a = (2 (i + 0.5)) / s - 1, b = (2 (j + 0.5)) / s - 1)
//     the branch-free frame of Duff et al.: sg = copysign(1, N.z), q = -1 / (sg + N.z), c = (N.x N.y) q,
//         T = (1 + ((sg N.x) N.x) q, sg c, -(sg N.x)),  B = (c, sg + (N.y N.y) q, -N.y)
//     per kept sample, k ascending: d = (T L_x + B L_y) + N L_z, not renormalised; the nearest texel of source level m in direction d:
//         the major axis by |x| >= |y| && |x| >= |z|, else |y| >= |z|, else z; (sc, tc, ma) the face table's inverse; s01 = (sc / ma + 1)
//         0.5; index min((int)(s01 size), size - 1), likewise t; term = c.ch * w_k, acc = acc + term from +0; stored as (r, g, b, 1).
//
// Out of scope: box projection / parallax correction, blending between probes, bilinear or cross-face filtering of the source, the BRDF
// split-sum LUT, an octahedral layout, a jpt_multi_* form, anisotropy, any change to how materials are shaded.  (Half-float and RGBE
// output: jpt_encode.h.)
#pragma once

#include "jpt_cube.h"

namespace jpt {

constexpr int32_t kReflSamplesMin = 8, kReflSamplesMax = 256, kReflSamplesDefault = 64;
constexpr int32_t kReflLevelsMin = 2, kReflLevelsMax = 9;   // log2(256) + 1
constexpr uint8_t kReflNoSample = 0xffu;                     // the level byte of a table entry past the kept ones

// One (cube, chain) shape, by value to the kernels: n probes of face size 1 << shift, per_row strips to an image row; n_levels output
// levels of K samples, of which count[l] are kept at level l (count[0] is not read).
struct ReflDev {
    uint32_t n = 0, per_row = 0, shift = 0, n_levels = 0, samples = 0;
    uint32_t count[kReflLevelsMax] = {};
    __host__ __device__ uint32_t face_size() const { return 1u << shift; }
};

// texels of one probe's source chain; where its level m starts; where output level l starts in a chain of n probes
inline uint64_t refl_probe_texels(uint32_t shift) { return (8ull << (2u * shift)) - 2ull; }
inline uint64_t refl_level_offset(uint32_t shift, uint32_t m) { return 8ull * ((1ull << (2u * shift)) - (1ull << (2u * (shift - m)))); }
inline uint64_t refl_out_offset(uint32_t n, uint32_t shift, uint32_t l) { return (uint64_t)n * refl_level_offset(shift, l); }
inline uint64_t refl_out_texels(uint32_t n, uint32_t shift, uint32_t n_levels)
{
    return n_levels > shift ? (uint64_t)n * refl_probe_texels(shift) : refl_out_offset(n, shift, n_levels);
}

#if defined(__HIPCC__)

// direction d -> (face, s, t) of a level of `size` texels a side: the nearest texel
__host__ __device__ __forceinline__ void refl_lookup(f3 d, uint32_t size, uint32_t& face, uint32_t& si, uint32_t& ti)
{
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    float sc, tc, ma;
    if (ax >= ay && ax >= az) {
        face = d.x < 0.0f ? 1u : 0u;
        sc = d.x < 0.0f ? d.z : -d.z;
        tc = -d.y;
        ma = ax;
    } else if (ay >= az) {
        face = d.y < 0.0f ? 3u : 2u;
        sc = d.x;
        tc = d.y < 0.0f ? -d.z : d.z;
        ma = ay;
    } else {
        face = d.z < 0.0f ? 5u : 4u;
        sc = d.z < 0.0f ? -d.x : d.x;
        tc = -d.y;
        ma = az;
    }
    const float fs = (float)size;
    const float s01 = (sc / ma + 1.0f) * 0.5f, t01 = (tc / ma + 1.0f) * 0.5f;
    // (|sc|, |tc| <= ma, so both products lie in [0, size]; the lower clamp changes no value and keeps a direction that is not a
    // number -- none is made from a finite frame and table -- inside the level)
    const int is = (int)(s01 * fs), it = (int)(t01 * fs), last = (int)size - 1;
    si = (uint32_t)(is < 0 ? 0 : (is < last ? is : last));
    ti = (uint32_t)(it < 0 ? 0 : (it < last ? it : last));
}

// the normal and the tangent frame of output texel (f, i, j) of a level of `size` texels a side
__host__ __device__ __forceinline__ void refl_frame(uint32_t f, uint32_t i, uint32_t j, uint32_t size, f3& n, f3& t, f3& b)
{
    const float fs = (float)size;
    const float ca = (2.0f * ((float)i + 0.5f)) / fs - 1.0f;
    const float cb = (2.0f * ((float)j + 0.5f)) / fs - 1.0f;
    n = normalize3(cube_face_direction(f, ca, cb));
    const float sg = __builtin_copysignf(1.0f, n.z);
    const float q = -1.0f / (sg + n.z);
    const float c = (n.x * n.y) * q;
    const float sx = sg * n.x;
    t = mk3(1.0f + (sx * n.x) * q, sg * c, -sx);
    b = mk3(c, sg + (n.y * n.y) * q, -n.y);
}

// One output texel of level l >= 1: `chain` is the probe's source chain, tab / lvl the level's `count` kept entries.  (The kernel of
// jpt_kernels_reflection.hip is this loop with the table in LDS.)
__host__ __device__ __forceinline__ float4 refl_texel(const float4* __restrict__ chain, uint32_t shift, uint32_t f, uint32_t i, uint32_t j, uint32_t size,
                                                      const float4* tab, const uint8_t* lvl, uint32_t count)
{
    f3 n, t, b;
    refl_frame(f, i, j, size, n, t, b);
    float r = 0.0f, g = 0.0f, bl = 0.0f;
    const uint32_t ss = 1u << (2u * shift);
    for (uint32_t k = 0; k < count; k++) {
        const float4 e = tab[k];
        const uint32_t m = lvl[k];
        const f3 d = (t * e.x + b * e.y) + n * e.z;
        const uint32_t sm = (1u << shift) >> m;
        uint32_t face, si, ti;
        refl_lookup(d, sm, face, si, ti);
        const float4 c = chain[8u * (ss - sm * sm) + (face * sm + ti) * sm + si];
        const float tr = c.x * e.w, tg = c.y * e.w, tb = c.z * e.w;
        r = r + tr;
        g = g + tg;
        bl = bl + tb;
    }
    return make_float4(r, g, bl, 1.0f);
}

// ---- the whole transform as the host runs it (jpt_debug_reflection_prefilter with JPT_DEVICE_HOST_ONLY): plain loops over the functions
// above.  accum4: the image the probes make, row-major; tab / lvl: n_levels * K entries, level l's at l * K (level 0's are not read);
// chain: scratch of n * refl_probe_texels float4; out: the output chain, refl_out_texels float4.
inline void reflection_prefilter_host(const float* accum4, uint32_t frame_count, const ReflDev& rd, const float4* tab, const uint8_t* lvl, float4* chain,
                                      float4* out)
{
    const uint32_t S = rd.face_size(), shift = rd.shift;
    const size_t width = (size_t)rd.per_row * 6u * S;
    const float fc = (float)frame_count;
    const uint64_t per_probe = refl_probe_texels(shift);
    for (uint32_t p = 0; p < rd.n; p++) {
        float4* ch = chain + p * per_probe;
        const size_t x0 = (size_t)(p % rd.per_row) * 6u * S, y0 = (size_t)(p / rd.per_row) * S;
        for (uint32_t f = 0; f < 6; f++)
            for (uint32_t j = 0; j < S; j++)
                for (uint32_t i = 0; i < S; i++) {
                    const float* px = accum4 + 4 * ((y0 + j) * width + x0 + (size_t)f * S + i);
                    ch[((size_t)f * S + j) * S + i] = make_float4(px[0] / fc, px[1] / fc, px[2] / fc, 0.0f);
                }
        for (uint32_t m = 0; m < shift; m++) {
            const uint32_t s0 = S >> m, s1 = s0 >> 1;
            const float4* src = ch + refl_level_offset(shift, m);
            float4* dst = ch + refl_level_offset(shift, m + 1);
            for (uint32_t f = 0; f < 6; f++)
                for (uint32_t j = 0; j < s1; j++)
                    for (uint32_t i = 0; i < s1; i++) {
                        const float4 a = src[((size_t)f * s0 + 2 * j) * s0 + 2 * i], b = src[((size_t)f * s0 + 2 * j) * s0 + 2 * i + 1];
                        const float4 c = src[((size_t)f * s0 + 2 * j + 1) * s0 + 2 * i], d = src[((size_t)f * s0 + 2 * j + 1) * s0 + 2 * i + 1];
                        dst[((size_t)f * s1 + j) * s1 + i] =
                            make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.0f);
                    }
        }
        for (uint32_t l = 0; l < rd.n_levels; l++) {
            const uint32_t s = S >> l;
            float4* o = out + refl_out_offset(rd.n, shift, l) + (size_t)p * 6u * s * s;
            for (uint32_t f = 0; f < 6; f++)
                for (uint32_t j = 0; j < s; j++)
                    for (uint32_t i = 0; i < s; i++) {
                        const size_t at = ((size_t)f * s + j) * s + i;
                        if (l == 0) {
                            const float4 c = ch[at];
                            o[at] = make_float4(c.x, c.y, c.z, 1.0f);
                        } else {
                            o[at] = refl_texel(ch, shift, f, i, j, s, tab + (size_t)l * rd.samples, lvl + (size_t)l * rd.samples, rd.count[l]);
                        }
                    }
        }
    }
}

#endif  // __HIPCC__

}  // namespace jpt
