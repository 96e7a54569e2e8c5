// jpt_sky.h -- the arithmetic of jpt_set_sky ("the procedural sky"): an environment map made on the device from
// the parameters of a gradient sky -- a sky and a ground gradient that meet at the horizon, and a disk with a halo for each sun; the
// form of Godot 4's ProceduralSkyMaterial without its cover texture.  No reference counterpart: the reference has its fixed gradient.
// Every step is one binary32 operation, a compare and select, floor, or an integer / bit operation, in source order: the device kernel
// (jpt_kernels_sky.hip) and the host forms (jpt_debug_sky with JPT_DEVICE_HOST_ONLY, jpt_debug_sky_radiance, jpt_debug_pow01) run
// these functions, and tests/np_sky.py restates them in numpy bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpt_device_math.h"

namespace jpt {

constexpr float kSkyHalfPi = 1.57079637f, kSkyPi = 3.14159274f, kSkyTwoPi = 6.28318548f;   // as jpt_device_math.h writes them
constexpr int kSkyMaxSuns = 4, kSkyMaxSamples = 8;
constexpr int kSkyBlock = 256;   // texels of one row per block

// What the kernel takes, by value: the caller's jpt_sky_params with everything the host derives once per call (sky_params_dev,
// jpt_lighting.cpp) -- the reciprocal curves, and per sun the unit direction (normalised in double, then rounded), the disk's radiance,
// amax = max(sun_angle_max, r) and inv_span = 1 / (amax - r) (0 when the span is 0: no texel takes the halo's branch then).
struct SkySunDev {
    float dir[3];
    float r, amax, inv_span;
    float rad[3];
};
struct SkyDev {
    float sky_top[3], sky_horizon[3], ground_bottom[3], ground_horizon[3];
    float sky_energy, ground_energy, exposure;
    float inv_sky_curve, inv_ground_curve, inv_sun_curve;
    int32_t n_suns;
    SkySunDev suns[kSkyMaxSuns];
};

// 1. pow01_(b, e) = b^e for b in [0, 1] and e in [1/8, 64], as exp2(e * log2 b).  b <= 0 gives 0 and b >= 1 gives 1, exactly.
//    log2 b: the exponent and mantissa are split in integers (a subnormal b is first scaled by 2^24, exactly); the mantissa m in [1, 2)
//    is folded to [sqrt(1/2), sqrt 2) -- m >= 1.41421354f is halved and the exponent raised, so a b just under 1 has exponent 0 and
//    its logarithm keeps its own precision --, then with s = (m - 1) / (m + 1): log2 m = s * (c1 + z (c3 + z (c5 + z (c7 + z c9)))),
//    z = s * s, c_k = 2 / (k ln 2) (the odd series of atanh; |s| <= 0.1716, the first dropped term is below 1e-9).
//    exp2 t, t = e * log2 b <= 0: t < -126 gives 0; n = floor(t + 0.5), f = t - n in [-1/2, 1/2] (exact), x = f * ln 2, the degree-7
//    Taylor polynomial of e^x in Horner form (|x| <= 0.3466: the remainder is below 6e-9), times 2^n made from its bits.  A result
//    below 2^-126 is 0.  The result is at most 1: for n = 0, x <= 0 and the polynomial is 1 + x * (a positive value).
//    Within 2^-21 of the float64 b^e over the whole domain (tests/test_sky_host.py).
__host__ __device__ __forceinline__ float pow01_(float b, float e)
{
    if (!(b > 0.0f)) return 0.0f;
    if (b >= 1.0f) return 1.0f;
    const bool sub = b < 1.17549435e-38f;
    const float bn = sub ? b * 16777216.0f : b;
    const uint32_t u = __builtin_bit_cast(uint32_t, bn);
    int ex = (int)(u >> 23) - (sub ? 151 : 127);
    float m = __builtin_bit_cast(float, (u & 0x007fffffu) | 0x3f800000u);
    if (m >= 1.41421354f) {
        m = m * 0.5f;
        ex = ex + 1;
    }
    const float s = (m - 1.0f) / (m + 1.0f);
    const float z = s * s;
    float p = 0.320598900f;
    p = p * z + 0.412198573f;
    p = p * z + 0.577078044f;
    p = p * z + 0.961796701f;
    p = p * z + 2.88539004f;
    const float l = (float)ex + p * s;
    const float t = e * l;
    if (t < -126.0f) return 0.0f;
    const float nf = __builtin_floorf(t + 0.5f);
    const float x = (t - nf) * 0.693147182f;
    float q = 1.98412701e-4f;
    q = q * x + 1.38888892e-3f;
    q = q * x + 8.33333377e-3f;
    q = q * x + 4.16666679e-2f;
    q = q * x + 0.166666672f;
    q = q * x + 0.5f;
    q = q * x + 1.0f;
    q = q * x + 1.0f;
    const float scale = __builtin_bit_cast(float, (uint32_t)((int)nf + 127) << 23);
    const float r = q * scale;
    return r < 1.17549435e-38f ? 0.0f : r;
}

// 2. the blend weight of a gradient or a halo: 1 - b^(1 / curve), both clamps included
__host__ __device__ __forceinline__ float sky_weight(float b, float inv_curve)
{
    return clamp_(1.0f - pow01_(clamp_(b, 0.0f, 1.0f), inv_curve), 0.0f, 1.0f);
}

// 3. the gradient at polar angle theta from +y, before the suns and the exposure; `upper` is d.y >= 0 of the direction it belongs to.
//    b = theta / (pi / 2): the sky blends horizon -> top with w(b), the ground horizon -> bottom with w(2 - b).
__host__ __device__ __forceinline__ f3 sky_gradient(const SkyDev& P, float theta, bool upper)
{
    const float b = theta / kSkyHalfPi;
    if (upper) {
        const float w = sky_weight(b, P.inv_sky_curve);
        return mk3(mix_(P.sky_horizon[0], P.sky_top[0], w) * P.sky_energy, mix_(P.sky_horizon[1], P.sky_top[1], w) * P.sky_energy,
                   mix_(P.sky_horizon[2], P.sky_top[2], w) * P.sky_energy);
    }
    const float w = sky_weight(2.0f - b, P.inv_ground_curve);
    return mk3(mix_(P.ground_horizon[0], P.ground_bottom[0], w) * P.ground_energy, mix_(P.ground_horizon[1], P.ground_bottom[1], w) * P.ground_energy,
               mix_(P.ground_horizon[2], P.ground_bottom[2], w) * P.ground_energy);
}

// 4. the suns over a gradient colour c of the upper hemisphere, in order: a = atan2_(|L x d|, L . d) (no arccosine: it is ill-conditioned
//    at a sun's size); inside the disk the disk's radiance replaces c, inside the halo c = mix_(R, c, w(1 - (a - r) * inv_span)).  A sun
//    further than amax changes nothing, so its weight is never evaluated.
__host__ __device__ __forceinline__ f3 sky_suns(const SkyDev& P, f3 d, f3 c)
{
    // (unrolled over the four slots with a uniform exit at n_suns: every index into the by-value block is then a constant, so the block
    // stays in scalar registers and is not copied to scratch for a run-time index)
#pragma unroll
    for (int s = 0; s < kSkyMaxSuns; s++) {
        if (s >= P.n_suns) break;
        const SkySunDev& sun = P.suns[s];
        const f3 L = mk3(sun.dir[0], sun.dir[1], sun.dir[2]);
        const f3 x = cross3(L, d);
        const float a = atan2_(__builtin_sqrtf(dot3(x, x)), dot3(L, d));
        if (a < sun.r) {
            c = mk3(sun.rad[0], sun.rad[1], sun.rad[2]);
        } else if (a < sun.amax) {
            const float w = sky_weight(1.0f - (a - sun.r) * sun.inv_span, P.inv_sun_curve);
            c = mk3(mix_(sun.rad[0], c.x, w), mix_(sun.rad[1], c.y, w), mix_(sun.rad[2], c.z, w));
        }
    }
    return c;
}

// 5. sky_radiance(theta, d): d a unit direction in the map's frame, theta its polar angle.  Suns do not show below the horizon.
__host__ __device__ __forceinline__ f3 sky_radiance(const SkyDev& P, float theta, f3 d)
{
    const bool upper = d.y >= 0.0f;
    f3 c = sky_gradient(P, theta, upper);
    if (upper) c = sky_suns(P, d, c);
    return c * P.exposure;
}

// 6. texel (i, j) of a w x h map from n x n subsamples, sub-rows outside: v = ((float)(j n + sj) + 0.5f) / (float)(h n), theta = v * pi,
//    u = ((float)(i n + si) + 0.5f) / (float)(w n), phi = (u - 0.5f) * 2 pi, d = (sin theta sin phi, cos theta, -(sin theta cos phi)) --
//    the inverse of env_radiance's mapping (jpt_shade.h), so texel centres land where the lookup puts them --, the radiances summed from 0
//    in that order, times 1.0f / (float)(n n).  theta is the sub-row's own value, not recomputed from d: the gradient (and which
//    hemisphere) depends on (j, sj) alone and is evaluated once per sub-row.
__host__ __device__ __forceinline__ f3 sky_texel(const SkyDev& P, int32_t w, int32_t h, int32_t n, int32_t i, int32_t j)
{
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    const float rows = (float)(h * n), cols = (float)(w * n);
    for (int32_t sj = 0; sj < n; sj++) {
        const float v = ((float)(j * n + sj) + 0.5f) / rows;
        const float theta = v * kSkyPi;
        float st, ct;
        sincos_(theta, st, ct);
        const bool upper = ct >= 0.0f;
        const f3 g = sky_gradient(P, theta, upper);
        for (int32_t si = 0; si < n; si++) {
            const float u = ((float)(i * n + si) + 0.5f) / cols;
            const float phi = (u - 0.5f) * kSkyTwoPi;
            float sp, cp;
            sincos_(phi, sp, cp);
            const f3 d = mk3(st * sp, ct, -(st * cp));
            const f3 c = upper ? sky_suns(P, d, g) : g;
            sum = sum + c * P.exposure;
        }
    }
    return sum * (1.0f / (float)(n * n));
}

}  // namespace jpt
