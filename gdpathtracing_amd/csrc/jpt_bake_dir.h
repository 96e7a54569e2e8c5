// jpt_bake_dir.h -- directional lightmaps (jpt_set_bake_directional): beside the sum of a texel's frames (the accumulation, the zeroth
// moment) a bake render keeps the three first moments of the incoming light,
//     M_k.c  =  sum over the frames f, in frame order, of  cur_f.c * d_f.k          k = world x, y, z;  c = r, g, b
// cur_f the frame's value exactly as wf2_accumulate adds it and d_f the direction in which the texel's path of frame f left the
// surface: bake_ray's ray.d (jpt_bake.h) for (px, global py, frame_index + f), not renormalised.  M_k / frame_count estimates
// (1 / pi) * integral of L(w) w_k cos(theta) dw, as accum / frame_count estimates (1 / pi) * integral of L(w) cos(theta) dw.  No SH
// constant is folded in (INTEGRATION.md has the mapping to L1 coefficients).
//
// The direction is bake_ray's, split so that a loop over a texel's frames does not repeat what depends on the texel alone:
//   bake_dir_texel   the normalised normal and the columns of its shading space (get_shading_space, as bake_ray builds them)
//   bake_dir_frame   the seeds, the jitter draw taken and discarded, the round of the copy, sincos_, the two square roots and the
//                    composition
// Every operation and its order are bake_ray's: tests/test_bake_dir_host.py holds the two to the same bits, and tests/np_bake_dir.py
// restates the sum in numpy.  The arithmetic is pinned (DESIGN.md "Pinned semantics"): a product and a sum are two roundings.
#pragma once

#include "jpt_bake.h"

namespace jpt {

#if defined(__HIPCC__)

// the per-texel part of bake_ray's direction: the columns of the shading space of the normalised normal
struct BakeDirTexel {
    f3 c0, c1, c2;
};

__host__ __device__ __forceinline__ BakeDirTexel bake_dir_texel(const float4 n4)
{
    const f3 nrm = normalize3(mk3(n4.x, n4.y, n4.z));
    const float sign = nrm.z > 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + nrm.z);
    const float b = nrm.x * nrm.y * a;
    BakeDirTexel t;
    t.c0 = mk3(1.0f + sign * nrm.x * nrm.x * a, sign * b, -sign * nrm.x);
    t.c1 = mk3(b, sign + nrm.y * nrm.y * a, -nrm.y);
    t.c2 = nrm;
    return t;
}

// the per-frame part: ray.d of bake_ray(p4, n4, px, py, frame, ...) for the texel whose columns are `t`
__host__ __device__ __forceinline__ f3 bake_dir_frame(const BakeDirTexel& t, int px, int py, uint32_t frame)
{
    uint32_t sx, sy;
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    uint32_t hx = sx ^ 0x3c6ef372u, hy = sy ^ 0xa54ff53au;
    float xi0, xi1;
    pcg2d(hx, hy, xi0, xi1);
    float sp, cp;
    sincos_((2.0f * JPT_PI) * xi0, sp, cp);
    const float radius = __builtin_sqrtf(xi1);
    const float z = __builtin_sqrtf(1.0f - radius * radius);
    const f3 local = mk3(radius * cp, radius * sp, z);
    return mk3(t.c0.x * local.x + t.c1.x * local.y + t.c2.x * local.z, t.c0.y * local.x + t.c1.y * local.y + t.c2.y * local.z,
               t.c0.z * local.x + t.c1.z * local.y + t.c2.z * local.z);
}

// A frame's value in JPT_ACCUM_REF_LDR8 as wf2_accumulate adds it: the rgba8 word store_final writes, read back.  (The device's
// from_unorm8 is the IEEE quotient q / 255 for every q in 0 .. 255, which the host takes as it is written.)
__host__ __device__ __forceinline__ f3 bake_dir_ldr8(const f3 r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return mk3(from_unorm8(unorm8(r.x)), from_unorm8(unorm8(r.y)), from_unorm8(unorm8(r.z)));
#else
    const float v[3] = {r.x, r.y, r.z};
    float q[3];
    for (int k = 0; k < 3; k++) {
        const float c = __builtin_fminf(__builtin_fmaxf(v[k], 0.0f), 1.0f);   // (minNum / maxNum: a NaN operand is ignored)
        q[k] = (float)(uint32_t)__builtin_floorf(c * 255.0f + 0.5f) / 255.0f;
    }
    return mk3(q[0], q[1], q[2]);
#endif
}

// the three moments of one texel: m[k] = (M_k.r, M_k.g, M_k.b)
struct BakeMoments {
    f3 m[3];
};

// one frame more, in wf2_accumulate's order: cur * d + M, or cur * d alone for the first frame after a reset
__host__ __device__ __forceinline__ void bake_moments_add(BakeMoments& M, bool have_prev, const f3 cur, const f3 d)
{
    const f3 px = cur * d.x, py = cur * d.y, pz = cur * d.z;
    M.m[0] = have_prev ? px + M.m[0] : px;
    M.m[1] = have_prev ? py + M.m[1] : py;
    M.m[2] = have_prev ? pz + M.m[2] : pz;
}

#endif  // __HIPCC__

}  // namespace jpt
