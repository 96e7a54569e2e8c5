// jpt_lens.h -- the thin-lens camera (jpt_set_lens): depth of field from an aperture radius and a focus distance.  A primary ray
// leaves a point of a disk around cam.position instead of cam.position itself, towards the point where the pinhole ray of the same
// pixel and frame meets the focal plane.  Nothing downstream of ray generation knows: the rays go into the queues as they are.
//
// The arithmetic is pinned (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations, restated in numpy by
// tests/np_lens.py); host and device run these two functions (the basis on the host once per render, the per-path step in the lens
// forms of the primary kernels, in the audit kernel and in jpt_debug_lens_rays).
#pragma once

#include "jpt_shade.h"

namespace jpt {

// The lens of one render, passed by value to its bounce-0 launch: radius 0 is the pinhole (nothing else is read then).
struct LensDev {
    float radius = 0.0f, focus = 0.0f;
    f3 f = {0.0f, 0.0f, 0.0f}, r = {0.0f, 0.0f, 0.0f}, u = {0.0f, 0.0f, 0.0f};   // forward, right, up (lens_basis)
};

// ivp * (nx, ny, 1, 1), divided by w: primary_ray's four sums and three divisions, the terms in its order
__host__ __device__ __forceinline__ f3 lens_unproject(const RefCamera& cam, float nx, float ny)
{
    const float* m = cam.ivp;
    float wx = m[0] * nx + m[4] * ny + m[8] + m[12];
    float wy = m[1] * nx + m[5] * ny + m[9] + m[13];
    float wz = m[2] * nx + m[6] * ny + m[10] + m[14];
    const float ww = m[3] * nx + m[7] * ny + m[11] + m[15];
    wx = wx / ww;
    wy = wy / ww;
    wz = wz / ww;
    return mk3(wx, wy, wz);
}

// The camera basis from the block the host set (jpt_set_camera), once per render: f through the image centre, r along the image's
// +x made orthogonal to f, u = r x f.  A Godot camera gives forward -z, right +x, up +y.  False when a component is not finite.
__host__ __device__ __forceinline__ bool lens_basis(const RefCamera& cam, LensDev& lens)
{
    const f3 position = mk3(cam.position.x, cam.position.y, cam.position.z);
    const f3 c0 = lens_unproject(cam, 0.0f, 0.0f);
    const f3 f = normalize3(c0 - position);
    const f3 c1 = lens_unproject(cam, 1.0f, 0.0f);
    const f3 r0 = c1 - c0;
    const f3 r = normalize3(r0 - f * dot3(r0, f));
    const f3 u = cross3(r, f);
    lens.f = f;
    lens.r = r;
    lens.u = u;
    const float all[9] = {f.x, f.y, f.z, r.x, r.y, r.z, u.x, u.y, u.z};
    bool finite = true;
    for (int k = 0; k < 9; k++) finite = finite && (all[k] - all[k] == 0.0f);
    return finite;
}

#if defined(__HIPCC__)

// The lens sample of a path, after primary_ray has made `ray` and left (sx, sy) as they are after the jitter draw: its randoms come
// from a COPY of the seeds, one pcg2d round of (sx ^ 0x85ebca6b, sy ^ 0xc2b2ae35) -- constants of its own, the path's sequence does
// not advance, so every later vertex draws what it draws under the pinhole.  (lu, lv) = radius sqrt(xi0) (cos, sin)(2 pi xi1), uniform
// on the disk; p = o + d * (focus / (d.f)) is where the pinhole ray meets the focal plane; the ray leaves (o + r lu) + u lv towards
// p.  A pinhole ray that does not point forward (!(d.f > 0)) is kept as it is.  lens_apply: the step from (xi0, xi1) on.
__host__ __device__ __forceinline__ void lens_apply(const LensDev& lens, float xi0, float xi1, Ray& ray)
{
    const float rad = lens.radius * __builtin_sqrtf(xi0);
    float s, c;
    sincos_(6.2831853f * xi1, s, c);
    const float lu = rad * c, lv = rad * s;
    const float cf = dot3(ray.d, lens.f);
    if (!(cf > 0.0f)) return;
    const float tf = lens.focus / cf;
    const f3 p = ray.o + ray.d * tf;
    const f3 o2 = (ray.o + lens.r * lu) + lens.u * lv;
    ray.o = o2;
    ray.d = normalize3(p - o2);
    ray.rD = rcp3(ray.d);
}
__host__ __device__ __forceinline__ void lens_ray(const LensDev& lens, uint32_t sx, uint32_t sy, Ray& ray)
{
    uint32_t hx = sx ^ 0x85ebca6bu, hy = sy ^ 0xc2b2ae35u;
    float xi0, xi1;
    pcg2d(hx, hy, xi0, xi1);
    lens_apply(lens, xi0, xi1, ray);
}

#endif  // __HIPCC__

}  // namespace jpt
