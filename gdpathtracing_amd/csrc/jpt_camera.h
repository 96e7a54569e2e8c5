// jpt_camera.h -- the camera models (jpt_set_camera_model): how a raster position becomes a primary ray.
//   JPT_CAMERA_PINHOLE     primary_ray (jpt_shade.h): from cam.position towards ivp * (nx, ny, 1, 1) -- not made here;
//   JPT_CAMERA_PROJECTIVE  from ivp * (nx, ny, -1, 1), the position's point on the near plane, towards ivp * (nx, ny, +1, 1), its
//                          point on the far plane: exact for an orthographic matrix (parallel rays), the pinhole's directions with
//                          near-plane clipping for a perspective one, and right for any invertible projection;
//   JPT_CAMERA_EQUIRECT    the full sphere around cam.position in the layout jpt_set_environment reads (the tail of env_sample),
//                          oriented by the basis lens_basis derives: row 0 the up pole, the centre column forward, columns to the right.
// Nothing downstream of ray generation knows: the rays go into the queues as they are, like the lens's.
//
// The arithmetic is pinned (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations, restated in numpy by
// tests/np_camera.py); host and device run these functions (the *_cam forms of the primary kernels, the audit kernel, the guide and
// picking kernels and jpt_debug_camera_rays).
#pragma once

#include "jpt_lens.h"

namespace jpt {

constexpr int32_t kCamPinhole = 0, kCamProjective = 1, kCamEquirect = 2;   // JPT_CAMERA_* of include/jpt.h (asserted in jpt_primary.cpp)

// The model of one render, passed by value to its bounce-0 launch: model 0 is the pinhole (nothing else is read then).
struct CamModelDev {
    int32_t model = kCamPinhole;
    f3 f = {0.0f, 0.0f, 0.0f}, r = {0.0f, 0.0f, 0.0f}, u = {0.0f, 0.0f, 0.0f};   // forward, right, up (lens_basis; read by EQUIRECT)
};

#if defined(__HIPCC__)

// ivp * (nx, ny, -1, 1), divided by its own w: lens_unproject's sums with the third term subtracted
__host__ __device__ __forceinline__ f3 camera_unproject_near(const RefCamera& cam, float nx, float ny)
{
    const float* m = cam.ivp;
    float wx = m[0] * nx + m[4] * ny - m[8] + m[12];
    float wy = m[1] * nx + m[5] * ny - m[9] + m[13];
    float wz = m[2] * nx + m[6] * ny - m[10] + m[14];
    const float ww = m[3] * nx + m[7] * ny - m[11] + m[15];
    wx = wx / ww;
    wy = wy / ww;
    wz = wz / ww;
    return mk3(wx, wy, wz);
}

// The ray of a raster position (fx, fy) in pixels -- (px + jc, py + js) of a path, or an exact position (the guides, picking) --
// under a model that is not the pinhole.  A non-finite component is not treated specially, as primary_ray treats none.
__host__ __device__ __forceinline__ Ray camera_raster_ray(const RefCamera& cam, const CamModelDev& cm, int width, int height, float fx, float fy)
{
    Ray ray;
    if (cm.model == kCamEquirect) {
        const float u = fx / (float)width, v = fy / (float)height;
        const float phi = (u - 0.5f) * 6.2831853f, theta = v * 3.14159265f;
        float st, ct, sp, cp;
        sincos_(theta, st, ct);
        sincos_(phi, sp, cp);
        const float mx = st * sp, my = ct, mz = st * cp;
        ray.o = mk3(cam.position.x, cam.position.y, cam.position.z);
        ray.d = normalize3((cm.r * mx + cm.u * my) + cm.f * mz);
    } else {
        const float scx = fx / (float)width * 2.0f - 1.0f;
        const float scy = fy / (float)height * 2.0f - 1.0f;
        const float nx = scx, ny = -scy;
        const f3 p1 = lens_unproject(cam, nx, ny);
        const f3 p0 = camera_unproject_near(cam, nx, ny);
        ray.o = p0;
        ray.d = normalize3(p1 - p0);
    }
    ray.rD = rcp3(ray.d);
    return ray;
}

// The ray of a path: primary_ray's seed and jitter, draw for draw, so (sx, sy) leave as they do under the pinhole and every later
// vertex draws what it draws today; then the model's ray of the jittered position.
__host__ __device__ __forceinline__ Ray camera_ray(const RefCamera& cam, const CamModelDev& cm, int width, int height, int px, int py, uint32_t frame,
                                                   uint32_t& sx, uint32_t& sy)
{
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    r1 = r1 * 0.25f;
    float js, jc;
    sincos_(6.2831853f * r1, js, jc);
    return camera_raster_ray(cam, cm, width, height, (float)px + jc, (float)py + js);
}

#endif  // __HIPCC__

}  // namespace jpt
