// jpt_primary_ray.h -- the first ray of (pixel, frame) under a PrimaryRays value (jpt_kernels.h), for host and device: what the
// jpt_debug_*_rays entry points show of a render's ray generation (jpt_debug.hip).  It calls the functions the twelve primary kernels
// and the audit kernel inline, in their combinations; those kernels do not call it (jpt_wf2_paths.h, jpt_ref_frame.h).
#pragma once

#include "jpt_kernels.h"

namespace jpt {

#if defined(__HIPCC__)

// False: the pixel has no path (an invalid texel of a bake render, a tile or a strip without a probe of a probe or cube render), and `ray` is all zeros.
__host__ __device__ __forceinline__ bool first_ray(const PrimaryRays& p, const RefCamera& cam, int width, int height, int px, int py, uint32_t frame, Ray& ray)
{
    uint32_t sx, sy;
    switch (p.kind) {
    case PrimaryRays::kPinhole:
        ray = primary_ray(cam, width, height, px, py, frame, sx, sy);
        return true;
    case PrimaryRays::kLens:
        ray = primary_ray(cam, width, height, px, py, frame, sx, sy);
        lens_ray(p.lens, sx, sy, ray);
        return true;
    case PrimaryRays::kCamModel:
        ray = camera_ray(cam, p.cam_model, width, height, px, py, frame, sx, sy);
        return true;
    case PrimaryRays::kBake: {
        const size_t i = (size_t)py * (size_t)width + (size_t)px;
        const float4 n4 = p.bake.normal[i];
        if (bake_texel_valid(n4)) {
            ray = bake_ray(p.bake.position[i], n4, px, py, frame, sx, sy);
            return true;
        }
        break;
    }
    case PrimaryRays::kProbe: {
        uint32_t q, i, j;
        if (probe_cell(p.probe, px, py, q, i, j)) {
            ray = probe_ray(probe_position(p.probe, q), i, j, p.probe.tile_w(), p.probe.tile_h(), px, py, frame, sx, sy);
            return true;
        }
        break;
    }
    case PrimaryRays::kCube: {
        uint32_t q, f, i, j;
        if (cube_cell(p.cube, px, py, q, f, i, j)) {
            ray = cube_ray(cube_position(p.cube, q), f, i, j, p.cube.face_size(), px, py, frame, sx, sy);
            return true;
        }
        break;
    }
    }
    ray.o = ray.d = ray.rD = mk3(0.0f, 0.0f, 0.0f);
    return false;
}

#endif  // __HIPCC__

}  // namespace jpt
