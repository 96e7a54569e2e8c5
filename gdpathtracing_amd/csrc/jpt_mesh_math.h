// jpt_mesh_math.h -- the per-triangle arithmetic of the native BLAS, written once for the host builder (jpt_builder.cpp: flatten,
// SahBlasBuilder) and for the device refit of a deformed mesh (jpt_kernels_mesh.hip, jpt_scene_update_mesh): plain float
// arithmetic only, compiled without contraction on both sides, so the two give the same bits.
#pragma once

#include "jpt_instance_math.h"   // JPT_HD, imin_, imax_
#include "jpt_types.h"

namespace jpt {

// v0 + the two Moller-Trumbore edges (the subtractions of main.glsl:231-232) and cross(e1, e2), each product and difference
// rounded on its own like the shader's (no contraction: Makefile)
JPT_HD void make_wide_tri(const float* a, const float* b, const float* c, WideTri& t)
{
    t.v0[0] = a[0]; t.v0[1] = a[1]; t.v0[2] = a[2];
    t.e1[0] = b[0] - a[0]; t.e1[1] = b[1] - a[1]; t.e1[2] = b[2] - a[2];
    t.e2[0] = c[0] - a[0]; t.e2[1] = c[1] - a[1]; t.e2[2] = c[2] - a[2];
    t.nx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
    t.ny = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
    t.nz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
}

// the padding of a mesh's boxes from the largest |coordinate| of its triangles' vertices (SahBlasBuilder::prepare): every
// Moller-Trumbore-accepted hit also passes the slab test in float
JPT_HD float mesh_box_pad(const float* lo, const float* hi)
{
    float m = 0.0f;
    for (int k = 0; k < 3; k++) m = imax_(m, imax_(iabs_(lo[k]), iabs_(hi[k])));
    return m * 2e-6f + 1e-30f;
}

// float -> int whose order as a signed integer is the float's order (non-NaN floats; -0 sorts below +0): the device reduces the
// mesh's vertex bounds with integer atomics on these, the host presets them
JPT_HD int32_t ordered_key(float f)
{
    union {
        float f;
        int32_t i;
    } v;
    v.f = f;
    return v.i >= 0 ? v.i : v.i ^ 0x7fffffff;
}
JPT_HD float from_ordered_key(int32_t k)
{
    union {
        float f;
        int32_t i;
    } v;
    v.i = k >= 0 ? k : k ^ 0x7fffffff;
    return v.f;
}

}  // namespace jpt
