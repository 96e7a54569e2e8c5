// jpt_mesh_math.h -- the per-triangle arithmetic of the native BLAS, written once for the host builder (jpt_builder.cpp: flatten,
// SahBlasBuilder) and for the device refit of a deformed mesh (jpt_kernels_mesh.hip, jpt_scene_update_mesh), and the refit
// arithmetic of the four-child records and of the instances' cut boxes, written once for the device refits (jpt_kernels_mesh.hip,
// jpt_kernels_post.hip), the host's mirror of the TLAS refit (jpt_scene_update.cpp) and the host builder (InstanceCuts): plain float
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

// ---- four-child records -------------------------------------------------------------------------------------------------------

// the union of the non-empty slots of record `r` into lo / hi; false (lo / hi untouched): it has none
JPT_HD bool record_union(const WideNode4& r, float* lo, float* hi)
{
    bool any = false;
    for (int j = 0; j < 4; j++) {
        if (r.child[j] == kEmptyChild) continue;
        const float bl[3] = {r.lo_x[j], r.lo_y[j], r.lo_z[j]};
        const float bh[3] = {r.hi_x[j], r.hi_y[j], r.hi_z[j]};
        for (int k = 0; k < 3; k++) {
            lo[k] = any ? imin_(lo[k], bl[k]) : bl[k];
            hi[k] = any ? imax_(hi[k], bh[k]) : bh[k];
        }
        any = true;
    }
    return any;
}

// The slots of one record refitted: a leaf slot (a negative reference) gets leaf_box(reference, lo, hi), an internal slot the union
// of the record below (`records`: the array internal references index; a record with no slot leaves the slot as it is).  Min and
// max are exact, so these are the boxes a host build of the same topology stores.
template <typename LeafBox>
JPT_HD void refit_slots(WideNode4& node, const WideNode4* records, LeafBox leaf_box)
{
    for (int k = 0; k < 4; k++) {
        const int32_t c = node.child[k];
        if (c == kEmptyChild) continue;
        float lo[3], hi[3];
        if (c < 0) leaf_box(c, lo, hi);
        else if (!record_union(records[c], lo, hi)) continue;
        node.lo_x[k] = lo[0]; node.lo_y[k] = lo[1]; node.lo_z[k] = lo[2];
        node.hi_x[k] = hi[0]; node.hi_y[k] = hi[1]; node.hi_z[k] = hi[2];
    }
}

// ---- an instance's world box from a cut through its mesh's tree (InstanceCuts, jpt_builder.cpp) ---------------------------------

// The union of the images of `n` cut boxes under an affine transform (column-major 4 x 4 `m`; `boxes`: centre.xyz, half extent.xyz
// each): centre' -+ |M| half extent (9 + 9 products instead of eight corners x 16).  A few ulp of the coordinates away from the
// corner rule's box: twice its padding, on the union.
JPT_HD void affine_cut_box(const float* m, const float* boxes, uint32_t n, float* lo_out, float* hi_out)
{
    float am[9];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) am[k * 3 + r] = __builtin_fabsf(m[k * 4 + r]);
    float lo[3] = {1e34f, 1e34f, 1e34f}, hi[3] = {-1e34f, -1e34f, -1e34f};   // (locals: no store per box through the out pointers)
    for (uint32_t k = 0; k < n; k++, boxes += 6)
        for (int r = 0; r < 3; r++) {
            const float wc = m[r] * boxes[0] + m[4 + r] * boxes[1] + m[8 + r] * boxes[2] + m[12 + r];
            const float we = am[r] * boxes[3] + am[3 + r] * boxes[4] + am[6 + r] * boxes[5];
            lo[r] = imin_(lo[r], wc - we);
            hi[r] = imax_(hi[r], wc + we);
        }
    float big = 0.0f;
    for (int r = 0; r < 3; r++) big = imax_(big, imax_(__builtin_fabsf(lo[r]), __builtin_fabsf(hi[r])));
    const float pad = big * 4e-6f;
    for (int r = 0; r < 3; r++) {
        lo_out[r] = lo[r] - pad;
        hi_out[r] = hi[r] + pad;
    }
}

// the instance's world box intersected with lo .. hi, unless that box is empty (or NaN) on an axis
JPT_HD void clip_world_box(RefInstance& inst, const float* lo, const float* hi)
{
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return;
    inst.aabbMin = Vec4{imax_(inst.aabbMin.x, lo[0]), imax_(inst.aabbMin.y, lo[1]), imax_(inst.aabbMin.z, lo[2]), inst.aabbMin.w};
    inst.aabbMax = Vec4{imin_(inst.aabbMax.x, hi[0]), imin_(inst.aabbMax.y, hi[1]), imin_(inst.aabbMax.z, hi[2]), inst.aabbMax.w};
}

}  // namespace jpt
