// jpt_skin.h -- blend shapes and linear blend skinning of one vertex (jpt_scene_pose_mesh): the functions mesh_skin_kernel
// (jpt_kernels_skin.hip) and the host form of jpt_debug_skin inline.  What Godot computes for a MeshInstance3D with a Skeleton3D /
// Skin and an ArrayMesh's blend shapes in relative mode (deltas); no reference counterpart (a changed mesh means
// GeometryGroup3D::build() again there).
//
// Every + and * below is one binary32 operation in the order written (-ffp-contract=off: no fma); DESIGN.md "Pinned semantics".
//
//   blend shapes   for each ACTIVE shape (weight != 0, ascending shape index): p = p + dP[s][v] * w per component, and
//                  n = n + dN[s][v] * w when the rig has normal deltas.  Nothing is normalised here.
//   skinning       K = 4 or 8 influences (K = 0: skipped).  M = B[b_0] * w_0 per entry of the transform12 layout (basis rows xx xy xz
//                  yx yy yz zx zy zz, then the origin), then M = M + B[b_i] * w_i for i = 1 .. K-1 in order -- every influence, zero
//                  weights included, weights as given.  x' = M[0]*x + M[1]*y + M[2]*z + M[9] left to right (y': 3 4 5 10, z': 6 7 8
//                  11); the normal takes the same rows without the origin (the blended matrix itself, not its inverse transpose).
//   normal         normalize3 of the result, once, at the end (also with K = 0); a degenerate result is what normalize3 gives.
#pragma once

#include "jpt_device_math.h"

namespace jpt {

constexpr int32_t kSkinMaxShapes = 256;     // blend shapes per rig (the active list's bound)
constexpr int32_t kSkinMaxBone = 4095;      // largest bone index (indices are stored in 16 bits)

// one active blend shape of a pose
struct SkinShape {
    uint32_t shape;
    float weight;
};

// p (and n, when dn is given) moved by shape s's delta of the vertex: d points at the vertex's three floats of the shape
__host__ __device__ __forceinline__ f3 skin_morph(f3 p, const float* __restrict__ d, float w)
{
    return mk3(p.x + d[0] * w, p.y + d[1] * w, p.z + d[2] * w);
}

// the twelve floats of bone b of a palette
__host__ __device__ __forceinline__ void skin_bone(const float* __restrict__ palette, uint32_t b, float* __restrict__ m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // (the staged palette is 16-byte aligned: three 16-byte loads)
    const float4* q = reinterpret_cast<const float4*>(palette) + (size_t)b * 3;
    const float4 r0 = q[0], r1 = q[1], r2 = q[2];
    m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w;
    m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
    m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
#else
    for (int j = 0; j < 12; j++) m[j] = palette[(size_t)b * 12 + j];
#endif
}

// the blended matrix of a vertex's K influences
template <int K>
__host__ __device__ __forceinline__ void skin_matrix(const float* __restrict__ palette, const uint32_t* __restrict__ bone,
                                                     const float* __restrict__ weight, float* __restrict__ m)
{
    float b[12];
    skin_bone(palette, bone[0], b);
    for (int j = 0; j < 12; j++) m[j] = b[j] * weight[0];
#pragma unroll
    for (int i = 1; i < K; i++) {
        skin_bone(palette, bone[i], b);
        for (int j = 0; j < 12; j++) m[j] = m[j] + b[j] * weight[i];
    }
}

__host__ __device__ __forceinline__ f3 skin_point(const float* __restrict__ m, f3 p)
{
    return mk3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[9], m[3] * p.x + m[4] * p.y + m[5] * p.z + m[10],
               m[6] * p.x + m[7] * p.y + m[8] * p.z + m[11]);
}
__host__ __device__ __forceinline__ f3 skin_dir(const float* __restrict__ m, f3 d)
{
    return mk3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[3] * d.x + m[4] * d.y + m[5] * d.z, m[6] * d.x + m[7] * d.y + m[8] * d.z);
}

// A rig as the device holds it (and the host form reads it): one mesh's vertices end to end, every array 16-byte aligned.
struct SkinRig {
    const float* bind_pos = nullptr;       // n_vertices x 3
    const float* bind_nrm = nullptr;       // the same, or null: the mesh's normals are not touched
    const uint16_t* bones = nullptr;       // n_vertices x influences
    const float* weights = nullptr;        // n_vertices x influences
    const float* dpos = nullptr;           // n_shapes x n_vertices x 3, shape-major
    const float* dnrm = nullptr;           // the same, or null: normals are not morphed
    uint32_t n_vertices = 0;
};

// One vertex of a pose: `active` lists the n_active shapes with a weight != 0 in ascending shape order; `palette`: 12 floats per bone.
// K is the rig's influence count (0, 4 or 8).
template <int K>
__host__ __device__ __forceinline__ void skin_vertex(const SkinRig& r, uint32_t v, const SkinShape* __restrict__ active, uint32_t n_active,
                                                     const float* __restrict__ palette, f3& p_out, f3& n_out)
{
    const bool with_n = r.bind_nrm != nullptr;
    f3 p = mk3(r.bind_pos[(size_t)v * 3], r.bind_pos[(size_t)v * 3 + 1], r.bind_pos[(size_t)v * 3 + 2]);
    f3 n = with_n ? mk3(r.bind_nrm[(size_t)v * 3], r.bind_nrm[(size_t)v * 3 + 1], r.bind_nrm[(size_t)v * 3 + 2]) : mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t k = 0; k < n_active; k++) {
        const size_t at = ((size_t)active[k].shape * r.n_vertices + v) * 3;
        const float w = active[k].weight;
        p = skin_morph(p, r.dpos + at, w);
        if (with_n && r.dnrm) n = skin_morph(n, r.dnrm + at, w);
    }
    if (K > 0) {
        uint32_t bone[K > 0 ? K : 1];
        float weight[K > 0 ? K : 1];
#if defined(__HIP_DEVICE_COMPILE__)
        // K x 16 bits and K floats per vertex: 8- and 16-byte loads
        if (K == 4) {
            const uint2 q = reinterpret_cast<const uint2*>(r.bones)[v];
            bone[0] = q.x & 0xffffu; bone[1] = q.x >> 16; bone[2] = q.y & 0xffffu; bone[3] = q.y >> 16;
        } else {
            const uint4 q = reinterpret_cast<const uint4*>(r.bones)[v];
            const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
            for (int i = 0; i < K; i++) bone[i] = (i & 1) ? w4[i >> 1] >> 16 : w4[i >> 1] & 0xffffu;
        }
        for (int i = 0; i < K; i += 4) {
            const float4 w = reinterpret_cast<const float4*>(r.weights)[((size_t)v * K + i) >> 2];
            weight[i] = w.x; weight[i + 1] = w.y; weight[i + 2] = w.z; weight[i + 3] = w.w;
        }
#else
        for (int i = 0; i < K; i++) bone[i] = r.bones[(size_t)v * K + i], weight[i] = r.weights[(size_t)v * K + i];
#endif
        float m[12];
        skin_matrix<(K > 0 ? K : 1)>(palette, bone, weight, m);
        p = skin_point(m, p);
        if (with_n) n = skin_dir(m, n);
    }
    p_out = p;
    n_out = with_n ? normalize3(n) : n;
}

// the whole mesh in plain loops (jpt_debug_skin with JPT_DEVICE_HOST_ONLY): packed float3 outputs, normals_out untouched without normals
inline void skin_host(const SkinRig& r, int32_t influences, const SkinShape* active, uint32_t n_active, const float* palette,
                      float* positions_out, float* normals_out)
{
    for (uint32_t v = 0; v < r.n_vertices; v++) {
        f3 p, n;
        if (influences == 8) skin_vertex<8>(r, v, active, n_active, palette, p, n);
        else if (influences == 4) skin_vertex<4>(r, v, active, n_active, palette, p, n);
        else skin_vertex<0>(r, v, active, n_active, palette, p, n);
        positions_out[(size_t)v * 3] = p.x; positions_out[(size_t)v * 3 + 1] = p.y; positions_out[(size_t)v * 3 + 2] = p.z;
        if (r.bind_nrm) normals_out[(size_t)v * 3] = n.x, normals_out[(size_t)v * 3 + 1] = n.y, normals_out[(size_t)v * 3 + 2] = n.z;
    }
}

}  // namespace jpt
