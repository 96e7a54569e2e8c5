// jpt_mesh_rebuild.h -- the arithmetic of jpt_scene_rebuild_mesh, written once for the device (jpt_kernels_mesh_rebuild.hip) and for
// jpt_debug_mesh_order's host form: a triangle's vertex box, and its 30-bit Morton code, which is the TLAS rebuild's code of that box
// (jpt_tlas_rebuild.h: no float step of its own).  The topology over the sorted triangles is make_tlas_template's.
#pragma once

#include "jpt_tlas_rebuild.h"

namespace jpt {

// The sort of jpt_scene_rebuild_mesh: a stable LSD radix sort over the 30-bit codes, 8 bits per pass.  A block of kMeshSortThreads
// threads owns a tile of kMeshSortTile consecutive keys, which it goes through in kMeshSortTile / kMeshSortThreads steps, in order.
constexpr int kMeshSortThreads = 256, kMeshSortWaves = kMeshSortThreads / 64;
constexpr uint32_t kMeshSortTile = 2048u;
constexpr int kMeshSortPasses = 4;
constexpr int kMeshScanThreads = 1024;   // the one block that scans a pass's [digit][block] table
constexpr uint32_t kMeshRebuildMaxTris = kLeafFirstMask + 1u;   // a leaf reference names one triangle of the scene in 25 bits

inline uint32_t mesh_sort_blocks(uint32_t n) { return (n + kMeshSortTile - 1u) / kMeshSortTile; }
// The sort's working set in 32-bit words: [8: the centre bounds, 6 ordered keys + pad][codes, n][triangles, n][codes', n][triangles', n]
// [the table, 256 x blocks].  After the (even number of) passes the sorted triangles are where the codes kernel wrote them.
inline size_t mesh_sort_words(uint32_t n) { return 8u + 4u * (size_t)n + 256u * (size_t)mesh_sort_blocks(n); }

// the box of a triangle's three vertices as leaf_box takes them (jpt_kernels_mesh.hip): from +-FLT_MAX, so a NaN coordinate is skipped
JPT_HD void tri_vertex_box(const float* v0, const float* v1, const float* v2, float* lo, float* hi)
{
    const float* v[3] = {v0, v1, v2};
    for (int k = 0; k < 3; k++) lo[k] = 3.40282347e38f, hi[k] = -3.40282347e38f;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) {
            lo[k] = imin_(lo[k], v[j][k]);
            hi[k] = imax_(hi[k], v[j][k]);
        }
}

// the code part of tlas_key of the box
JPT_HD uint32_t mesh_tri_code(const float* lo, const float* hi, const float* bmin, const float* inv)
{
    return (uint32_t)(tlas_key(lo, hi, bmin, inv, 0u) >> 15);
}

// ---- host only ----

// The host form of the order kernels: `vidx` holds three indices into `verts` (3 floats each) per triangle; codes per triangle (may be
// null) and the triangle (0 .. n - 1) at each sorted position: ascending by (code, triangle)
inline void mesh_order_host(const float* verts, const uint32_t* vidx, uint32_t n, uint32_t* codes_out, uint32_t* sorted_out)
{
    std::vector<float> lo((size_t)n * 3), hi((size_t)n * 3);
    for (uint32_t i = 0; i < n; i++)
        tri_vertex_box(verts + (size_t)vidx[(size_t)i * 3] * 3, verts + (size_t)vidx[(size_t)i * 3 + 1] * 3, verts + (size_t)vidx[(size_t)i * 3 + 2] * 3,
                       &lo[(size_t)i * 3], &hi[(size_t)i * 3]);
    int32_t kmin[3] = {kTlasKeyBoundsMin, kTlasKeyBoundsMin, kTlasKeyBoundsMin}, kmax[3] = {kTlasKeyBoundsMax, kTlasKeyBoundsMax, kTlasKeyBoundsMax};
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const float c = tlas_centre(lo[(size_t)i * 3 + k], hi[(size_t)i * 3 + k]);
            if (!tlas_finite(c)) continue;
            kmin[k] = std::min(kmin[k], ordered_key(c));
            kmax[k] = std::max(kmax[k], ordered_key(c));
        }
    float bmin[3], inv[3];
    for (int k = 0; k < 3; k++) {
        bmin[k] = from_ordered_key(kmin[k]);
        inv[k] = tlas_inv_extent(bmin[k], from_ordered_key(kmax[k]));
    }
    std::vector<uint64_t> keys(n);   // code above the triangle: unique, so std::sort gives the stable order
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t code = mesh_tri_code(&lo[(size_t)i * 3], &hi[(size_t)i * 3], bmin, inv);
        if (codes_out) codes_out[i] = code;
        keys[i] = ((uint64_t)code << 32) | i;
    }
    std::sort(keys.begin(), keys.end());
    for (uint32_t p = 0; p < n; p++) sorted_out[p] = (uint32_t)(keys[p] & 0xffffffffull);
}

}  // namespace jpt
