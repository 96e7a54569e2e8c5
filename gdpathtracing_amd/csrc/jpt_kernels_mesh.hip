// jpt_kernels_mesh.hip -- deforming a committed mesh on the device (jpt_scene_update_mesh): new triangle records from new vertex
// positions, then the boxes of the mesh's four-child BLAS records refitted bottom-up over the topology of the last commit, then
// the mesh's root box in the reference-layout node array the instance refit reads.  No reference counterpart (a changed mesh
// means GeometryGroup3D::build() again there).
//
// Every box is the one a JPT_BUILD_SAH_WATERTIGHT commit of the same topology stores: a leaf slot is the union of its triangles'
// vertex boxes widened by the mesh's padding (SahBlasBuilder::build_into), an internal slot the union of the slots of the record
// below.  Min and max are exact and x -> fl(x - pad) is monotone, so the union of padded boxes is the padded union: the refit
// reproduces the commit's float records bit for bit when the vertices are the committed ones.
#include "jpt_kernels.h"
#include "jpt_mesh_math.h"
#include "jpt_nodeq.h"

namespace jpt {

namespace {

constexpr float kFltMax = 3.40282347e38f;

__device__ __forceinline__ float bound_pad(const int32_t* __restrict__ bounds)
{
    const float lo[3] = {from_ordered_key(bounds[0]), from_ordered_key(bounds[1]), from_ordered_key(bounds[2])};
    const float hi[3] = {from_ordered_key(bounds[3]), from_ordered_key(bounds[4]), from_ordered_key(bounds[5])};
    return mesh_box_pad(lo, hi);
}

// the box of triangles first .. first + count - 1 (device order), unpadded (std::min / std::max from +-FLT_MAX, as Box3::grow)
__device__ __forceinline__ void leaf_box(const MeshRefitArgs& a, uint32_t first, uint32_t count, float* lo, float* hi)
{
    for (int k = 0; k < 3; k++) lo[k] = kFltMax, hi[k] = -kFltMax;
    for (uint32_t t = first; t < first + count; t++)
        for (int j = 0; j < 3; j++) {
            const float* v = a.verts + (size_t)a.vidx[(size_t)t * 3 + j] * 3;
            for (int k = 0; k < 3; k++) {
                lo[k] = imin_(lo[k], v[k]);
                hi[k] = imax_(hi[k], v[k]);
            }
        }
}

__device__ __forceinline__ void leaf_span(int32_t ref, uint32_t& first, uint32_t& count)
{
    const uint32_t l = (uint32_t)~ref;
    first = l & kLeafFirstMask;
    count = (l >> kLeafCountShift) + 1u;
}

// one record: its slots from the leaves' triangles or from the (already refitted) records below (jpt_mesh_math.h), then its
// quantised form
__device__ void refit_record(const MeshRefitArgs& a, uint32_t ri, float pad)
{
    WideNode4* node = a.nodes4 + ri;
    refit_slots(*node, a.nodes4, [&](int32_t ref, float* lo, float* hi) {
        uint32_t first, count;
        leaf_span(ref, first, count);
        leaf_box(a, first, count, lo, hi);
        for (int j = 0; j < 3; j++) lo[j] = lo[j] - pad, hi[j] = hi[j] + pad;
    });
    WideNodeQ q;
    quantize_node4(*node, q);
    a.nodesq[ri] = q;
}

}  // namespace

// One thread per triangle of the mesh: its WideTri (flatten's expressions, jpt_mesh_math.h) and, when normals are given, the vertex
// normals of its ShadeTri; the block's bounds of the vertices go to the mesh's bounds with integer atomics on ordered keys (the
// padding is a function of the mesh's largest |coordinate|, SahBlasBuilder::prepare).
__global__ __launch_bounds__(256) void mesh_tri_kernel(MeshRefitArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float lo[3] = {kFltMax, kFltMax, kFltMax}, hi[3] = {-kFltMax, -kFltMax, -kFltMax};
    if (i < a.n_tris) {
        const uint32_t t = a.tri_first + i;
        const uint32_t ix[3] = {a.vidx[(size_t)t * 3], a.vidx[(size_t)t * 3 + 1], a.vidx[(size_t)t * 3 + 2]};
        float v[3][3];
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) {
                v[j][k] = a.verts[(size_t)ix[j] * 3 + k];
                lo[k] = imin_(lo[k], v[j][k]);
                hi[k] = imax_(hi[k], v[j][k]);
            }
        WideTri w;
        make_wide_tri(v[0], v[1], v[2], w);
        a.wtris[t] = w;
        if (a.normals) {
            ShadeTri& s = a.shade[t];
            for (int k = 0; k < 3; k++) {
                s.n0[k] = a.normals[(size_t)ix[0] * 3 + k];
                s.n1[k] = a.normals[(size_t)ix[1] * 3 + k];
                s.n2[k] = a.normals[(size_t)ix[2] * 3 + k];
            }
        }
    }
    // (no NaN reaches the reduction: imin_ / imax_ from +-FLT_MAX skip a NaN coordinate, as Box3::grow does)
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
        }
    __shared__ float part[4][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) part[wave][k] = lo[k], part[wave][3 + k] = hi[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); w++)
            for (int k = 0; k < 3; k++) {
                lo[k] = fminf(lo[k], part[w][k]);
                hi[k] = fmaxf(hi[k], part[w][3 + k]);
            }
        for (int k = 0; k < 3; k++) {
            atomicMin(&a.bounds[k], ordered_key(lo[k]));
            atomicMax(&a.bounds[3 + k], ordered_key(hi[k]));
        }
    }
}

// one level of the mesh's schedule, one thread per record (the wide levels near the leaves)
__global__ __launch_bounds__(256) void mesh_refit_level_kernel(MeshRefitArgs a, uint32_t begin, uint32_t end)
{
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end) return;
    refit_record(a, a.order[i], bound_pad(a.bounds));
}

// the remaining levels in one block, deepest first; __syncthreads orders the levels (as tlas4_refit_kernel)
__global__ __launch_bounds__(1024) void mesh_refit_top_kernel(MeshRefitArgs a, uint32_t first_level, uint32_t n_levels)
{
    const float pad = bound_pad(a.bounds);
    for (uint32_t l = first_level; l < n_levels; l++) {
        for (uint32_t i = a.level_start[l] + threadIdx.x; i < a.level_start[l + 1]; i += blockDim.x) refit_record(a, a.order[i], pad);
        __syncthreads();
    }
}

// The mesh's root box into the reference-layout node array (what instance_refit_kernel bounds an instance by), and the cut boxes
// of the mesh's instances dropped (they are boxes of the committed vertices): one thread per instance, thread 0 the root.
__global__ __launch_bounds__(256) void mesh_root_kernel(MeshRefitArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        float lo[3], hi[3];
        bool any = true;
        if (a.root4 >= 0) {
            any = record_union(a.nodes4[a.root4], lo, hi);
        } else {
            uint32_t first, count;
            leaf_span(a.root4, first, count);
            leaf_box(a, first, count, lo, hi);
            const float pad = bound_pad(a.bounds);
            for (int k = 0; k < 3; k++) lo[k] = lo[k] - pad, hi[k] = hi[k] + pad;
        }
        if (any) {
            RefBvhNode& r = a.bvh[a.bvh_root];
            r.aabbMin.x = lo[0]; r.aabbMin.y = lo[1]; r.aabbMin.z = lo[2];
            r.aabbMax.x = hi[0]; r.aabbMax.y = hi[1]; r.aabbMax.z = hi[2];
        }
    }
    if (i < a.n_instances && a.cut_range && a.instances[i].blas_index == a.bvh_root) a.cut_range[2 * (size_t)i + 1] = 0u;
}

void launch_mesh_refit(hipStream_t stream, const MeshRefitArgs& a, const uint32_t* h_level_start, uint32_t n_levels)
{
    launch_mesh_tris(stream, a);
    launch_mesh_records(stream, a, h_level_start, n_levels);
}

void launch_mesh_tris(hipStream_t stream, const MeshRefitArgs& a)
{
    if (a.n_tris == 0) return;
    hipLaunchKernelGGL(mesh_tri_kernel, dim3((a.n_tris + 255u) / 256u), dim3(256), 0, stream, a);
}

void launch_mesh_records(hipStream_t stream, const MeshRefitArgs& a, const uint32_t* h_level_start, uint32_t n_levels)
{
    if (a.n_tris == 0) return;
    // a grid per level up to the last level that holds more records than one block has threads, then one block for the levels
    // above it (a small mesh: one launch)
    uint32_t split = n_levels;
    while (split > 0 && h_level_start[split] - h_level_start[split - 1] <= 1024u) split--;
    for (uint32_t l = 0; l < split; l++) {
        const uint32_t n = h_level_start[l + 1] - h_level_start[l];
        if (n) hipLaunchKernelGGL(mesh_refit_level_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, h_level_start[l], h_level_start[l + 1]);
    }
    if (split < n_levels) hipLaunchKernelGGL(mesh_refit_top_kernel, dim3(1), dim3(1024), 0, stream, a, split, n_levels);
    const uint32_t n_threads = a.n_instances > 0u ? a.n_instances : 1u;
    hipLaunchKernelGGL(mesh_root_kernel, dim3((n_threads + 255u) / 256u), dim3(256), 0, stream, a);
}

}  // namespace jpt
