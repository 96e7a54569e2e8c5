// jpt_kernels_mesh_rebuild.hip -- a new topology for a committed mesh, made on the device (jpt_scene_rebuild_mesh): the mesh's triangles
// sorted along a Morton curve through the centres of their vertex boxes (the arithmetic: jpt_mesh_rebuild.h, which is
// jpt_tlas_rebuild.h's), for any triangle count.  The child words over the sorted triangles are tlas_template_kernel's
// (jpt_kernels_tlas.hip), the boxes and quantised records the refit's (jpt_kernels_mesh.hip).  No reference counterpart: the reference
// rebuilds on the host.
//
// The sort is a stable LSD radix sort, four passes of 8 bits over the 30-bit codes, the triangle indices carried along.  A pass is
// three launches -- the digit histogram of every block's tile into a [digit][block] table, the exclusive scan of the table, the
// scatter -- and the launches are its only seams: no block waits for another, no global atomic decides a position, nothing spills.
#include "jpt_kernels.h"
#include "jpt_mesh_rebuild.h"

namespace jpt {

namespace {

constexpr int kSteps = (int)(kMeshSortTile / (uint32_t)kMeshSortThreads);
static_assert(kMeshSortTile % (uint32_t)kMeshSortThreads == 0 && kMeshSortThreads == 256, "a tile is whole steps of one thread per digit");

__device__ inline int32_t wave_min(int32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ inline int32_t wave_max(int32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__device__ inline void tri_box(const MeshOrderArgs& a, uint32_t i, float* lo, float* hi)
{
    const uint32_t* ix = a.vidx + (size_t)(a.tri_first + i) * 3;
    tri_vertex_box(a.verts + (size_t)ix[0] * 3, a.verts + (size_t)ix[1] * 3, a.verts + (size_t)ix[2] * 3, lo, hi);
}

}  // namespace

// where the minimum and the maximum of the finite centres start
__global__ __launch_bounds__(64) void mesh_order_init_kernel(int32_t* __restrict__ bounds)
{
    if (threadIdx.x < 8) bounds[threadIdx.x] = threadIdx.x < 3 ? kTlasKeyBoundsMin : threadIdx.x < 6 ? kTlasKeyBoundsMax : 0;
}

// One thread per triangle: the bounds of the finite centres per axis, reduced in the wave, then in the block, then with integer atomics
// on ordered keys (order-independent), as mesh_tri_kernel reduces the vertex bounds
__global__ __launch_bounds__(kMeshSortThreads) void mesh_centre_bounds_kernel(MeshOrderArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t kmin[3] = {kTlasKeyBoundsMin, kTlasKeyBoundsMin, kTlasKeyBoundsMin}, kmax[3] = {kTlasKeyBoundsMax, kTlasKeyBoundsMax, kTlasKeyBoundsMax};
    if (i < a.n_tris) {
        float lo[3], hi[3];
        tri_box(a, i, lo, hi);
        for (int k = 0; k < 3; k++) {
            const float c = tlas_centre(lo[k], hi[k]);
            if (tlas_finite(c)) kmin[k] = kmax[k] = ordered_key(c);
        }
    }
    __shared__ int32_t part[kMeshSortWaves][6];
    const uint32_t wave = threadIdx.x >> 6;
    for (int k = 0; k < 3; k++) {
        const int32_t lo = wave_min(kmin[k]), hi = wave_max(kmax[k]);
        if ((threadIdx.x & 63u) == 0) part[wave][k] = lo, part[wave][3 + k] = hi;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int32_t lo = part[0][threadIdx.x], hi = part[0][3 + threadIdx.x];
        for (int w = 1; w < kMeshSortWaves; w++) lo = min(lo, part[w][threadIdx.x]), hi = max(hi, part[w][3 + threadIdx.x]);
        int32_t* bounds = reinterpret_cast<int32_t*>(a.work);
        atomicMin(&bounds[threadIdx.x], lo);
        atomicMax(&bounds[3 + threadIdx.x], hi);
    }
}

// one thread per triangle: its code and its index among the scene's triangles
__global__ __launch_bounds__(kMeshSortThreads) void mesh_codes_kernel(MeshOrderArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_tris) return;
    const int32_t* bounds = reinterpret_cast<const int32_t*>(a.work);
    float bmin[3], inv[3];
    for (int k = 0; k < 3; k++) {
        bmin[k] = from_ordered_key(bounds[k]);
        inv[k] = tlas_inv_extent(bmin[k], from_ordered_key(bounds[3 + k]));
    }
    float lo[3], hi[3];
    tri_box(a, i, lo, hi);
    a.work[8 + i] = mesh_tri_code(lo, hi, bmin, inv);
    a.work[8 + (size_t)a.n_tris + i] = a.tri_first + i;
}

// pass step 1: the digits of the block's tile counted with LDS atomics, into column `block` of the [digit][block] table
__global__ __launch_bounds__(kMeshSortThreads) void mesh_sort_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, int shift, uint32_t* __restrict__ table)
{
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kMeshSortTile;
    for (int s = 0; s < kSteps; s++) {
        const uint32_t i = base + (uint32_t)s * kMeshSortThreads + threadIdx.x;
        if (i < n) atomicAdd(&s_hist[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s_hist[threadIdx.x];
}

// pass step 2: the exclusive scan of the table's `len` words in place, by one block.  Each of the sixteen waves owns `seg` consecutive
// words, which it goes through 64 at a time (coalesced; kScanBatch loads in flight): first their sum, then -- behind the one barrier,
// from the sum of the waves before it -- every word's prefix by a wave scan per 64 words and a running carry.
__global__ __launch_bounds__(kMeshScanThreads) void mesh_sort_scan_kernel(uint32_t* __restrict__ table, uint32_t len, uint32_t seg)
{
    constexpr uint32_t kScanBatch = 8;
    __shared__ uint32_t s_wave[kMeshScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t begin = min(wave * seg, len), end = min(begin + seg, len);
    const uint32_t steps = (seg + 63u) / 64u;
    uint32_t own = 0;
    for (uint32_t k0 = 0; k0 < steps; k0 += kScanBatch)
        for (uint32_t j = 0; j < kScanBatch; j++) {
            const uint32_t i = begin + (k0 + j) * 64u + lane;
            if (i < end) own += table[i];   // (k0 + j >= steps: i >= end)
        }
    for (int d = 32; d > 0; d >>= 1) own += __shfl_xor(own, d);
    if (lane == 0) s_wave[wave] = own;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t w = 0; w < wave; w++) run += s_wave[w];
    for (uint32_t k0 = 0; k0 < steps; k0 += kScanBatch) {
        uint32_t v[kScanBatch];
        for (uint32_t j = 0; j < kScanBatch; j++) {
            const uint32_t i = begin + (k0 + j) * 64u + lane;
            v[j] = i < end ? table[i] : 0u;
        }
        for (uint32_t j = 0; j < kScanBatch; j++) {
            const uint32_t i = begin + (k0 + j) * 64u + lane;
            uint32_t incl = v[j];
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if ((int)lane >= d) incl += up;
            }
            if (i < end) table[i] = run + incl - v[j];
            run += __shfl(incl, 63);
        }
    }
}

// pass step 3: the block reads its tile again, step by step in order.  Inside a wave a key's rank among the equal digits before it comes
// from eight ballots; across the step's waves a per-digit walk over the waves' counts gives each wave's first position and moves the
// digit's next position on (the tile step of tlas_order_kernel).  The digit's first position for this block is the scanned table's.
__global__ __launch_bounds__(kMeshSortThreads) void mesh_sort_scatter_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                             uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out, uint32_t n,
                                                                             int shift, const uint32_t* __restrict__ table)
{
    __shared__ uint32_t s_first[256];
    __shared__ uint32_t s_count[kMeshSortWaves][256];
    __shared__ uint32_t s_offset[kMeshSortWaves][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    s_first[tid] = table[(size_t)tid * gridDim.x + blockIdx.x];
    for (int w = 0; w < kMeshSortWaves; w++) s_count[w][tid] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kMeshSortTile;
    for (int s = 0; s < kSteps; s++) {
        const uint32_t i = base + (uint32_t)s * kMeshSortThreads + tid;
        const bool valid = i < n;
        const uint32_t key = valid ? keys[i] : 0u, val = valid ? vals[i] : 0u;
        const uint32_t digit = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long with = __ballot(valid && bit);
            same &= bit ? with : ~with;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_count[wave][digit] = (uint32_t)__popcll(same);
        __syncthreads();
        {
            uint32_t run = s_first[tid];
            for (int w = 0; w < kMeshSortWaves; w++) {
                const uint32_t cnt = s_count[w][tid];
                s_offset[w][tid] = run;
                s_count[w][tid] = 0;
                run += cnt;
            }
            s_first[tid] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t at = s_offset[wave][digit] + rank;   // (< n: the table counted exactly these keys)
            keys_out[at] = key;
            vals_out[at] = val;
        }
        // (the next step's counts are written after its ballots and read after its first barrier: nobody is still here then)
    }
}

// the root word of every instance of the mesh at `bvh_root` (instance_refit_kernel never writes it)
__global__ __launch_bounds__(256) void mesh_root_word_kernel(WideInstance* __restrict__ winst4, const RefInstance* __restrict__ instances, uint32_t n_instances,
                                                             uint32_t bvh_root, int32_t root)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_instances && instances[i].blas_index == bvh_root) winst4[i].root = root;
}

void launch_mesh_order_codes(hipStream_t stream, const MeshOrderArgs& a)
{
    const uint32_t n = a.n_tris;
    if (n == 0) return;
    const uint32_t per_tri = (n + (uint32_t)kMeshSortThreads - 1u) / (uint32_t)kMeshSortThreads;
    hipLaunchKernelGGL(mesh_order_init_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<int32_t*>(a.work));
    hipLaunchKernelGGL(mesh_centre_bounds_kernel, dim3(per_tri), dim3(kMeshSortThreads), 0, stream, a);
    hipLaunchKernelGGL(mesh_codes_kernel, dim3(per_tri), dim3(kMeshSortThreads), 0, stream, a);
}

void launch_mesh_order_sort(hipStream_t stream, const MeshOrderArgs& a)
{
    const uint32_t n = a.n_tris;
    if (n == 0) return;
    const uint32_t blocks = mesh_sort_blocks(n);
    uint32_t *keys = a.work + 8, *vals = keys + n, *keys2 = vals + n, *vals2 = keys2 + n, *table = vals2 + n;
    const uint32_t len = 256u * blocks, waves = (uint32_t)kMeshScanThreads / 64u, seg = (len + waves - 1u) / waves;
    for (int pass = 0; pass < kMeshSortPasses; pass++) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(mesh_sort_hist_kernel, dim3(blocks), dim3(kMeshSortThreads), 0, stream, keys, n, shift, table);
        hipLaunchKernelGGL(mesh_sort_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, stream, table, len, seg);
        hipLaunchKernelGGL(mesh_sort_scatter_kernel, dim3(blocks), dim3(kMeshSortThreads), 0, stream, keys, vals, keys2, vals2, n, shift, table);
        std::swap(keys, keys2);
        std::swap(vals, vals2);
    }
    static_assert(kMeshSortPasses % 2 == 0, "the sorted triangles end where mesh_order_sorted says");
}

void launch_mesh_root_words(hipStream_t stream, WideInstance* winst4, const RefInstance* instances, uint32_t n_instances, uint32_t bvh_root, int32_t root)
{
    if (n_instances == 0) return;
    hipLaunchKernelGGL(mesh_root_word_kernel, dim3((n_instances + 255u) / 256u), dim3(256), 0, stream, winst4, instances, n_instances, bvh_root, root);
}

}  // namespace jpt
