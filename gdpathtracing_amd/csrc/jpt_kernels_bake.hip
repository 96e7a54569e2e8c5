// jpt_kernels_bake.hip -- lightmap baking's own kernels (jpt_bake.h has the arithmetic): the UV2 rasteriser of jpt_bake_add_surface
// and its host form (the same __host__ __device__ functions in a plain loop).  The bake forms of the bounce-0 kernels are in
// jpt_kernels_wf2.hip (jpt_wf2_paths.h, JPT_BAKE), the audit kernel's branch in jpt_ref_frame.h; the argument checks and the
// context's entry points in jpt_primary.cpp; the probe of jpt_debug_bake_rays in jpt_debug.hip.
//
// The rasteriser is three launches on one stream:
//   bake_clear    winner[i] = 0xffffffff for every texel;
//   bake_cover    one thread per triangle: walk the texels of its clipped bounding box (bake_tri_box), atomicMin(winner, t) where the texel's centre
//                 is covered (bake_cover, jpt_bake.h) -- the lowest triangle index wins a texel whatever the threads' order;
//   bake_write    one thread per texel with a winner: bake_resolve -> position4, normal4.  Texels without one keep what they held,
//                 so a later surface replaces what its own triangles cover and leaves the rest.
// Coverage is decided at texel centres (no conservative rasterisation, no dilation: include/jpt.h says what is out of scope).  One
// thread walks a whole triangle: a lightmap's triangles are many and small, and the walk's cost is the box's area, at most the image.
#include "../../include/jpt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "jpt_kernels.h"

namespace jpt {

namespace {

constexpr int kBakeBlock = 256;

__global__ __launch_bounds__(kBakeBlock) void bake_clear(uint32_t* __restrict__ winner, uint32_t n)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBakeBlock + threadIdx.x;
    if (i < n) winner[i] = kBakeNoWinner;
}

__global__ __launch_bounds__(kBakeBlock) void bake_cover_kernel(BakeSurfaceDev s, int32_t width, int32_t height, uint32_t* __restrict__ winner)
{
    const uint32_t t = blockIdx.x * (uint32_t)kBakeBlock + threadIdx.x;
    if (t >= s.n_tris) return;
    const BakeTri2 q = bake_tri2(s, t, width, height);
    if (!bake_tri_drawn(q)) return;
    int32_t x0, y0, x1, y1;
    if (!bake_tri_box(q, width, height, x0, y0, x1, y1)) return;   // (inside the image: 0 <= x0, x1 < width, 0 <= y0, y1 < height)
    for (int32_t y = y0; y <= y1; y++)
        for (int32_t x = x0; x <= x1; x++) {
            float eb, ec;
            if (bake_cover(q, x, y, eb, ec)) atomicMin(&winner[(size_t)y * (size_t)width + (size_t)x], t);
        }
}

__global__ __launch_bounds__(kBakeBlock) void bake_write_kernel(BakeSurfaceDev s, int32_t width, int32_t height, const uint32_t* __restrict__ winner,
                                                                float4* __restrict__ position4, float4* __restrict__ normal4)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBakeBlock + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const uint32_t t = winner[i];
    if (t >= s.n_tris) return;   // (no winner)
    float4 p4, n4;
    bake_resolve(s, t, width, height, (int32_t)(i % (uint32_t)width), (int32_t)(i / (uint32_t)width), p4, n4);
    position4[i] = p4;
    normal4[i] = n4;
}

unsigned blocks_for(size_t n) { return (unsigned)((n + (size_t)kBakeBlock - 1) / (size_t)kBakeBlock); }

}  // namespace

void launch_bake_raster(hipStream_t stream, const BakeSurfaceDev& surf, int32_t width, int32_t height, uint32_t* winner, float4* position4,
                        float4* normal4)
{
    if (width <= 0 || height <= 0 || surf.n_tris == 0) return;
    const size_t n = (size_t)width * (size_t)height;   // (<= 2^26: check_bake_size)
    hipLaunchKernelGGL(bake_clear, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, winner, (uint32_t)n);
    hipLaunchKernelGGL(bake_cover_kernel, dim3(blocks_for(surf.n_tris)), dim3(kBakeBlock), 0, stream, surf, width, height, winner);
    hipLaunchKernelGGL(bake_write_kernel, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, surf, width, height, winner, position4, normal4);
}

void bake_raster_host(const BakeSurfaceDev& surf, int32_t width, int32_t height, float4* position4, float4* normal4)
{
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++)
            for (uint32_t t = 0; t < surf.n_tris; t++) {   // (the first triangle that covers the centre is the lowest index)
                const BakeTri2 q = bake_tri2(surf, t, width, height);
                float eb, ec;
                int32_t x0, y0, x1, y1;
                if (!bake_tri_drawn(q) || !bake_tri_box(q, width, height, x0, y0, x1, y1)) continue;
                if (x < x0 || x > x1 || y < y0 || y > y1 || !bake_cover(q, x, y, eb, ec)) continue;
                const size_t i = (size_t)y * (size_t)width + (size_t)x;
                bake_resolve(surf, t, width, height, x, y, position4[i], normal4[i]);
                break;
            }
}

}  // namespace jpt
