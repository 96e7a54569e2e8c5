// jpt_kernels_bake.hip -- lightmap baking's own kernels (jpt_bake.h has the arithmetic): the UV2 rasteriser of jpt_bake_add_surface,
// the probe of jpt_debug_bake_rays, their host forms (the same __host__ __device__ functions in plain loops) and the argument checks
// the context's calls and the debug entry points share.  The bake forms of the bounce-0 kernels are in jpt_kernels_wf2.hip
// (jpt_wf2_paths.h, JPT_BAKE), the audit kernel's branch in jpt_ref_frame.h.
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

__global__ __launch_bounds__(kBakeBlock) void bake_rays_probe(BakeDev bake, int32_t width, int32_t height, uint32_t frame, float* __restrict__ origins3,
                                                              float* __restrict__ dirs3, uint8_t* __restrict__ valid)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBakeBlock + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    const float4 n4 = bake.normal[i];
    const bool ok = bake_texel_valid(n4);
    Ray ray;
    ray.o = ray.d = ray.rD = mk3(0.0f, 0.0f, 0.0f);
    uint32_t sx, sy;
    if (ok) ray = bake_ray(bake.position[i], n4, (int)(i % (uint32_t)width), (int)(i / (uint32_t)width), frame, sx, sy);
    origins3[3 * (size_t)i] = ray.o.x;
    origins3[3 * (size_t)i + 1] = ray.o.y;
    origins3[3 * (size_t)i + 2] = ray.o.z;
    dirs3[3 * (size_t)i] = ray.d.x;
    dirs3[3 * (size_t)i + 1] = ray.d.y;
    dirs3[3 * (size_t)i + 2] = ray.d.z;
    valid[i] = ok ? 1 : 0;
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

void launch_bake_rays_probe(hipStream_t stream, const BakeDev& bake, int32_t width, int32_t height, uint32_t frame, float* origins3, float* dirs3,
                            uint8_t* valid)
{
    if (width <= 0 || height <= 0) return;
    const size_t n = (size_t)width * (size_t)height;
    hipLaunchKernelGGL(bake_rays_probe, dim3(blocks_for(n)), dim3(kBakeBlock), 0, stream, bake, width, height, frame, origins3, dirs3, valid);
}

void bake_rays_host(const float4* position4, const float4* normal4, int32_t width, int32_t height, uint32_t frame, float* origins3, float* dirs3,
                    uint8_t* valid)
{
    const size_t n = (size_t)width * (size_t)height;
    for (size_t i = 0; i < n; i++) {
        const bool ok = bake_texel_valid(normal4[i]);
        Ray ray;
        ray.o = ray.d = ray.rD = mk3(0.0f, 0.0f, 0.0f);
        uint32_t sx, sy;
        if (ok) ray = bake_ray(position4[i], normal4[i], (int)(i % (size_t)width), (int)(i / (size_t)width), frame, sx, sy);
        origins3[3 * i] = ray.o.x;
        origins3[3 * i + 1] = ray.o.y;
        origins3[3 * i + 2] = ray.o.z;
        dirs3[3 * i] = ray.d.x;
        dirs3[3 * i + 1] = ray.d.y;
        dirs3[3 * i + 2] = ray.d.z;
        valid[i] = ok ? 1 : 0;
    }
}

int check_bake_size(const char* call, int32_t width, int32_t height, std::string& why)
{
    if (width < 1 || height < 1) {
        why = std::string(call) + ": width and height must be >= 1";
        return JPT_E_INVALID;
    }
    if ((uint64_t)width * (uint64_t)height > kBakeMaxTexels) {
        why = std::string(call) + ": more than 2^26 texels";
        return JPT_E_LIMIT;
    }
    return JPT_OK;
}

int check_bake_texels(const char* call, const float* position4, const float* normal4, size_t n, std::string& why)
{
    for (size_t i = 0; i < n; i++) {
        const float* nn = normal4 + 4 * i;
        const float* pp = position4 + 4 * i;
        if (!(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2] > 0.0f)) continue;   // (an invalid texel: nothing of it is read)
        bool finite = true;
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(nn[k]) && std::isfinite(pp[k]);
        if (!finite) {
            why = std::string(call) + ": valid texel " + std::to_string(i) + " has a non-finite position or normal component";
            return JPT_E_INVALID;
        }
    }
    return JPT_OK;
}

int check_bake_surface(const char* call, const float* vertices, const float* normals, const int32_t* indices, int32_t n_vertices, int32_t n_indices,
                       const float* uv2, const float* transform12, std::string& why)
{
    if (!vertices || !normals || !indices || !uv2 || !transform12) {
        why = std::string(call) + ": null argument (vertices, normals, indices, uv2 and transform12 are read)";
        return JPT_E_INVALID;
    }
    if (n_vertices < 0 || n_indices < 0 || n_indices % 3 != 0) {
        why = std::string(call) + ": n_vertices must be >= 0 and n_indices a multiple of 3";
        return JPT_E_INVALID;
    }
    if ((uint32_t)(n_indices / 3) > kBakeMaxTriangles) {
        why = std::string(call) + ": more than 2^24 triangles in one call";
        return JPT_E_LIMIT;
    }
    for (int32_t k = 0; k < n_indices; k++)
        if (indices[k] < 0 || indices[k] >= n_vertices) {
            why = std::string(call) + ": index " + std::to_string(k) + " is out of range";
            return JPT_E_INVALID;
        }
    return JPT_OK;
}

}  // namespace jpt
