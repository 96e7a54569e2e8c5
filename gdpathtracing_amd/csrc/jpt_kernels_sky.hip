// jpt_kernels_sky.hip -- jpt_set_sky: the environment map of a procedural sky written in place (the arithmetic: jpt_sky.h, which the
// host forms of jpt_debug_sky run as well).
//
// One streaming ALU kernel: one thread per texel, a block takes 256 consecutive texels of one row (blockIdx.y is the row), so a wave's
// 64 stores are 1 KiB of one row.  The parameter block is a kernel argument passed by value: wave-uniform, read with scalar loads from
// the kernel-argument segment and held in SGPRs.  The row, the sub-row loop and the sun loop are uniform too; only the column varies
// across a wave, and the only divergence is between texels inside and outside a sun's disk or halo.  Per sub-row the gradient is
// evaluated once (sky_texel); per subsample one sincos_, and per sun one cross product, square root and atan2_ -- pow01_ only inside a
// halo.  Nothing is loaded from global memory; one 16-byte store per texel.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "jpt_kernels.h"
#include "jpt_sky.h"

namespace jpt {

namespace {

__global__ __launch_bounds__(kSkyBlock) void sky_kernel(const SkyDev P, int32_t w, int32_t h, int32_t n, float4* __restrict__ out)
{
    const int32_t i = (int32_t)(blockIdx.x * (uint32_t)kSkyBlock + threadIdx.x), j = (int32_t)blockIdx.y;
    if (i >= w) return;
    const f3 c = sky_texel(P, w, h, n, i, j);
    out[(size_t)j * (size_t)w + (size_t)i] = make_float4(c.x, c.y, c.z, 0.0f);
}

}  // namespace

void launch_sky(hipStream_t stream, const SkyDev& P, int32_t w, int32_t h, int32_t n, float4* out)
{
    if (w <= 0 || h <= 0) return;
    const dim3 grid((unsigned)((w + kSkyBlock - 1) / kSkyBlock), (unsigned)h);   // h <= 8192: within the grid's y limit
    hipLaunchKernelGGL(sky_kernel, grid, dim3(kSkyBlock), 0, stream, P, w, h, n, out);
}

}  // namespace jpt
