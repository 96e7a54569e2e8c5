// jpt_kernels_lightmap.hip -- jpt_bake_finish: the guides of a bake's texel images, the chart-aware a-trous filter over the running
// mean and the dilation of the finished map.  No reference counterpart.  The arithmetic is pinned in jpt_lightmap.h / DESIGN.md
// section 2; nothing here writes a buffer a render reads, and nothing depends on the order threads run in (no atomics: every kernel
// reads images an earlier launch finished and writes its own texel of another).
#include "../../include/jpt.h"
#include "jpt_atrous_pass.h"
#include "jpt_lightmap.h"
#include "jpt_kernels.h"

namespace jpt {

namespace {

constexpr int kTexelBlock = 256;

// ---- prepare: one thread per texel -------------------------------------------------------------------------------------------------------
// colour0 may be null (a filter pass follows, and forms the mean while it stages)
__global__ __launch_bounds__(kTexelBlock) void lightmap_prepare_kernel(const float4* __restrict__ position4, const float4* __restrict__ normal4,
                                                                      const float4* __restrict__ sums, float frame_count, int32_t width,
                                                                      int32_t height, float4* __restrict__ xg, float4* __restrict__ ng,
                                                                      float4* __restrict__ colour0)
{
    const size_t i = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (i >= (size_t)width * (size_t)height) return;
    const int32_t y = (int32_t)(i / (size_t)width), x = (int32_t)(i - (size_t)y * (size_t)width);
    float4 gx, gn;
    lightmap_guides(position4, normal4, width, height, x, y, gx, gn);
    xg[i] = gx;
    ng[i] = gn;
    if (colour0) colour0[i] = lightmap_colour0(sums[i], frame_count, gx);
}

// ---- dilate: one thread per texel ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTexelBlock) void lightmap_dilate_kernel(const float4* __restrict__ in, float4* __restrict__ out, int32_t width, int32_t height)
{
    const size_t i = (size_t)blockIdx.x * kTexelBlock + threadIdx.x;
    if (i >= (size_t)width * (size_t)height) return;
    const int32_t y = (int32_t)(i / (size_t)width), x = (int32_t)(i - (size_t)y * (size_t)width);
    out[i] = lightmap_dilate(in, width, height, x, y);
}

// ---- filter ---------------------------------------------------------------------------------------------------------------------------------
struct LightmapArgs {
    const float4* __restrict__ in;   // FIRST: the accumulation (sums); else i_k
    const float4* __restrict__ x;    // xg
    const float4* __restrict__ n;    // ng
    float4* __restrict__ out;        // i_k+1
    int32_t width, height;
    float frame_count;               // FIRST: what the sums are divided by
    LightmapTaps taps;
};

// what a pass reads and writes (atrous_pass' Filter): the first one forms the mean of a valid texel; a texel outside the image is
// staged as invalid
template <bool FIRST>
struct LightmapFilter : LightmapArgs {
    static __device__ __forceinline__ float4 outside_x() { return lightmap_invalid_x(); }
    __device__ __forceinline__ float4 colour(size_t g, const float4& xg) const
    {
        const float4 v = in[g];
        if (!FIRST) return v;
        return lightmap_colour0(v, frame_count, xg);
    }
    __device__ __forceinline__ void write(size_t idx, const float4& r) const { out[idx] = r; }
};

// One pass, one lane per texel (jpt_atrous_pass.h): tiled for HALO = 2 * step > 0, gathered for HALO = 0 (steps >= 4)
template <int HALO, bool FIRST>
__global__ __launch_bounds__(kAtrousBlock) void lightmap_filter_kernel(LightmapFilter<FIRST> f)
{
    atrous_pass<HALO>(f, f.width, f.height, f.taps.ps.step);
}

}  // namespace

float4* launch_lightmap_finish(hipStream_t stream, const LightmapParams& prm, int width, int height, const float4* sums, float frame_count,
                               const float4* position4, const float4* normal4, float4* xg, float4* ng, float4* ping, float4* pong)
{
    if (width <= 0 || height <= 0) return ping;
    const size_t n = (size_t)width * (size_t)height;   // (<= 2^26: check_bake_size)
    const unsigned texel_blocks = (unsigned)((n + kTexelBlock - 1) / kTexelBlock);
    hipLaunchKernelGGL(lightmap_prepare_kernel, dim3(texel_blocks), dim3(kTexelBlock), 0, stream, position4, normal4, sums, frame_count, (int32_t)width,
                       (int32_t)height, xg, ng, prm.passes == 0 ? ping : (float4*)nullptr);
    LightmapArgs a = {};
    a.x = xg;
    a.n = ng;
    a.width = width;
    a.height = height;
    a.frame_count = frame_count;
    a.taps.ps.npow = prm.normal_power_log2;
    a.taps.ps.sd2 = prm.sigma_distance * prm.sigma_distance;
    a.taps.ps.sp2 = prm.sigma_plane * prm.sigma_plane;
    float sc = prm.sigma_color;
    // (pass 0 writes `ping`; with passes == 0 the prepare kernel wrote i_0 there: the dilation starts from what was written last)
    float4* cur = atrous_launch_passes(0, prm.passes, prm.passes, true, width, height, sums, ping, pong,
                                       [&](auto halo, int k, const float4* src, float4* dst, bool, dim3 grid, dim3 block) {
                                           constexpr int HALO = decltype(halo)::value;
                                           a.in = src;
                                           a.out = dst;
                                           a.taps.ps.step = 1 << k;
                                           a.taps.ps.sc2 = sc * sc;
                                           sc = sc * 0.5f;
                                           hipLaunchKernelGGL((lightmap_filter_kernel<HALO, HALO == 2>), grid, block, 0, stream, LightmapFilter<HALO == 2>{a});
                                       });
    if (!cur) cur = ping;
    float4* nxt = cur == ping ? pong : ping;
    for (int k = 0; k < prm.dilate; k++) {
        hipLaunchKernelGGL(lightmap_dilate_kernel, dim3(texel_blocks), dim3(kTexelBlock), 0, stream, (const float4*)cur, nxt, (int32_t)width, (int32_t)height);
        float4* t = cur;
        cur = nxt;
        nxt = t;
    }
    return cur;
}

}  // namespace jpt
