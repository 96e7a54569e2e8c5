// jpt_kernels_lightmap.hip -- jpt_bake_finish: the guides of a bake's texel images, the chart-aware a-trous filter over the running
// mean and the dilation of the finished map.  No reference counterpart.  The arithmetic is pinned in jpt_lightmap.h / DESIGN.md
// section 2; nothing here writes a buffer a render reads, and nothing depends on the order threads run in (no atomics: every kernel
// reads images an earlier launch finished and writes its own texel of another).
#include "../../include/jpt.h"
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
    const float4* __restrict__ xg;
    const float4* __restrict__ ng;
    float4* __restrict__ out;        // i_k+1
    int32_t width, height;
    float frame_count;               // FIRST: what the sums are divided by
    LightmapPass ps;
};

constexpr int kTileW = 32, kTileH = 8, kFilterBlock = kTileW * kTileH;

template <bool FIRST>
__device__ __forceinline__ float4 lightmap_colour(const LightmapArgs& a, size_t idx, const float4& xg)
{
    const float4 v = a.in[idx];
    if (!FIRST) return v;
    return lightmap_colour0(v, a.frame_count, xg);
}

// One pass, one lane per texel, 32 x 8 texels per block: atrous_kernel's arrangement (jpt_kernels_denoise.hip).  HALO = 2 * step > 0
// (steps 1 and 2): the block stages its tile and a HALO-texel border of colour, xg and ng in LDS with 16-byte accesses (the first
// pass forms the mean while it stages: once per staged texel, not once per tap) and reads its 25 taps from there -- a wave's two
// rows are 32 consecutive float4 each, which ds_read_b128 serves without a bank conflict.  HALO = 0 (steps >= 4): the taps of a
// wave's row are themselves contiguous rows of 32 texels, so 16-byte gathers straight from memory coalesce; a tile's border would be
// larger than the tile.  A texel outside the image is staged as invalid; no tap reads it (taps outside the image are skipped).
template <int HALO, bool FIRST>
__global__ __launch_bounds__(kFilterBlock) void lightmap_filter_kernel(LightmapArgs a)
{
    const int lx = (int)threadIdx.x & (kTileW - 1), ly = (int)threadIdx.x / kTileW;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < a.width && y < a.height;
    const size_t idx = (size_t)y * (size_t)a.width + (size_t)x;
    if (HALO > 0) {
        constexpr int TW = kTileW + 2 * HALO, TH = kTileH + 2 * HALO, s = HALO / 2;
        __shared__ float4 tc[TW * TH], tx[TW * TH], tn[TW * TH];
        for (int i = (int)threadIdx.x; i < TW * TH; i += kFilterBlock) {
            const int gx = x0 - HALO + i % TW, gy = y0 - HALO + i / TW;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), px = lightmap_invalid_x(), nn = c;
            if (gx >= 0 && gy >= 0 && gx < a.width && gy < a.height) {
                const size_t g = (size_t)gy * (size_t)a.width + (size_t)gx;
                px = a.xg[g];
                nn = a.ng[g];
                c = lightmap_colour<FIRST>(a, g, px);
            }
            tc[i] = c;
            tx[i] = px;
            tn[i] = nn;
        }
        __syncthreads();
        if (!inside) return;
        const int ci = (ly + HALO) * TW + (lx + HALO);
        const LightmapTexel p{tc[ci], tx[ci], tn[ci]};
        if (p.x.w < 0.0f) {
            a.out[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return;
        }
        LightmapPass ps = a.ps;
        ps.step = s;
        LightmapSum sum;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx, qy = y + s * dy;
                if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                const int qi = ci + s * dy * TW + s * dx;
                const LightmapTexel q{tc[qi], tx[qi], tn[qi]};
                sum.tap(p, q, dx, dy, ps);
            }
        }
        a.out[idx] = sum.result(p);
    } else {
        if (!inside) return;
        const int s = a.ps.step;
        const float4 pxg = a.xg[idx];
        if (pxg.w < 0.0f) {
            a.out[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return;
        }
        const LightmapTexel p{lightmap_colour<FIRST>(a, idx, pxg), pxg, a.ng[idx]};
        LightmapSum sum;
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + s * dy;
            if (qy < 0 || qy >= a.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx;
                if (qx < 0 || qx >= a.width) continue;
                const size_t g = (size_t)qy * (size_t)a.width + (size_t)qx;
                const float4 qxg = a.xg[g];
                const LightmapTexel q{lightmap_colour<FIRST>(a, g, qxg), qxg, a.ng[g]};
                sum.tap(p, q, dx, dy, a.ps);
            }
        }
        a.out[idx] = sum.result(p);
    }
}

template <int HALO, bool FIRST>
void launch_filter_pass(hipStream_t stream, const LightmapArgs& a)
{
    const dim3 grid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH)), block(kFilterBlock);
    hipLaunchKernelGGL((lightmap_filter_kernel<HALO, FIRST>), grid, block, 0, stream, a);
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
    LightmapArgs a;
    a.xg = xg;
    a.ng = ng;
    a.width = width;
    a.height = height;
    a.frame_count = frame_count;
    a.ps.npow = prm.normal_power_log2;
    a.ps.sd2 = prm.sigma_distance * prm.sigma_distance;
    a.ps.sp2 = prm.sigma_plane * prm.sigma_plane;
    float sc = prm.sigma_color;
    const float4* src = sums;
    float4 *dst = ping, *other = pong;
    for (int k = 0; k < prm.passes; k++, sc = sc * 0.5f) {
        a.in = src;
        a.out = dst;
        a.ps.step = 1 << k;
        a.ps.sc2 = sc * sc;
        if (k == 0) launch_filter_pass<2, true>(stream, a);
        else if (k == 1) launch_filter_pass<4, false>(stream, a);
        else launch_filter_pass<0, false>(stream, a);
        src = dst;
        float4* t = dst;
        dst = other;
        other = t;
    }
    // (with passes == 0 the prepare kernel wrote i_0 into ping: the dilation starts from there)
    float4* cur = prm.passes == 0 ? ping : const_cast<float4*>(src);
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
