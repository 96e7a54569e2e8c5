// jpt_atrous_pass.h -- one pass of an a-trous filter over a 32 x 8-pixel tile, written once for jpt_denoise's three routes
// (jpt_kernels_denoise.hip, jpt_kernels_denoise_var.hip, jpt_kernels_denoise_history.hip) and jpt_bake_finish's filter
// (jpt_kernels_lightmap.hip): the bounds handling, the pinned tap order (dy outer, dx inner; taps outside the image skipped), the
// halo indexing and the "last pass writes `ping`" rule, on the device and on the host.  The arithmetic is not here: a filter brings
// it as its Taps (AtrousTaps of jpt_denoise.h, AtrousVarTaps of jpt_denoise_var.h, LightmapTaps of jpt_lightmap.h), and the kernels
// are thin wrappers that add what a pass reads and writes.  No reference counterpart.
#pragma once

#include "jpt_denoise_var.h"
#include "jpt_shade.h"

#include <type_traits>

namespace jpt {

// the prefilter of the centre (x, y), fed v(dx, dy) of its 3 x 3 neighbours inside the image in the pinned order; a filter without
// one (AtrousNoPrefilter) reads nothing
template <class Taps, class V>
__host__ __device__ __forceinline__ typename Taps::Prefilter atrous_prefilter(int x, int y, int width, int height, V v)
{
    typename Taps::Prefilter pre;
    if constexpr (!std::is_same<typename Taps::Prefilter, AtrousNoPrefilter>::value) {
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                pre.tap(v(dx, dy), dx, dy);
            }
        }
    }
    return pre;
}

// ---- the host form ------------------------------------------------------------------------------------------------------------
// Passes 0 .. passes - 1 of any of the filters, from the image `a` (`b`: as large) with the guides xg, ng; taps_of(k) gives the Taps
// of pass k (called once per pass, in order).  Returns the one of a, b that holds the result.  Tap coordinates are int64_t: the
// spacing of pass 5 times 2 leaves a 65536-wide image.
template <class TapsOf>
float4* atrous_passes_host(int passes, int32_t width, int32_t height, const float4* xg, const float4* ng, float4* a, float4* b, TapsOf taps_of)
{
    using Taps = decltype(taps_of(0));
    for (int k = 0; k < passes; k++) {
        const Taps taps = taps_of(k);
        const int s = 1 << k;
        for (int32_t y = 0; y < height; y++)
            for (int32_t x = 0; x < width; x++) {
                const size_t ip = (size_t)y * width + x;
                if (taps.skip(xg[ip])) {
                    b[ip] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    continue;
                }
                const typename Taps::Pixel p{a[ip], xg[ip], ng[ip]};
                const auto c = taps.centre(s, atrous_prefilter<Taps>(x, y, width, height, [&](int dx, int dy) { return a[(size_t)(y + dy) * width + (size_t)(x + dx)].w; }));
                typename Taps::Sum sum;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int64_t qx = (int64_t)x + (int64_t)s * dx, qy = (int64_t)y + (int64_t)s * dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t iq = (size_t)qy * width + (size_t)qx;
                        const typename Taps::Pixel q{a[iq], xg[iq], ng[iq]};
                        taps.tap(sum, p, q, dx, dy, c);
                    }
                b[ip] = sum.result(p);
            }
        float4* t = a;
        a = b;
        b = t;
    }
    return a;
}

// ---- the launches -------------------------------------------------------------------------------------------------------------
constexpr int kAtrousTileW = 32, kAtrousTileH = 8, kAtrousBlock = kAtrousTileW * kAtrousTileH;

// Passes first_pass .. end_pass - 1 of a filter of `passes` passes, ping-pong between `ping` and `pong`; pass first_pass reads `src`.
// Pass k is launch(halo, k, src, dst, last, grid, block): halo is std::integral_constant 2, 4 (the tiled forms of steps 1 and 2) or
// 0 (the gathered form of steps >= 4), last says k is the filter's last pass.  The last pass writes `ping`; with ping_first pass 0
// does instead (whichever the last one writes then).  Returns what the last launched pass wrote (none: null).
template <class Launch>
float4* atrous_launch_passes(int first_pass, int end_pass, int passes, bool ping_first, int width, int height, const float4* src, float4* ping,
                             float4* pong, Launch launch)
{
    const dim3 grid((unsigned)((width + kAtrousTileW - 1) / kAtrousTileW), (unsigned)((height + kAtrousTileH - 1) / kAtrousTileH)), block(kAtrousBlock);
    float4* dst = nullptr;
    for (int k = first_pass; k < end_pass; k++) {
        dst = ((ping_first ? k : passes - 1 - k) & 1) ? pong : ping;
        const bool last = k + 1 == passes;
        if (k == 0) launch(std::integral_constant<int, 2>(), k, src, dst, last, grid, block);
        else if (k == 1) launch(std::integral_constant<int, 4>(), k, src, dst, last, grid, block);
        else launch(std::integral_constant<int, 0>(), k, src, dst, last, grid, block);
        src = dst;
    }
    return dst;
}

// ---- the device form ----------------------------------------------------------------------------------------------------------
// A Filter is a kernel's view of its arguments: `taps` (its Taps), the guides `x` and `n`, `in` (what the gathered prefilter reads
// the .w of), colour(g, xg): what the pass reads at pixel g, whose guide xg the caller has just loaded; outside_x(): the x guide of a
// staged pixel outside the image (its colour and n are zeros; no tap reads it); write(idx, r): the store.  A staging Source is the
// x, n, colour and outside_x of that.
template <int HALO>
struct AtrousTiles {
    static constexpr int TW = kAtrousTileW + 2 * HALO, TH = kAtrousTileH + 2 * HALO;
    const float4 *c, *x, *n;
};

// The block stages its tile at (x0, y0) and a HALO-pixel border of colour, x and n in LDS with 16-byte accesses -- a first pass forms
// its colour while it stages: once per staged pixel, not once per tap -- and waits for it.  The tiles are allocated in every kernel
// that reaches an instantiation: each <HALO, Source> belongs to one kernel.
template <int HALO, class Source>
__device__ __forceinline__ AtrousTiles<HALO> atrous_stage(const Source& f, int x0, int y0, int width, int height)
{
    constexpr int TW = AtrousTiles<HALO>::TW, TH = AtrousTiles<HALO>::TH;
    __shared__ float4 tc[TW * TH], tx[TW * TH], tn[TW * TH];
    for (int i = (int)threadIdx.x; i < TW * TH; i += kAtrousBlock) {
        const int gx = x0 - HALO + i % TW, gy = y0 - HALO + i / TW;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), px = Source::outside_x(), nn = c;
        if (gx >= 0 && gy >= 0 && gx < width && gy < height) {
            const size_t g = (size_t)gy * (size_t)width + (size_t)gx;
            px = f.x[g];
            nn = f.n[g];
            c = f.colour(g, px);
        }
        tx[i] = px;   // (in the order the loads were issued: no store waits for a later load)
        tn[i] = nn;
        tc[i] = c;
    }
    __syncthreads();
    return {tc, tx, tn};
}

// One pass, one lane per pixel, 32 x 8 pixels per block of kAtrousBlock lanes.  HALO = 2 * step > 0 (steps 1 and 2): the 25 taps and
// the prefilter (spacing 1: HALO >= 2 covers it) are read from the staged tiles -- a wave's two rows are 32 consecutive float4 each,
// which ds_read_b128 serves without a bank conflict.  HALO = 0 (steps >= 4): the taps of a wave's row are themselves contiguous rows
// of 32 pixels, so 16-byte gathers straight from memory coalesce; a tile's border would be larger than the tile.
template <int HALO, class Filter>
__device__ __forceinline__ void atrous_pass(const Filter& f, int width, int height, int step)
{
    using Taps = typename std::decay<decltype(f.taps)>::type;
    using Pixel = typename Taps::Pixel;
    const int lx = (int)threadIdx.x & (kAtrousTileW - 1), ly = (int)threadIdx.x / kAtrousTileW;
    const int x0 = (int)blockIdx.x * kAtrousTileW, y0 = (int)blockIdx.y * kAtrousTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < width && y < height;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    if (HALO > 0) {
        constexpr int TW = AtrousTiles<HALO>::TW, s = HALO / 2;
        const AtrousTiles<HALO> t = atrous_stage<HALO>(f, x0, y0, width, height);
        if (!inside) return;
        const int ci = (ly + HALO) * TW + (lx + HALO);
        const Pixel p{t.c[ci], t.x[ci], t.n[ci]};
        if (f.taps.skip(p.x)) {
            f.write(idx, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            return;
        }
        const auto c = f.taps.centre(s, atrous_prefilter<Taps>(x, y, width, height, [&](int dx, int dy) { return t.c[ci + dy * TW + dx].w; }));
        typename Taps::Sum sum;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx, qy = y + s * dy;
                if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                const int qi = ci + s * dy * TW + s * dx;
                const Pixel q{t.c[qi], t.x[qi], t.n[qi]};
                f.taps.tap(sum, p, q, dx, dy, c);
            }
        }
        f.write(idx, sum.result(p));
    } else {
        if (!inside) return;
        const int s = step;
        const float4 px = f.x[idx];
        if (f.taps.skip(px)) {
            f.write(idx, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            return;
        }
        const Pixel p{f.colour(idx, px), px, f.n[idx]};
        const auto c = f.taps.centre(s, atrous_prefilter<Taps>(x, y, width, height, [&](int dx, int dy) { return f.in[(size_t)((int64_t)idx + (int64_t)dy * width + dx)].w; }));
        typename Taps::Sum sum;
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + s * dy;
            if (qy < 0 || qy >= height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx;
                if (qx < 0 || qx >= width) continue;
                const size_t g = (size_t)qy * (size_t)width + (size_t)qx;
                const float4 qxg = f.x[g];
                const Pixel q{f.colour(g, qxg), qxg, f.n[g]};
                f.taps.tap(sum, p, q, dx, dy, c);
            }
        }
        f.write(idx, sum.result(p));
    }
}

// what the last pass of jpt_denoise writes of its result r, on every route: the remodulated image (r, g, b, 1), r.w into var_out (a
// variance-guided route) and, unless ldr is null, unorm8(ACES(denoised))
template <bool VAR>
__device__ __forceinline__ void atrous_write_last(const float4& r, size_t idx, const float4* albedo, float4* out, float* var_out, uint32_t* ldr)
{
    const float4 am = atrous_amod(albedo[idx]);
    const f3 den = mk3(r.x * am.x, r.y * am.y, r.z * am.z);
    out[idx] = make_float4(den.x, den.y, den.z, 1.0f);
    if (VAR) var_out[idx] = r.w;
    if (ldr) {
        const f3 col = aces_film(den);
        ldr[idx] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xFF000000u;
    }
}

// The variance-guided passes' arguments and Filter, for the two files that launch them: atrous_var_kernel (jpt_kernels_denoise_var.hip)
// and atrous_var_pre_kernel, pass 0 over the pre-formed (i, v) image of the history route (jpt_kernels_denoise_history.hip).
struct AtrousVarArgs {
    const float4* __restrict__ in;    // FIRST: the accumulation (sums); else (i_k, v_k)
    const float4* __restrict__ m2;    // FIRST: the plane of jpt_set_variance
    const float4* __restrict__ x;     // position_t
    const float4* __restrict__ n;     // normal
    const float4* __restrict__ albedo;   // read by the first pass (demodulation) and the last (remodulation)
    float4* __restrict__ out;         // (i_k+1, v_k+1); LAST: the denoised image (r, g, b, 1)
    uint32_t* __restrict__ ldr;       // LAST: unorm8(ACES(denoised)) (may be null)
    float* __restrict__ var_out;      // LAST: v of the last pass
    int32_t width, height, step;
    float nf, q;                      // FIRST: (float)frame_count and nf * (nf - 1)
    AtrousVarTaps taps;
};

// (frame_count and m2: read by pass 0 over the sums alone)
inline AtrousVarArgs atrous_var_args(const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, const float4* m2, uint32_t frame_count,
                                     const float4* position_t, const float4* normal, const float4* albedo, uint32_t* ldr, float* var_out)
{
    AtrousVarArgs a = {};
    a.m2 = m2;
    a.x = position_t;
    a.n = normal;
    a.albedo = albedo;
    a.ldr = ldr;
    a.var_out = var_out;
    a.width = width;
    a.height = height;
    a.nf = (float)frame_count;
    a.q = a.nf * (a.nf - 1.0f);
    a.taps = AtrousVarTaps{prm.normal_power_log2, prm.sigma_plane, vprm.sigma_variance * vprm.sigma_variance, vprm.variance_floor};
    return a;
}

template <bool FIRST, bool LAST>
struct AtrousVarFilter : AtrousVarArgs {
    static __device__ __forceinline__ float4 outside_x() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __device__ __forceinline__ float4 colour(size_t g, const float4&) const
    {
        const float4 v = in[g];
        if (!FIRST) return v;
        return atrous_var_first(v, m2[g], nf, q, albedo[g]);
    }
    __device__ __forceinline__ void write(size_t idx, const float4& r) const
    {
        if (LAST) atrous_write_last<true>(r, idx, albedo, out, var_out, ldr);
        else out[idx] = r;
    }
};

}  // namespace jpt
