// jpt_denoise_history.h -- the arithmetic of jpt_denoise with jpt_set_denoise_history on ("the history stage"): the
// temporal third of SVGF (Schied et al. 2017).  Each call integrates the mean of its frames into a per-pixel history that is reprojected
// from the previous call's view and validated against the previous call's position and normal guides, and estimates the variance of the
// integrated value -- from the history where it is long enough, from the 5 x 5 neighbourhood where it is not.  No reference counterpart.
//
// A history texel is three float4: a = (m.rgb, N), b = (n.xyz, S), x = position_t -- the integrated demodulated colour and the history
// length, the normal and the sum of squared deviations (West's update, jpt_variance.h), the first hit.  Per pixel p with this call's
// guides X = position_t, n = normal, albedo, and nf = (float)frame_count:
//   1  c = atrous_demodulate(sum, nf, albedo).  t < 0 or c not finite: the texel is (c, 0), (n, 0), X and the filter gets (c, +0).
//   2  identical view: the one tap is the previous texel of p itself, taken as it is (no multiplication) when its N > 0, its m and S
//      are finite and atrous_geom_weight(p, tap) > 0.  Otherwise clip = vp_prev * (X, 1), each row left to right; clip.w > 0 or no history;
//      nx = clip.x / clip.w, ny = clip.y / clip.w, u = (nx + 1) / 2 * W, v = (1 - ny) / 2 * H, pu = u - 0.5, pv = v - 0.5; -1 < pu < W
//      and -1 < pv < H or no history; x0 = floor(pu), fx = pu - x0 (y likewise); taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
//      (x0 + 1, y0 + 1) in this order with bilinear weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; a tap outside the image
//      is skipped.
//   3  wt = bilinear * atrous_geom_weight(p, tap, normal_power_log2, history.sigma_plane); a tap with N = 0, an m or an S that is not
//      finite (one sample with |d|^2 past FLT_MAX makes S = inf, which (1 - al) never shrinks: such a texel is not passed on, and the
//      pixels that would tap it start over) or a NaN weight has weight 0, and a tap of weight 0 is not multiplied.  sum wt > 0:
//      m_h, S_h, N_h = (sum wt * value) / sum wt.
//   4  N = max(min(N_h + nf, max_history), nf), al = nf / N, d = c - m_h, m = m_h + al * d,
//      S = (1 - al) * (S_h + al * (d.r * d.r + d.g * d.g + d.b * d.b)).  Without history m = c, S = 0, N = nf (al = 1).
//   5  with history and N_h >= min_history: v_0 = (S * al) / (1 - al).  Else over the 5 x 5 window of this call's c (dy outer, dx inner;
//      inside the image, colour finite, atrous_geom_weight against the centre > 0; the centre always): the mean per channel, then
//      S_s = sum |c_q - mean|^2 / count, v_0 = S_s * al; fewer than two taps: +0.  A v_0 that is not finite or not > 0 is +0.
//   6  the filter gets (m, v_0); the new texel is (m, N), (n, S), X.
// Each + - * / is one binary32 operation in the order written (-ffp-contract=off): history_kernel (jpt_kernels_denoise_history.hip) and
// the host form of jpt_debug_denoise_history run these functions, and tests/np_denoise_history.py restates them bit for bit.
#pragma once

#include "jpt_denoise.h"

#include <cmath>
#include <string>

namespace jpt {

struct HistoryParams {   // jpt_denoise_history_params
    int32_t enable = 0;
    int32_t max_history = 32;
    int32_t min_history = 4;
    float sigma_plane = 0.05f;
};

// the checks of jpt_set_denoise_history, also run by jpt_debug_denoise_history (`reserved`: the struct's last four fields)
inline int check_denoise_history_params(const HistoryParams& p, const int32_t* reserved, std::string& why)
{
    if (p.enable != 0 && p.enable != 1) why = "jpt_denoise_history_params: enable must be 0 or 1";
    else if (p.max_history < 1 || p.max_history > 65536) why = "jpt_denoise_history_params: max_history must be in [1, 65536]";
    else if (p.min_history < 1 || p.min_history > p.max_history) why = "jpt_denoise_history_params: min_history must be in [1, max_history]";
    else if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) why = "jpt_denoise_history_params: sigma_plane must be finite and > 0";
    else if (reserved[0] != 0 || reserved[1] != 0 || reserved[2] != 0 || reserved[3] != 0) why = "jpt_denoise_history_params: reserved must be 0";
    else return 0;    // JPT_OK
    return -1;        // JPT_E_INVALID
}

struct HistoryView {   // RefCamera::vp of the previous call, column-major
    float vp[16];
};

struct HistoryTexel {
    float4 a, b, x;   // (m.rgb, N), (n.xyz, S), position_t
};

// what the stage knows of a pixel once its history is gathered and integrated
struct HistoryPixel {
    float4 m;        // (m.rgb, v_0): v_0 is final unless `spatial`
    float N, S, al;
    bool spatial;    // v_0 is the neighbourhood's: history_spatial
};

// step 2: the previous call's raster position of X, less half a pixel; false: no history
__host__ __device__ __forceinline__ bool history_project(const HistoryView& pv, const float4& X, int width, int height, float& pu, float& pvv)
{
    const float* m = pv.vp;
    const float cx = m[0] * X.x + m[4] * X.y + m[8] * X.z + m[12];
    const float cy = m[1] * X.x + m[5] * X.y + m[9] * X.z + m[13];
    const float cw = m[3] * X.x + m[7] * X.y + m[11] * X.z + m[15];
    if (!(cw > 0.0f)) return false;
    const float nx = cx / cw, ny = cy / cw;
    const float u = (nx + 1.0f) / 2.0f * (float)width, v = (1.0f - ny) / 2.0f * (float)height;
    pu = u - 0.5f;
    pvv = v - 0.5f;
    return pu > -1.0f && pu < (float)width && pvv > -1.0f && pvv < (float)height;
}

// step 3: the weighted sums over the taps, fed in the pinned order
struct HistoryGather {
    float r = 0.0f, g = 0.0f, b = 0.0f, s = 0.0f, n = 0.0f, w = 0.0f;
    __host__ __device__ __forceinline__ static bool usable(const HistoryTexel& q) { return q.a.w > 0.0f && atrous_finite3(q.a) && atrous_finite(q.b.w); }
    __host__ __device__ __forceinline__ void tap(const AtrousPixel& p, const HistoryTexel& q, float bilinear, int npow, float sigma_plane)
    {
        const AtrousPixel t{q.a, q.x, q.b};
        float wt = bilinear * atrous_geom_weight(p, t, npow, sigma_plane);
        if (!usable(q) || wt != wt) wt = 0.0f;
        const bool use = wt != 0.0f;
        r = r + (use ? q.a.x * wt : 0.0f);
        g = g + (use ? q.a.y * wt : 0.0f);
        b = b + (use ? q.a.z * wt : 0.0f);
        s = s + (use ? q.b.w * wt : 0.0f);
        n = n + (use ? q.a.w * wt : 0.0f);
        w = w + wt;
    }
};

// steps 4 and 5 (the history's variance): c the sample; `have`: (mh, Sh, Nh) is an accepted history
__host__ __device__ __forceinline__ HistoryPixel history_integrate(const float4& c, bool have, const float4& mh, float Sh, float Nh, float nf, float maxh,
                                                                   float minh)
{
    HistoryPixel o;
    if (!have) {
        o.m = make_float4(c.x, c.y, c.z, 0.0f);
        o.N = nf;
        o.S = 0.0f;
        o.al = nf / o.N;
        o.spatial = true;
        return o;
    }
    float t = Nh + nf;
    t = t < maxh ? t : maxh;
    o.N = t > nf ? t : nf;
    o.al = nf / o.N;
    const float dx = c.x - mh.x, dy = c.y - mh.y, dz = c.z - mh.z;
    o.m = make_float4(mh.x + o.al * dx, mh.y + o.al * dy, mh.z + o.al * dz, 0.0f);
    o.S = (1.0f - o.al) * (Sh + o.al * (dx * dx + dy * dy + dz * dz));
    o.spatial = !(Nh >= minh);
    if (!o.spatial) {
        const float v = (o.S * o.al) / (1.0f - o.al);
        o.m.w = (atrous_finite(v) && v > 0.0f) ? v : 0.0f;
    }
    return o;
}

// step 5, the neighbourhood's variance: whether tap q of the window counts, and the two running sums
__host__ __device__ __forceinline__ bool history_spatial_accept(const AtrousPixel& p, const AtrousPixel& q, int dx, int dy, int npow, float sigma_plane)
{
    if (dx == 0 && dy == 0) return true;
    return atrous_finite3(q.c) && atrous_geom_weight(p, q, npow, sigma_plane) > 0.0f;
}
struct HistorySpatial {
    float r = 0.0f, g = 0.0f, b = 0.0f, count = 0.0f, ss = 0.0f;
    __host__ __device__ __forceinline__ void mean_tap(const float4& c)
    {
        r = r + c.x;
        g = g + c.y;
        b = b + c.z;
        count = count + 1.0f;
    }
    __host__ __device__ __forceinline__ void mean_done()
    {
        r = r / count;
        g = g / count;
        b = b / count;
    }
    __host__ __device__ __forceinline__ void dist_tap(const float4& c)
    {
        const float dx = c.x - r, dy = c.y - g, dz = c.z - b;
        ss = ss + (dx * dx + dy * dy + dz * dz);
    }
    __host__ __device__ __forceinline__ float result(float al) const
    {
        if (count < 2.0f) return 0.0f;
        const float v = (ss / count) * al;
        return (atrous_finite(v) && v > 0.0f) ? v : 0.0f;
    }
};

// steps 1 to 4 of pixel (x, y) over the previous set (pa null: none): the pixel, and whether it is a live one (a hit with a finite sample)
template <typename Load>
__host__ __device__ __forceinline__ bool history_pixel(int x, int y, int width, int height, const float4& c, const float4& X, const float4& n, bool have_prev,
                                                       bool same_view, const HistoryView& view, const HistoryParams& hp, int npow, float nf, Load prev,
                                                       HistoryPixel& o)
{
    if (X.w < 0.0f || !atrous_finite3(c)) {
        o.m = make_float4(c.x, c.y, c.z, 0.0f);
        o.N = 0.0f;
        o.S = 0.0f;
        o.al = 1.0f;
        o.spatial = false;
        return false;
    }
    const AtrousPixel p{c, X, n};
    bool have = false;
    float4 mh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float Sh = 0.0f, Nh = 0.0f;
    if (have_prev && same_view) {
        const HistoryTexel q = prev(x, y);
        const AtrousPixel t{q.a, q.x, q.b};
        if (HistoryGather::usable(q) && atrous_geom_weight(p, t, npow, hp.sigma_plane) > 0.0f) {
            have = true;
            mh = q.a;
            Sh = q.b.w;
            Nh = q.a.w;
        }
    } else if (have_prev) {
        float pu, pv;
        if (history_project(view, X, width, height, pu, pv)) {
            const float flx = __builtin_floorf(pu), fly = __builtin_floorf(pv);
            const float fx = pu - flx, fy = pv - fly;
            const int x0 = (int)flx, y0 = (int)fly;
            HistoryGather sum;
            for (int k = 0; k < 4; k++) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                const float bw = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                sum.tap(p, prev(qx, qy), bw, npow, hp.sigma_plane);
            }
            if (sum.w > 0.0f) {
                have = true;
                mh = make_float4(sum.r / sum.w, sum.g / sum.w, sum.b / sum.w, 0.0f);
                Sh = sum.s / sum.w;
                Nh = sum.n / sum.w;
            }
        }
    }
    o = history_integrate(c, have, mh, Sh, Nh, nf, (float)hp.max_history, (float)hp.min_history);
    return true;
}

// the whole stage on the host (jpt_debug_denoise_history with JPT_DEVICE_HOST_ONLY): pa / pb / px the previous set or null; iv = (m, v_0),
// na / nb the new set's first two planes (the third is position_t itself)
inline void history_host(int32_t width, int32_t height, const HistoryParams& hp, int npow, const float4* sum4, uint32_t frame_count, const float4* position_t,
                         const float4* normal, const float4* albedo, const HistoryView& view, bool same_view, const float4* pa, const float4* pb,
                         const float4* px, float4* iv, float4* na, float4* nb)
{
    const size_t npx = (size_t)width * height;
    const float nf = (float)frame_count;
    float4* c = new float4[npx];
    for (size_t i = 0; i < npx; i++) c[i] = atrous_demodulate(sum4[i], nf, albedo[i]);
    auto prev = [&](int qx, int qy) {
        const size_t g = (size_t)qy * width + (size_t)qx;
        return HistoryTexel{pa[g], pb[g], px[g]};
    };
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const size_t ip = (size_t)y * width + x;
            HistoryPixel o;
            const bool live = history_pixel(x, y, width, height, c[ip], position_t[ip], normal[ip], pa != nullptr, same_view, view, hp, npow, nf, prev, o);
            if (live && o.spatial) {
                const AtrousPixel p{c[ip], position_t[ip], normal[ip]};
                HistorySpatial sp;
                for (int pass = 0; pass < 2; pass++) {
                    for (int dy = -2; dy <= 2; dy++)
                        for (int dx = -2; dx <= 2; dx++) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                            const size_t iq = (size_t)qy * width + (size_t)qx;
                            const AtrousPixel q{c[iq], position_t[iq], normal[iq]};
                            if (!history_spatial_accept(p, q, dx, dy, npow, hp.sigma_plane)) continue;
                            if (pass == 0) sp.mean_tap(q.c);
                            else sp.dist_tap(q.c);
                        }
                    if (pass == 0) sp.mean_done();
                }
                o.m.w = sp.result(o.al);
            }
            iv[ip] = o.m;
            na[ip] = make_float4(o.m.x, o.m.y, o.m.z, o.N);
            nb[ip] = make_float4(normal[ip].x, normal[ip].y, normal[ip].z, o.S);
        }
    delete[] c;
}

}  // namespace jpt
