// jpt_denoise_var.h -- the arithmetic of jpt_denoise with jpt_set_denoise_variance on ("the variance-guided
// a-trous filter"): the filter of jpt_denoise.h with its colour tolerance taken from the measured variance of the mean, as SVGF
// (Schied et al. 2017) takes it, instead of a fixed sigma_color.  No reference counterpart.
//
// With nf = (float)frame_count, q = nf * (nf - 1.0f), a = atrous_amod(albedo) and m2 the plane of jpt_set_variance (jpt_variance.h):
//     i_0   = atrous_demodulate(sum, nf, albedo)
//     v_0   = m2.x / q / (a.x * a.x) + m2.y / q / (a.y * a.y) + m2.z / q / (a.z * a.z)      (left to right; not finite or not > 0: +0)
// the variance of |i_0| as a sum over the channels, which is what |dc|^2, a sum over the channels, is measured against.  Pass k
// carries (i_k.rgb, v_k) in one float4.  Per pixel p of pass k, tap spacing 2^k:
//     gv    = sum of (h3(dy) * h3(dx)) * v_k(q) / sum of (h3(dy) * h3(dx)), h3 = (1 2 1) / 4, over the 3 x 3 neighbours q at spacing 1
//             (whatever k) inside the image, dy outer, dx inner
//     den   = (sigma_variance * sigma_variance) * gv + variance_floor                        (not halved per pass: v_k shrinks instead)
//     wc(q) = 1 / (1 + |c_q - c_p|^2 / den);   wt(q) = (h(dy) * h(dx)) * (e(q) * wc(q)), e = atrous_geom_weight; the centre's e * wc is 1
//     i_k+1 = sum wt * c_q / sum wt;           v_k+1 = sum (wt * wt) * v_q / (sum wt * sum wt)
// with jpt_denoise.h's tap order and rules: a tap outside the image is skipped, a tap whose colour is not finite or whose e * wc is a
// NaN has weight 0, a tap of weight 0 is not multiplied, a centre whose colour is not finite keeps its colour -- and its v.
// sigma_color is not read.  After the last pass the image is (i * a, 1) as jpt_denoise's, and v of the last pass is an output.
//
// Each + - * / is one binary32 operation in the order written (-ffp-contract=off): the device kernels (jpt_kernels_denoise_var.hip)
// and the host form of jpt_debug_atrous_variance run these functions through the one pass body of jpt_atrous_pass.h, and
// tests/np_denoise_var.py restates them bit for bit.
#pragma once

#include "jpt_denoise.h"

#include <cmath>
#include <string>

namespace jpt {

struct AtrousVarParams {   // jpt_denoise_variance_params
    int32_t enable = 0;
    float sigma_variance = 2.0f;
    float variance_floor = 1e-6f;
};
// (null: the defaults; `reserved`: the struct's last field) -- for jpt_set_denoise_variance and jpt_debug_atrous_variance alike
inline AtrousVarParams denoise_variance_params_of(const jpt_denoise_variance_params* p, int32_t& reserved)
{
    reserved = p ? p->reserved : 0;
    return p ? AtrousVarParams{p->enable, p->sigma_variance, p->variance_floor} : AtrousVarParams();
}

// the checks of jpt_set_denoise_variance, also run by jpt_debug_atrous_variance (`reserved`: the struct's last field)
inline int check_denoise_variance_params(const AtrousVarParams& p, int32_t reserved, std::string& why)
{
    if (p.enable != 0 && p.enable != 1) why = "jpt_denoise_variance_params: enable must be 0 or 1";
    else if (!std::isfinite(p.sigma_variance) || !(p.sigma_variance > 0.0f)) why = "jpt_denoise_variance_params: sigma_variance must be finite and > 0";
    else if (!std::isfinite(p.variance_floor) || !(p.variance_floor > 0.0f)) why = "jpt_denoise_variance_params: variance_floor must be finite and > 0";
    else if (reserved != 0) why = "jpt_denoise_variance_params: reserved must be 0";
    else return 0;    // JPT_OK
    return -1;        // JPT_E_INVALID
}

// the binomial kernel (1 2 1) / 4 of the variance prefilter
__host__ __device__ __forceinline__ float atrous_h3(int k) { return k == 1 ? 0.5f : 0.25f; }

// (i_0, v_0) of a pixel: q = nf * (nf - 1)
__host__ __device__ __forceinline__ float4 atrous_var_first(const float4& sum, const float4& m2, float nf, float q, const float4& albedo)
{
    const float4 a = atrous_amod(albedo);
    float4 c = atrous_demodulate(sum, nf, albedo);
    const float v = m2.x / q / (a.x * a.x) + m2.y / q / (a.y * a.y) + m2.z / q / (a.z * a.z);
    c.w = (atrous_finite(v) && v > 0.0f) ? v : 0.0f;
    return c;
}

// gv of one pixel, as a running sum the caller feeds the neighbours inside the image in the pinned order (dy = -1..1 outer, dx = -1..1 inner)
struct AtrousVarPrefilter {
    float num = 0.0f, w = 0.0f;
    __host__ __device__ __forceinline__ void tap(float v, int dx, int dy)
    {
        const float wt = atrous_h3(dy + 1) * atrous_h3(dx + 1);
        num = num + wt * v;
        w = w + wt;
    }
    // den of the pixel's colour weights: sv2 = sigma_variance * sigma_variance
    __host__ __device__ __forceinline__ float den(float sv2, float floor) const { return sv2 * (num / w) + floor; }
};

// One pixel of one pass: AtrousSum with the colour weight measured against den, and the variance carried along in c.w
struct AtrousVarSum {
    float r = 0.0f, g = 0.0f, b = 0.0f, w = 0.0f, vs = 0.0f;
    __host__ __device__ __forceinline__ void tap(const AtrousPixel& p, const AtrousPixel& q, int dx, int dy, int npow, float sigma_plane, float den)
    {
        float ew = 1.0f;
        if (!(dx == 0 && dy == 0)) {
            const float e = atrous_geom_weight(p, q, npow, sigma_plane);
            const float cx = q.c.x - p.c.x, cy = q.c.y - p.c.y, cz = q.c.z - p.c.z;
            const float wc = 1.0f / (1.0f + (cx * cx + cy * cy + cz * cz) / den);
            ew = e * wc;
        }
        float wt = (atrous_h(dy + 2) * atrous_h(dx + 2)) * ew;
        if (!atrous_finite3(q.c) || ew != ew) wt = 0.0f;
        // (a tap of weight 0 adds nothing -- it is not multiplied: inf * 0 must not reach the sums)
        const bool use = wt != 0.0f;
        r = r + (use ? q.c.x * wt : 0.0f);
        g = g + (use ? q.c.y * wt : 0.0f);
        b = b + (use ? q.c.z * wt : 0.0f);
        vs = vs + (use ? (wt * wt) * q.c.w : 0.0f);
        w = w + wt;
    }
    __host__ __device__ __forceinline__ float4 result(const AtrousPixel& p) const
    {
        if (!atrous_finite3(p.c)) return p.c;
        return make_float4(r / w, g / w, b / w, vs / (w * w));
    }
};

// what the pass body asks of this filter (AtrousTaps' members): the prefilter, and den is what the taps of a centre share
struct AtrousVarTaps {
    using Pixel = AtrousPixel;
    using Sum = AtrousVarSum;
    using Prefilter = AtrousVarPrefilter;
    int32_t npow;
    float sigma_plane, sv2, floor;   // sv2 = sigma_variance * sigma_variance
    __host__ __device__ __forceinline__ bool skip(const float4&) const { return false; }
    __host__ __device__ __forceinline__ float centre(int, const Prefilter& pre) const { return pre.den(sv2, floor); }
    __host__ __device__ __forceinline__ void tap(Sum& sum, const Pixel& p, const Pixel& q, int dx, int dy, float den) const
    {
        sum.tap(p, q, dx, dy, npow, sigma_plane, den);
    }
};

}  // namespace jpt
