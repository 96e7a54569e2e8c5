// jpt_display.h -- the arithmetic of jpt_display ("the display transform"): exposure, a pyramid bloom, a
// selectable tone map and an output transfer over the running mean of the progressive accumulation or over jpt_denoise's image.
// No reference counterpart beyond its fixed unorm8(ACES(mean)) (the reference lists "bloom, controllable tone-mapping" among its
// wanted features).  Everything is + - * /, floor, fabs, compares and selects, one binary32 operation each in source order: the
// device kernels (jpt_kernels_display.hip) and the host form of jpt_debug_display run these functions, and tests/np_display.py
// restates them in float32 numpy bit for bit.  aces_film, unorm8 and clamp_ of the render kernels are restated here (they are
// device-only where they live), with the clamp written as two selects so that host and device agree on -0 and NaN.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

namespace jpt {

constexpr int kDisplayMaxLevels = 6;

struct DisplayParams {   // jpt_display_params
    int32_t source = 0;     // JPT_DISPLAY_SOURCE_ACCUM
    int32_t tonemap = 0;    // JPT_TONEMAP_ACES_REF
    int32_t transfer = 0;   // JPT_TRANSFER_LINEAR
    int32_t bloom_levels = 0;
    float exposure = 1.0f;
    float white = 4.0f;
    float bloom_threshold = 1.0f;
    float bloom_strength = 0.25f;
};

// the checks of jpt_set_display_params, also run by jpt_debug_display
inline int check_display_params(const DisplayParams& p, std::string& why)
{
    if (p.source < 0 || p.source > 1) why = "jpt_display_params: source must be JPT_DISPLAY_SOURCE_ACCUM or JPT_DISPLAY_SOURCE_DENOISED";
    else if (p.tonemap < 0 || p.tonemap > 2) why = "jpt_display_params: tonemap must be JPT_TONEMAP_ACES_REF, _REINHARD or _CLAMP";
    else if (p.transfer < 0 || p.transfer > 1) why = "jpt_display_params: transfer must be JPT_TRANSFER_LINEAR or JPT_TRANSFER_SRGB";
    else if (p.bloom_levels < 0 || p.bloom_levels > kDisplayMaxLevels) why = "jpt_display_params: bloom_levels must be in [0, 6]";
    else if (!std::isfinite(p.exposure) || !(p.exposure >= 0.0f)) why = "jpt_display_params: exposure must be finite and >= 0";
    else if (!std::isfinite(p.white) || !(p.white > 0.0f)) why = "jpt_display_params: white must be finite and > 0";
    else if (!std::isfinite(p.bloom_threshold) || !(p.bloom_threshold >= 0.0f)) why = "jpt_display_params: bloom_threshold must be finite and >= 0";
    else if (!std::isfinite(p.bloom_strength) || !(p.bloom_strength >= 0.0f)) why = "jpt_display_params: bloom_strength must be finite and >= 0";
    else return 0;    // JPT_OK
    return -1;        // JPT_E_INVALID
}

// What the kernels take of the parameters: w2 = white * white and strength_n = bloom_strength / (float)bloom_levels are computed
// once on the host.
struct DisplayConsts {
    int32_t tonemap, transfer, levels;
    float exposure, w2, threshold, strength_n;
};
inline DisplayConsts display_consts(const DisplayParams& p)
{
    DisplayConsts k;
    k.tonemap = p.tonemap;
    k.transfer = p.transfer;
    k.levels = p.bloom_levels;
    k.exposure = p.exposure;
    k.w2 = p.white * p.white;
    k.threshold = p.bloom_threshold;
    k.strength_n = p.bloom_levels > 0 ? p.bloom_strength / (float)p.bloom_levels : 0.0f;
    return k;
}

// T[k], k = 1..255: the binary32 nearest to eotf((k - 0.5) / 255), eotf(e) = e / 12.92 for e <= 0.04045, else
// ((e + 0.055) / 1.055)^2.4 (IEC 61966-2-1), evaluated in binary64.  The sRGB code of a tone-mapped value v is the number of
// entries T[k] <= v: round-to-nearest of the encoded value without a pow on the device.  Entry 0 is not part of the table.
#define JPT_DISPLAY_SRGB_T255 \
    0.000151763496f, 0.000455290487f, 0.000758817478f, 0.00106234441f, 0.0013658714f, 0.00166939839f, 0.00197292538f, 0.00227645249f, \
    0.00257997937f, 0.00288350624f, 0.00318830088f, 0.00350925932f, 0.00384831498f, 0.00420574797f, 0.00458183279f, 0.00497683743f, \
    0.00539102405f, 0.00582465064f, 0.00627796957f, 0.00675122766f, 0.00724466844f, 0.00775853032f, 0.00829304848f, 0.00884845294f, \
    0.00942497049f, 0.0100228256f, 0.010642237f, 0.011283421f, 0.0119465925f, 0.0126319602f, 0.0133397318f, 0.0140701123f, \
    0.0148233026f, 0.0155995032f, 0.0163989104f, 0.0172217153f, 0.0180681143f, 0.0189382937f, 0.0198324434f, 0.0207507443f, \
    0.0216933824f, 0.0226605386f, 0.0236523896f, 0.0246691145f, 0.0257108882f, 0.0267778821f, 0.0278702695f, 0.0289882198f, \
    0.0301319025f, 0.0313014798f, 0.0324971229f, 0.0337189883f, 0.0349672437f, 0.0362420455f, 0.0375435539f, 0.0388719253f, \
    0.04022732f, 0.041609887f, 0.0430197865f, 0.0444571637f, 0.0459221713f, 0.0474149622f, 0.0489356853f, 0.0504844859f, \
    0.0520615056f, 0.0536668971f, 0.055300802f, 0.0569633618f, 0.0586547181f, 0.0603750125f, 0.0621243827f, 0.0639029741f, \
    0.0657109171f, 0.0675483495f, 0.0694154128f, 0.0713122338f, 0.0732389539f, 0.0751957074f, 0.0771826133f, 0.0791998208f, \
    0.0812474415f, 0.0833256245f, 0.085434489f, 0.0875741541f, 0.089744769f, 0.091946438f, 0.0941793025f, 0.0964434743f, \
    0.098739095f, 0.101066269f, 0.10342513f, 0.105815805f, 0.108238399f, 0.110693045f, 0.113179862f, 0.115698971f, \
    0.118250482f, 0.120834522f, 0.123451203f, 0.126100644f, 0.128782958f, 0.131498262f, 0.134246677f, 0.137028307f, \
    0.13984327f, 0.142691687f, 0.145573661f, 0.148489311f, 0.151438728f, 0.15442206f, 0.157439381f, 0.160490826f, \
    0.163576499f, 0.166696489f, 0.169850931f, 0.173039913f, 0.176263571f, 0.179521978f, 0.182815254f, 0.186143503f, \
    0.189506829f, 0.192905352f, 0.196339145f, 0.199808344f, 0.203313038f, 0.206853345f, 0.210429341f, 0.214041144f, \
    0.217688844f, 0.22137256f, 0.225092396f, 0.228848428f, 0.232640758f, 0.236469507f, 0.240334779f, 0.244236633f, \
    0.248175204f, 0.252150565f, 0.256162852f, 0.260212123f, 0.264298469f, 0.268422037f, 0.272582889f, 0.276781112f, \
    0.281016797f, 0.285290092f, 0.289601028f, 0.293949723f, 0.298336297f, 0.30276081f, 0.30722335f, 0.311724037f, \
    0.31626296f, 0.32084018f, 0.325455844f, 0.330109984f, 0.334802747f, 0.339534163f, 0.344304383f, 0.349113464f, \
    0.353961498f, 0.358848572f, 0.363774776f, 0.368740231f, 0.373744965f, 0.378789127f, 0.383872777f, 0.388996005f, \
    0.3941589f, 0.399361521f, 0.404604018f, 0.40988642f, 0.415208817f, 0.420571357f, 0.425974041f, 0.431417018f, \
    0.436900347f, 0.442424119f, 0.447988421f, 0.453593314f, 0.459238917f, 0.464925289f, 0.470652521f, 0.476420701f, \
    0.482229918f, 0.488080233f, 0.493971765f, 0.499904543f, 0.505878687f, 0.511894286f, 0.517951429f, 0.524050117f, \
    0.530190527f, 0.536372721f, 0.542596757f, 0.548862696f, 0.555170655f, 0.561520696f, 0.567912877f, 0.574347317f, \
    0.580824137f, 0.587343335f, 0.593904972f, 0.600509226f, 0.607156098f, 0.613845706f, 0.62057811f, 0.62735337f, \
    0.634171605f, 0.641032875f, 0.647937238f, 0.654884815f, 0.661875665f, 0.668909788f, 0.675987363f, 0.683108449f, \
    0.690273106f, 0.697481334f, 0.704733372f, 0.712029159f, 0.719368815f, 0.72675246f, 0.734180033f, 0.741651773f, \
    0.749167681f, 0.756727815f, 0.764332294f, 0.77198112f, 0.779674411f, 0.787412286f, 0.795194745f, 0.803021908f, \
    0.810893834f, 0.818810523f, 0.826772213f, 0.834778786f, 0.842830479f, 0.850927293f, 0.859069228f, 0.867256522f, \
    0.875489056f, 0.883767068f, 0.892090559f, 0.900459588f, 0.908874214f, 0.917334557f, 0.925840616f, 0.934392571f, \
    0.942990363f, 0.951634169f, 0.960324049f, 0.969060004f, 0.977842152f, 0.986670554f, 0.995545268f
constexpr float kDisplaySrgbT[256] = {0.0f, JPT_DISPLAY_SRGB_T255};

__host__ __device__ __forceinline__ int display_level_size(int n) { return (n + 1) >> 1; }
__host__ __device__ __forceinline__ bool display_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e38f; }
// clamp_ of the render kernels (fmin(fmax(x, lo), hi): a NaN gives lo) as two selects
__host__ __device__ __forceinline__ float display_clamp(float x, float lo, float hi)
{
    const float t = x > lo ? x : lo;
    return t < hi ? t : hi;
}
__host__ __device__ __forceinline__ int display_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 1. base: c = (sum / fc) * exposure
__host__ __device__ __forceinline__ float4 display_base(const float4& sum, float fc, float exposure)
{
    return make_float4((sum.x / fc) * exposure, (sum.y / fc) * exposure, (sum.z / fc) * exposure, 0.0f);
}

// 2. bright pass: what of c lies over the threshold, by luminance; 0 for a pixel with a non-finite channel
__host__ __device__ __forceinline__ float4 display_bright(const float4& c, float threshold)
{
    const float lum = 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z;
    if (!display_finite(c.x) || !display_finite(c.y) || !display_finite(c.z) || !(lum > threshold)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float k = (lum - threshold) / lum;
    return make_float4(c.x * k, c.y * k, c.z * k, 0.0f);
}

// 3. down: the weights (1 3 3 1) / 8 of the 4 x 4 taps at 2x - 1 + i, 2y - 1 + j; a running sum fed j outer, i inner
__host__ __device__ __forceinline__ float display_w4(int i) { return (i == 1 || i == 2) ? 0.375f : 0.125f; }
struct DisplaySum {
    float r = 0.0f, g = 0.0f, b = 0.0f;
    __host__ __device__ __forceinline__ void tap(const float4& v, float wt)
    {
        r = r + v.x * wt;
        g = g + v.y * wt;
        b = b + v.z * wt;
    }
};

// 4. up: the two taps of the 2 x tent along one axis for coordinate p of the finer level; `hi` = the coarser level's last index
__host__ __device__ __forceinline__ void display_tent(int p, int hi, int idx[2], float wt[2])
{
    const int h = p >> 1;
    if ((p & 1) == 0) {
        idx[0] = display_clampi(h - 1, hi);
        idx[1] = display_clampi(h, hi);
        wt[0] = 0.25f;
        wt[1] = 0.75f;
    } else {
        idx[0] = display_clampi(h, hi);
        idx[1] = display_clampi(h + 1, hi);
        wt[0] = 0.75f;
        wt[1] = 0.25f;
    }
}
// T(coarse)(x, y): rows outer, columns inner; coarse is cw x ch pixels
__host__ __device__ __forceinline__ DisplaySum display_tent_sum(const float4* coarse, int cw, int ch, int x, int y)
{
    int ix[2], iy[2];
    float wx[2], wy[2];
    display_tent(x, cw - 1, ix, wx);
    display_tent(y, ch - 1, iy, wy);
    DisplaySum s;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) s.tap(coarse[(size_t)iy[j] * (size_t)cw + (size_t)ix[i]], wy[j] * wx[i]);
    return s;
}

// 6. tone maps
__host__ __device__ __forceinline__ float display_aces(float x)   // aces_film, progressive_rendering.glsl:19-26
{
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    return display_clamp((x * (a * x + b)) / (x * (c * x + d) + e), 0.0f, 1.0f);
}
__host__ __device__ __forceinline__ float display_reinhard(float o, float w2)
{
    return display_clamp((o * (1.0f + o / w2)) / (1.0f + o), 0.0f, 1.0f);
}
__host__ __device__ __forceinline__ float display_tonemap(int mode, float o, float w2)
{
    return mode == 0 ? display_aces(o) : (mode == 1 ? display_reinhard(o, w2) : display_clamp(o, 0.0f, 1.0f));
}

// 7. transfers: unorm8 of the render kernels, and the search of the table (t[1..255], eight steps)
__host__ __device__ __forceinline__ uint32_t display_unorm8(float v)
{
    return (uint32_t)__builtin_floorf(display_clamp(v, 0.0f, 1.0f) * 255.0f + 0.5f);
}
__host__ __device__ __forceinline__ uint32_t display_srgb_code(float v, const float* t)
{
    uint32_t code = 0;
    for (uint32_t step = 128; step != 0; step >>= 1)
        if (t[code + step] <= v) code += step;
    return code;
}

// 5.-7. of one pixel: o = c + bloom * strength_n (HAVE_BLOOM), the tone map, the transfer; v = the tone-mapped value
template <bool HAVE_BLOOM>
__host__ __device__ __forceinline__ uint32_t display_resolve(const DisplayConsts& k, const float4& c, const DisplaySum& bloom, const float* srgb_t,
                                                             float4& v)
{
    float ox = c.x, oy = c.y, oz = c.z;
    if (HAVE_BLOOM) {
        ox = c.x + bloom.r * k.strength_n;
        oy = c.y + bloom.g * k.strength_n;
        oz = c.z + bloom.b * k.strength_n;
    }
    v = make_float4(display_tonemap(k.tonemap, ox, k.w2), display_tonemap(k.tonemap, oy, k.w2), display_tonemap(k.tonemap, oz, k.w2), 1.0f);
    if (k.transfer == 1) return display_srgb_code(v.x, srgb_t) | (display_srgb_code(v.y, srgb_t) << 8) | (display_srgb_code(v.z, srgb_t) << 16) | 0xFF000000u;
    return display_unorm8(v.x) | (display_unorm8(v.y) << 8) | (display_unorm8(v.z) << 16) | 0xFF000000u;
}

// elements of the pyramid D_1 .. D_levels of a width x height image, and where level k (1-based) starts
inline size_t display_pyramid_elems(int32_t width, int32_t height, int levels, size_t* offsets /* [levels + 1], may be null */)
{
    size_t total = 0;
    int w = width, h = height;
    for (int k = 1; k <= levels; k++) {
        w = display_level_size(w);
        h = display_level_size(h);
        if (offsets) offsets[k] = total;
        total += (size_t)w * (size_t)h;
    }
    return total;
}

// the whole transform on the host (jpt_debug_display with device -1): src = sums (or an image, fc = 1); either output may be null
inline void display_host(int32_t width, int32_t height, const DisplayParams& prm, const float4* src, float fc, float4* out_f32, uint32_t* out_rgba8)
{
    const DisplayConsts k = display_consts(prm);
    const int N = k.levels;
    const size_t n = (size_t)width * height;
    float4* lvl[kDisplayMaxLevels + 1] = {};
    int lw[kDisplayMaxLevels + 1], lh[kDisplayMaxLevels + 1];
    lw[0] = width;
    lh[0] = height;
    if (N > 0) {
        lvl[0] = new float4[n];
        for (size_t i = 0; i < n; i++) lvl[0][i] = display_bright(display_base(src[i], fc, k.exposure), k.threshold);
        for (int l = 0; l < N; l++) {
            const int w = lw[l], h = lh[l], cw = display_level_size(w), ch = display_level_size(h);
            lw[l + 1] = cw;
            lh[l + 1] = ch;
            lvl[l + 1] = new float4[(size_t)cw * ch];
            for (int y = 0; y < ch; y++)
                for (int x = 0; x < cw; x++) {
                    DisplaySum s;
                    for (int j = 0; j < 4; j++)
                        for (int i = 0; i < 4; i++) {
                            const int sx = display_clampi(2 * x - 1 + i, w - 1), sy = display_clampi(2 * y - 1 + j, h - 1);
                            s.tap(lvl[l][(size_t)sy * w + sx], display_w4(j) * display_w4(i));
                        }
                    lvl[l + 1][(size_t)y * cw + x] = make_float4(s.r, s.g, s.b, 0.0f);
                }
        }
        for (int l = N - 1; l >= 1; l--)
            for (int y = 0; y < lh[l]; y++)
                for (int x = 0; x < lw[l]; x++) {
                    const DisplaySum t = display_tent_sum(lvl[l + 1], lw[l + 1], lh[l + 1], x, y);
                    float4& d = lvl[l][(size_t)y * lw[l] + x];
                    d = make_float4(d.x + t.r, d.y + t.g, d.z + t.b, 0.0f);
                }
    }
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const float4 c = display_base(src[i], fc, k.exposure);
            float4 v;
            uint32_t q;
            if (N > 0) q = display_resolve<true>(k, c, display_tent_sum(lvl[1], lw[1], lh[1], x, y), kDisplaySrgbT, v);
            else q = display_resolve<false>(k, c, DisplaySum(), kDisplaySrgbT, v);
            if (out_f32) out_f32[i] = v;
            if (out_rgba8) out_rgba8[i] = q;
        }
    for (int l = 0; l <= N; l++) delete[] lvl[l];
}

// jpt_display's launches (jpt_kernels_display.hip), on `stream`: from `src` (width * height sums, or an image with fc = 1) to the
// tone-mapped image `out_f32` ((r, g, b, 1)) and its encoded image `out_rgba8`.  `pyramid` holds display_pyramid_elems(width,
// height, bloom_levels) elements and is written only when bloom_levels > 0 (else it may be null).  Nothing else is written.
// `metered` (jpt_set_auto_exposure; else null): the device's metered exposure, read by kernels of their own as the launches run;
// the exposure is then prm.exposure * *metered, one binary32 multiply, in the bloom's base and in the resolve.
void launch_display(hipStream_t stream, const DisplayParams& prm, int width, int height, const float4* src, float fc, float4* pyramid,
                    float4* out_f32, uint32_t* out_rgba8, const float* metered = nullptr);

}  // namespace jpt
