// jpt_shade.h -- per-path device code shared by every tracing kernel: RNG, primary-ray generation,
// shading-record fetch, the diffuse + GGX mixture BRDF with VNDF sampling, and the path update.
// Replaces main.glsl:163-222,372-421 and brdfs.glsl:1-138 of the reference
// (project/addons/jar_path_tracing/src/shaders/).
#pragma once

#include "jpt_device_math.h"
#include "jpt_types.h"

namespace jpt {

#define JPT_PI 3.141592653589793238462643f  // brdfs.glsl:1

struct Ray {  // main.glsl:26-30
    f3 o, d, rD;
};

struct Hit {  // the fields of HitInfo (main.glsl:62-71) that survive traversal
    float t;
    float u, v;
    uint32_t tri;   // index into the reference-order triangle arrays
    uint32_t inst;  // BLAS instance id
    f3 lo, ld;      // ray origin / direction in the hit instance's local space (position = lo + t*ld)
};

struct Shading {  // main.glsl:73-82
    f3 position, normal, out_dir;
    float lambert_out;
    f3 emission, diffuse_albedo, fresnel_0;
    float roughness;
};

struct SceneShading {  // cold, once-per-hit data: kept in the reference layout
    const ShadeTri* __restrict__ tri_data;
    const RefInstance* __restrict__ instances;
    const RefMaterial* __restrict__ materials;
    const uint8_t* __restrict__ tex;
    const ReachTri* __restrict__ reach_tri;    // reach records (jpt_types.h), null when the scene has none
    const ReachInst* __restrict__ reach_inst;
    bool retrace_ties;                         // the reference's own trees are on the device: a hit the walk flagged as an exact
                                               // distance tie is set aside and traced again on them (wf2_finish)
    uint32_t n_materials, n_instances;
    int32_t tex_res, n_layers;
    int32_t sampler_mode;  // JPT_SAMPLER_*: bit 0 repeat, bit 1 linear
};

// ---- the environment map (jpt_set_environment): what a ray that leaves the scene sees instead of sample_sky -------------------

constexpr int32_t kEnvMaxWidth = 16384, kEnvMaxHeight = 8192;

// The map as the kernels see it, passed by value with every render: w x h texels (r, g, b, 0), row-major, row 0 the +y pole;
// `rot` the row-major world -> map rotation, `intensity` the scale of every texel.
struct EnvDev {
    const float4* __restrict__ texels;
    int32_t w, h;
    float rot[9];
    float intensity;
};

// the column / row of a floor()ed texel coordinate: columns wrap modulo w, rows clamp to [0, h - 1], a NaN is 0 (tex_index's rules)
__host__ __device__ __forceinline__ int32_t env_column(float f, int32_t w)
{
    if (f != f || f >= 1073741824.0f || f <= -1073741824.0f) return 0;
    const int32_t i = (int32_t)f % w;
    return i < 0 ? i + w : i;
}
__host__ __device__ __forceinline__ int32_t env_row(float f, int32_t h)
{
    if (f != f) return 0;
    if (f >= (float)(h - 1)) return h - 1;
    return f <= 0.0f ? 0 : (int32_t)f;
}
__host__ __device__ __forceinline__ float env_lerp(float p, float q, float t) { return p + t * (q - p); }

// The radiance the map sends along world direction d (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations,
// restated in numpy by tests/test_environment_host.py).  m = R d; phi = atan2(m.x, -m.z), theta = atan2(|m.xz|, m.y); bilinear
// between the texel centres around ((phi / 2pi + 1/2) w - 1/2, theta / pi h - 1/2), times the intensity.  The device and the host
// mirror (jpt_debug_env_lookup) run this one function.
__host__ __device__ __forceinline__ f3 env_radiance(const EnvDev& e, f3 d)
{
    const float mx = e.rot[0] * d.x + e.rot[1] * d.y + e.rot[2] * d.z;
    const float my = e.rot[3] * d.x + e.rot[4] * d.y + e.rot[5] * d.z;
    const float mz = e.rot[6] * d.x + e.rot[7] * d.y + e.rot[8] * d.z;
    const float phi = atan2_(mx, -mz);
    const float theta = atan2_(__builtin_sqrtf(mx * mx + mz * mz), my);
    const float fu = (phi * 0.159154943f + 0.5f) * (float)e.w - 0.5f;   // 1 / 2pi
    const float fv = theta * 0.318309886f * (float)e.h - 0.5f;          // 1 / pi
    const float i0 = __builtin_floorf(fu), j0 = __builtin_floorf(fv);
    float a = fu - i0, b = fv - j0;
    if (a != a) a = 0.0f;
    if (b != b) b = 0.0f;
    const uint32_t x0 = (uint32_t)env_column(i0, e.w), x1 = (uint32_t)env_column(i0 + 1.0f, e.w);
    const uint32_t r0 = (uint32_t)env_row(j0, e.h) * (uint32_t)e.w, r1 = (uint32_t)env_row(j0 + 1.0f, e.h) * (uint32_t)e.w;
    const float4 t00 = e.texels[r0 + x0], t10 = e.texels[r0 + x1], t01 = e.texels[r1 + x0], t11 = e.texels[r1 + x1];
    const float cx = env_lerp(env_lerp(t00.x, t10.x, a), env_lerp(t01.x, t11.x, a), b);
    const float cy = env_lerp(env_lerp(t00.y, t10.y, a), env_lerp(t01.y, t11.y, a), b);
    const float cz = env_lerp(env_lerp(t00.z, t10.z, a), env_lerp(t01.z, t11.z, a), b);
    return f3{cx * e.intensity, cy * e.intensity, cz * e.intensity};
}

// ---- importance sampling of the map (jpt_set_environment_sampling, JPT_ENV_SAMPLING_MIS) -------------------------------------
//
// A piecewise-constant distribution over the texels: texel (i, j) of row i weighs lum(i, j) * sin(theta_i), theta_i the row
// centre's polar angle, lum = 0.2126 r + 0.7152 g + 0.0722 b (the intensity scales every texel alike: the tables are the map's).
// Per row a conditional CDF over its columns, and a marginal CDF over the rows, both normalised sequential prefix sums whose last
// entry is exactly 1 (a row of weight 0 is all 1s).  Built by one function, on the device (env_tables_rows / env_tables_marginal,
// jpt_kernels_post.hip) and on the host (jpt_debug_env_tables), so the two give the same bits.

struct EnvSampDev {   // the tables of the context's map, passed by value with every MIS render
    const float* __restrict__ cond;   // h rows of w entries
    const float* __restrict__ marg;   // h entries
    float total;                      // sum of all weights; 0: the map is black and is never sampled (pdf 0)
};

__host__ __device__ __forceinline__ float env_row_sin(int32_t i, int32_t h)
{
    float s, c;
    sincos_(((float)i + 0.5f) / (float)h * 3.14159274f, s, c);
    return s;
}
__host__ __device__ __forceinline__ float env_weight(const float4 t, float row_sin)
{
    return (0.2126f * t.x + 0.7152f * t.y + 0.0722f * t.z) * row_sin;
}
// row i of the conditional CDF (w entries at `out`); returns the row's weight
__host__ __device__ __forceinline__ float env_build_row(const float4* texels, int32_t w, int32_t h, int32_t i, float* out)
{
    const float rs = env_row_sin(i, h);
    float sum = 0.0f;
    for (int32_t j = 0; j < w; j++) {
        sum = sum + env_weight(texels[(size_t)i * (size_t)w + (size_t)j], rs);
        out[j] = sum;
    }
    for (int32_t j = 0; j < w - 1; j++) out[j] = sum > 0.0f ? out[j] / sum : 1.0f;
    out[w - 1] = 1.0f;
    return sum;
}
// the marginal CDF from the rows' weights (in place, h entries); returns the total
__host__ __device__ __forceinline__ float env_build_marginal(float* rows, int32_t h)
{
    float sum = 0.0f;
    for (int32_t i = 0; i < h; i++) {
        sum = sum + rows[i];
        rows[i] = sum;
    }
    for (int32_t i = 0; i < h - 1; i++) rows[i] = sum > 0.0f ? rows[i] / sum : 1.0f;
    rows[h - 1] = 1.0f;
    return sum;
}
// the first k in [0, n) with cdf[k] > x (np.searchsorted(cdf, x, side="right")), for x < cdf[n - 1] = 1
__host__ __device__ __forceinline__ int32_t env_upper_bound(const float* cdf, int32_t n, float x)
{
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// The density, per unit solid angle, with which env_sample draws world direction d: (weight_ij / total) * w h / (2 pi^2 sin theta),
// (i, j) the texel the lookup's mapping puts d in (m = R d, u = phi / 2pi + 1/2, v = theta / pi), sin theta = |m.xz|.  0 when
// sin theta = 0 or the map is black.
__host__ __device__ __forceinline__ float env_pdf(const EnvDev& e, const EnvSampDev& s, f3 d)
{
    if (!(s.total > 0.0f)) return 0.0f;
    const float mx = e.rot[0] * d.x + e.rot[1] * d.y + e.rot[2] * d.z;
    const float my = e.rot[3] * d.x + e.rot[4] * d.y + e.rot[5] * d.z;
    const float mz = e.rot[6] * d.x + e.rot[7] * d.y + e.rot[8] * d.z;
    const float sin_t = __builtin_sqrtf(mx * mx + mz * mz);
    if (!(sin_t > 0.0f)) return 0.0f;
    const float phi = atan2_(mx, -mz);
    const float theta = atan2_(sin_t, my);
    const int32_t j = env_column(__builtin_floorf((phi * 0.159154943f + 0.5f) * (float)e.w), e.w);
    const int32_t i = env_row(__builtin_floorf(theta * 0.318309886f * (float)e.h), e.h);
    const float wt = env_weight(e.texels[(size_t)i * (size_t)e.w + (size_t)j], env_row_sin(i, e.h));
    return wt / s.total * ((float)e.w * (float)e.h) / (19.7392088f * sin_t);   // 2 pi^2
}
// A world direction drawn with the tables from (xi0, xi1) in [0, 1] (each clamped below 1): the row by xi1 on the marginal CDF,
// the column by xi0 on the row's conditional CDF, the point inside the texel by where xi falls between the texel's CDF entries;
// u, v -> phi = (u - 1/2) 2pi, theta = v pi -> m = (sin theta sin phi, cos theta, -sin theta cos phi), d = R^T m.  pdf_out =
// env_pdf(d).  A black map: d = 0, pdf 0.
__host__ __device__ __forceinline__ f3 env_sample(const EnvDev& e, const EnvSampDev& s, float xi0, float xi1, float& pdf_out)
{
    pdf_out = 0.0f;
    if (!(s.total > 0.0f)) return f3{0.0f, 0.0f, 0.0f};
    xi0 = xi0 < 0.99999994f ? xi0 : 0.99999994f;
    xi1 = xi1 < 0.99999994f ? xi1 : 0.99999994f;
    const int32_t i = env_upper_bound(s.marg, e.h, xi1);
    const float m0 = i > 0 ? s.marg[i - 1] : 0.0f, m1 = s.marg[i];
    const float* row = s.cond + (size_t)i * (size_t)e.w;
    const int32_t j = env_upper_bound(row, e.w, xi0);
    const float c0 = j > 0 ? row[j - 1] : 0.0f, c1 = row[j];
    const float dv = (xi1 - m0) / (m1 - m0), du = (xi0 - c0) / (c1 - c0);
    const float u = ((float)j + du) / (float)e.w, v = ((float)i + dv) / (float)e.h;
    float st, ct, sp, cp;
    sincos_(v * 3.14159274f, st, ct);
    sincos_((u - 0.5f) * 6.28318548f, sp, cp);
    const float mx = st * sp, my = ct, mz = -(st * cp);
    const f3 d{e.rot[0] * mx + e.rot[3] * my + e.rot[6] * mz, e.rot[1] * mx + e.rot[4] * my + e.rot[7] * mz,
               e.rot[2] * mx + e.rot[5] * my + e.rot[8] * mz};
    pdf_out = env_pdf(e, s, d);
    return d;
}

// ---- importance sampling of the emissive triangles (jpt_set_light_sampling, JPT_LIGHT_SAMPLING_MIS) ---------------------------
//
// An emitter is an (instance, triangle) pair whose emission Le (get_shading_data's material lookup: emission.rgb * max(0,
// emission.w)) has luminance lum(Le) = 0.2126 r + 0.7152 g + 0.0722 b > 0; the host lists them (instance-major, triangles in
// ascending index), the device derives their world geometry and power, lum(Le) * world area, from the arrays the renders read
// (light_tables_*, jpt_kernels_post.hip).  A power that is not finite and > 0 (zero-area, degenerate) is 0: never drawn.
// Emitters fall into blocks of kLightBlock; per block a normalised sequential prefix sum (the last entry exactly 1, a block of
// power 0 all 1s), then the same over the block totals -- env_build_marginal on both levels.

constexpr uint32_t kLightBlock = 256;

struct LightDev {   // the tables of the context's scene, passed by value with every light-sampling render
    const float4* __restrict__ tri;   // per emitter three entries: (P0, Le.r), (E1, Le.g), (E2, Le.b) -- world vertex 0 and edges
    const float* __restrict__ cdf;    // per emitter: the conditional CDF of its block
    const float* __restrict__ marg;   // per block: the marginal CDF; marg[n_blocks] = the total power
    const WideTri* __restrict__ wtris;   // the scene's triangle records: the hit triangle's edges (light_hit_weight)
    uint32_t n, n_blocks;
};

__host__ __device__ __forceinline__ float light_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// Le of triangle slot `slot` of instance `inst`: get_shading_data's lookup (an unchecked slot reads on into the next instance's
// record, a word past the array is material 0, an out-of-range index is material 0)
__host__ __device__ __forceinline__ void light_emission(const RefInstance* instances, uint32_t n_instances, const RefMaterial* materials,
                                                       uint32_t n_materials, uint32_t inst, uint32_t slot, float* le)
{
    const unsigned long long word = (unsigned long long)inst * 44ull + 41ull + (unsigned long long)slot;
    uint32_t mat_id = word < (unsigned long long)n_instances * 44ull ? reinterpret_cast<const uint32_t*>(instances)[word] : 0u;
    if (mat_id >= n_materials) mat_id = 0;
    const RefMaterial& m = materials[mat_id];
    const float em = m.emission.w > 0.0f ? m.emission.w : 0.0f;   // fmax(0, w), NaN -> 0
    le[0] = m.emission.x * em;
    le[1] = m.emission.y * em;
    le[2] = m.emission.z * em;
}

// ---- transparent materials (jpt_set_material_extensions, JPT_MATERIAL_EXT_TRANSMISSION) --------------------------------------
//
// GpuMaterial's padding[0] / padding[1] as transmission / ior, sanitised here: what the *_tx kernels and the host's scan of its
// materials mirror (lighting_bound, jpt_lighting.cpp) both run.
__host__ __device__ __forceinline__ float material_transmission(float t)   // NaN -> 0, then [0, 1]
{
    t = t == t ? t : 0.0f;
    return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
}
__host__ __device__ __forceinline__ float material_ior(float i)   // NaN -> 1, then [1, 4]
{
    i = i == i ? i : 1.0f;
    return i < 1.0f ? 1.0f : (i > 4.0f ? 4.0f : i);
}

// What a dielectric vertex leaves where the BRDF density of its sampled direction would go (Wf2Nee::pdf, the audit kernel's
// p_brdf): the next vertex's emission and miss weights are exactly 1.  No density is -1 (they are >= 0 or NaN).
constexpr float kDeltaDensity = -1.0f;

// One smooth dielectric event (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations; tests/np_transmission.py
// restates it).  n: the facing shading normal, v: the direction back along the ray (both unit), ior: the material's (sanitised
// here), front: the ray arrives from outside.  m = n, or -n when n.v < 0 (a shading normal tilted past the ray: the event happens
// on the side the ray is on); c = min(|n.v|, 1); eta = 1 / ior (front) or ior, eta' its inverse ratio, ior or 1 / ior;
// k = 1 - (eta eta)(1 - c c).  k < 0: total internal reflection, F = 1, returns 2.  Otherwise ct = sqrt(k),
// F = 0.5 (rs rs + rp rp), rs = (c - eta' ct) / (c + eta' ct), rp = (ct - eta' c) / (ct + eta' c); an F that is not <= 1 (0 / 0 at
// grazing incidence with ior 1) is 1.  xi_f < F: reflection, returns 1; else refraction, returns 0.
// Reflection (1, 2): d = m (2 c) - v, as it is.  Refraction: d = normalize(m (eta c - ct) - v eta).  No NaN from unit n, v.
__host__ __device__ __forceinline__ int dielectric_event(f3 n, f3 v, float ior, bool front, float xi_f, f3& d, float& fresnel)
{
    ior = material_ior(ior);
    const float ndv = n.x * v.x + n.y * v.y + n.z * v.z;
    const bool below = ndv < 0.0f;
    const f3 m{below ? -n.x : n.x, below ? -n.y : n.y, below ? -n.z : n.z};
    float c = __builtin_fabsf(ndv);
    c = c < 1.0f ? c : 1.0f;
    const float inv = 1.0f / ior;
    const float eta = front ? inv : ior, etap = front ? ior : inv;
    const float k = 1.0f - (eta * eta) * (1.0f - c * c);
    int event = 2;
    float ct = 0.0f;
    fresnel = 1.0f;
    if (!(k < 0.0f)) {
        ct = __builtin_sqrtf(k);
        const float a = etap * ct, b = etap * c;
        const float rs = (c - a) / (c + a), rp = (ct - b) / (ct + b);
        const float f = 0.5f * (rs * rs + rp * rp);
        fresnel = f <= 1.0f ? f : 1.0f;
        event = xi_f < fresnel ? 1 : 0;
    }
    if (event != 0) {
        const float t = 2.0f * c;
        d = f3{m.x * t - v.x, m.y * t - v.y, m.z * t - v.z};
    } else {
        const float g = eta * c - ct;
        const f3 r{m.x * g - v.x * eta, m.y * g - v.y * eta, m.z * g - v.z * eta};
        const float il = 1.0f / __builtin_sqrtf(r.x * r.x + r.y * r.y + r.z * r.z);
        d = f3{r.x * il, r.y * il, r.z * il};
    }
    return event;
}

#if defined(__HIPCC__)   // (everything below is device code; the host layer -- jpt_capi.cpp, jpt_multi.cpp -- sees the structs above only)

// ---- RNG (main.glsl:163-181) -----------------------------------------------------------------

__host__ __device__ __forceinline__ void pcg2d(uint32_t& sx, uint32_t& sy, float& rx, float& ry)
{
    uint32_t x = 1664525u * sx + 1013904223u;
    uint32_t y = 1664525u * sy + 1013904223u;
    x += 1664525u * y;
    y += 1664525u * x;
    x ^= x >> 16;
    y ^= y >> 16;
    x += 1664525u * y;
    y += 1664525u * x;
    x ^= x >> 16;
    y ^= y >> 16;
    sx = x;
    sy = y;
    rx = (float)x * 2.32830643654e-10f;
    ry = (float)y * 2.32830643654e-10f;
}

__host__ __device__ __forceinline__ void prng_seed(uint32_t px, uint32_t py, uint32_t frame, uint32_t& sx, uint32_t& sy)
{
    uint32_t x = px * 0x9e3779b9u + frame;
    uint32_t y = py * 0x9e3779b9u + frame;
    x ^= x >> 16;
    y ^= y >> 16;
    sx = x * 0x9e3779b9u;
    sy = y * 0x9e3779b9u;
}

// ---- primary ray (main.glsl:405-421, box_muller :183-187) -------------------------------------

__host__ __device__ __forceinline__ Ray primary_ray(const RefCamera& cam, int width, int height, int px, int py, uint32_t frame,
                                           uint32_t& sx, uint32_t& sy)
{
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    r1 = r1 * 0.25f;
    // box_muller: R = sqrt(-2 log(r0)) is dead code in the reference; only theta is used
    float js, jc;
    sincos_(6.2831853f * r1, js, jc);
    const float scx = ((float)px + jc) / (float)width * 2.0f - 1.0f;
    const float scy = ((float)py + js) / (float)height * 2.0f - 1.0f;
    const float nx = scx, ny = -scy;
    const float* m = cam.ivp;
    float wx = m[0] * nx + m[4] * ny + m[8] + m[12];
    float wy = m[1] * nx + m[5] * ny + m[9] + m[13];
    float wz = m[2] * nx + m[6] * ny + m[10] + m[14];
    const float ww = m[3] * nx + m[7] * ny + m[11] + m[15];
    wx = wx / ww;
    wy = wy / ww;
    wz = wz / ww;
    Ray ray;
    ray.o = mk3(cam.position.x, cam.position.y, cam.position.z);
    ray.d = normalize3(mk3(wx, wy, wz) - ray.o);
    ray.rD = rcp3(ray.d);
    return ray;
}

// The ray through an exact raster position (no jitter): the arithmetic of primary_ray from `scx` on.  Used to bound what the
// jittered rays of a pixel can see (wf2_accumulate); `ww_out` = the clip-space w the position divides by.
__device__ __forceinline__ f3 raster_direction(const RefCamera& cam, int width, int height, float fx, float fy, float& ww_out)
{
    const float scx = fx / (float)width * 2.0f - 1.0f;
    const float scy = fy / (float)height * 2.0f - 1.0f;
    const float nx = scx, ny = -scy;
    const float* m = cam.ivp;
    float wx = m[0] * nx + m[4] * ny + m[8] + m[12];
    float wy = m[1] * nx + m[5] * ny + m[9] + m[13];
    float wz = m[2] * nx + m[6] * ny + m[10] + m[14];
    const float ww = m[3] * nx + m[7] * ny + m[11] + m[15];
    ww_out = ww;
    wx = wx / ww;
    wy = wy / ww;
    wz = wz / ww;
    return normalize3(mk3(wx, wy, wz) - mk3(cam.position.x, cam.position.y, cam.position.z));
}

// The same direction to a few ulp, for callers that only BOUND what a pixel's rays can see (wf2_accumulate's sky cells, which
// keep a margin a thousand times the rounding of this arithmetic): the six divisions and the square root of raster_direction as
// reciprocal estimates (v_rcp_f32 / v_rsq_f32, 1 ulp each), 30 instructions instead of 90.  Never used for a value that is stored.
__device__ __forceinline__ f3 raster_direction_approx(const RefCamera& cam, float two_over_w, float two_over_h, float fx, float fy, float& ww_out)
{
    const float nx = fx * two_over_w - 1.0f, ny = -(fy * two_over_h - 1.0f);
    const float* m = cam.ivp;
    const float wx = m[0] * nx + m[4] * ny + m[8] + m[12];
    const float wy = m[1] * nx + m[5] * ny + m[9] + m[13];
    const float wz = m[2] * nx + m[6] * ny + m[10] + m[14];
    const float ww = m[3] * nx + m[7] * ny + m[11] + m[15];
    ww_out = ww;
    const float iw = __builtin_amdgcn_rcpf(ww);
    const f3 v = mk3(wx * iw - cam.position.x, wy * iw - cam.position.y, wz * iw - cam.position.z);
    const float il = __builtin_amdgcn_rsqf(v.x * v.x + v.y * v.y + v.z * v.z);
    return mk3(v.x * il, v.y * il, v.z * il);
}

__device__ __forceinline__ f3 sample_sky(f3 d)  // main.glsl:189-192
{
    const float t = 0.5f * (d.y + 1.0f);
    return mk3(mix_(0.95f, 0.9f, t) * 1.0f, mix_(0.95f, 0.94f, t) * 1.0f, mix_(0.95f, 1.0f, t) * 1.0f);
}

// texture(textureArray, vec3(uv, layer)) (main.glsl:214).  The sampler state is a parameter (jpt_set_params); what
// each mode computes is pinned in oracle/oracle_trace.c::sample_texture (Vulkan texel addressing: nearest floor(u*res),
// linear around u*res - 0.5, clamp-to-edge or non-negative modulo, mix() of the four UNORM8 texels, no sRGB decode).
__device__ __forceinline__ int tex_index(float f, int res, bool repeat)
{
    if (f != f) return 0;
    if (!repeat) {   // clamp-to-edge saturates BEFORE the cast: +inf and 1e9 are the last texel, -inf the first
        if (f >= (float)(res - 1)) return res - 1;
        return f <= 0.0f ? 0 : (int)f;
    }
    if (f >= 1073741824.0f || f <= -1073741824.0f) return 0;   // repeat: the modulo of a float this large is not defined by the pin
    int i = (int)f;
    i %= res;
    return i < 0 ? i + res : i;
}
__device__ __forceinline__ f3 texel(const SceneShading& sc, int layer, int ix, int iy)
{
    const uint32_t p = reinterpret_cast<const uint32_t*>(sc.tex)[((size_t)layer * sc.tex_res + iy) * sc.tex_res + ix];
    return mk3(from_unorm8(p & 255u), from_unorm8((p >> 8) & 255u), from_unorm8((p >> 16) & 255u));
}
// FILTER: 0 the sampler mode's own bit decides at run time, 1 nearest only, 2 linear only (the shading kernel is instantiated
// per filter: the bilinear path's four texels and weights cost it a wave per SIMD)
template <int FILTER = 0>
__device__ __forceinline__ f3 sample_texture(const SceneShading& sc, float u, float v, int layer)
{
    if (!sc.tex || sc.n_layers <= 0 || sc.tex_res <= 0) return mk3(0.0f, 0.0f, 0.0f);
    if (layer >= sc.n_layers) layer = sc.n_layers - 1;
    const int res = sc.tex_res;
    const bool repeat = (sc.sampler_mode & 1) != 0, linear = FILTER == 0 ? (sc.sampler_mode & 2) != 0 : FILTER == 2;
    const float x = u * (float)res, y = v * (float)res;
    if (!linear) return texel(sc, layer, tex_index(__builtin_floorf(x), res, repeat), tex_index(__builtin_floorf(y), res, repeat));
    const float xs = x - 0.5f, ys = y - 0.5f;
    const float fx = __builtin_floorf(xs), fy = __builtin_floorf(ys);
    float a = xs - fx, b = ys - fy;
    if (a != a) a = 0.0f;
    if (b != b) b = 0.0f;
    const int x0 = tex_index(fx, res, repeat), x1 = tex_index(fx + 1.0f, res, repeat);
    const int y0 = tex_index(fy, res, repeat), y1 = tex_index(fy + 1.0f, res, repeat);
    const f3 t00 = texel(sc, layer, x0, y0), t10 = texel(sc, layer, x1, y0);
    const f3 t01 = texel(sc, layer, x0, y1), t11 = texel(sc, layer, x1, y1);
    const f3 r0 = mk3(mix_(t00.x, t10.x, a), mix_(t00.y, t10.y, a), mix_(t00.z, t10.z, a));
    const f3 r1 = mk3(mix_(t01.x, t11.x, a), mix_(t01.y, t11.y, a), mix_(t01.z, t11.z, a));
    return mk3(mix_(r0.x, r1.x, b), mix_(r0.y, r1.y, b), mix_(r0.z, r1.z, b));
}

// ---- shading record (main.glsl:194-222) -------------------------------------------------------

// the triangle's shading record as four aligned 16-byte loads: n0.xyz n1.x | n1.yz n2.xy | n2.z uv0 uv1.x | uv1.y uv2 slot
struct ShadeTriRegs {
    float4 q0, q1, q2, q3;
};
__device__ __forceinline__ ShadeTriRegs load_shade_tri(const SceneShading& sc, uint32_t tri)
{
    const float4* tq = reinterpret_cast<const float4*>(sc.tri_data + tri);
    return ShadeTriRegs{tq[0], tq[1], tq[2], tq[3]};
}

// (the record is passed in so that a caller can ask for it early, together with its other gathers)
// TEX = 0: the scene has no texture array, so texture() returns zero for every material that names a layer (what
// sample_texture answers then, without carrying the sampler code in the kernel)
// (TEX: 0 no texture array, 1 nearest filter, 2 linear filter, 3 either, decided by the sampler mode at run time)
template <int TEX = 3>
__device__ __forceinline__ Shading get_shading_data(const SceneShading& sc, const Hit& h, bool front, const ShadeTriRegs& tr)
{
    Shading s;
    const float4 q0 = tr.q0, q1 = tr.q1, q2 = tr.q2, q3 = tr.q3;
    const RefInstance& b = sc.instances[h.inst];
    const uint32_t slot = __float_as_uint(q3.w);
    // b.materials[tri.materialIndex] is unchecked in the reference (main.glsl:198): slots past 2 read on into the next
    // instance's record; a read past the END of the instance buffer returns 0 (Vulkan robust buffer access; the same
    // pin as the oracle's), so no uploaded material_index can make the kernel read outside the array
    const unsigned long long word = (unsigned long long)h.inst * 44ull + 41ull + (unsigned long long)slot;
    uint32_t mat_id = word < (unsigned long long)sc.n_instances * 44ull ? reinterpret_cast<const uint32_t*>(sc.instances)[word] : 0u;
    if (mat_id >= sc.n_materials) mat_id = 0;
    const RefMaterial& material = sc.materials[mat_id];

    const float u = h.u, v = h.v;
    const float w0 = 1.0f - u - v;
    // (the texture first, while little else is live: the sampler's four texels and weights are the kernel's register peak;
    // the operations and their order per value are those of main.glsl:200-218 wherever they stand)
    f3 albedo = mk3(material.albedo.x, material.albedo.y, material.albedo.z);
    if (material.albedo_texture_index >= 0) {
        const float uvx = q2.y * w0 + q2.w * u + q3.y * v;
        const float uvy = q2.z * w0 + q3.x * u + q3.z * v;
        albedo = albedo * (TEX == 0 ? mk3(0.0f, 0.0f, 0.0f) : sample_texture<(TEX == 3 ? 0 : TEX)>(sc, uvx, uvy, material.albedo_texture_index));
    }
    const f3 lpos = h.lo + h.ld * h.t;  // hitInfo.position = ray.o + t * ray.d (main.glsl:249)
    s.position = xform_point(b.transform, lpos);
    s.out_dir = normalize3(xform_dir(b.transform, -h.ld));
    f3 n = mk3(q0.x, q0.y, q0.z) * w0 + mk3(q0.w, q1.x, q1.y) * u + mk3(q1.z, q1.w, q2.x) * v;
    n = normalize3(xform_dir(b.transform, n));
    s.normal = front ? n : -n;

    s.lambert_out = dot3(s.normal, s.out_dir);
    const float em = fmax_(0.0f, material.emission.w);
    s.emission = mk3(material.emission.x * em, material.emission.y * em, material.emission.z * em);

    const float metalicity = material.metallic;
    s.fresnel_0 = mk3(mix_(0.02f, albedo.x, metalicity), mix_(0.02f, albedo.y, metalicity), mix_(0.02f, albedo.z, metalicity));
    s.diffuse_albedo = albedo - albedo * metalicity;
    s.roughness = fmax_(0.006f, material.roughness);
    return s;
}

// ---- BRDF (brdfs.glsl) ------------------------------------------------------------------------

__device__ __forceinline__ float schlick_factor(float cosine_theta)  // brdfs.glsl:4-6
{
    const float factor = 1.0f - cosine_theta;
    const float factor_squared = factor * factor;
    return factor_squared * factor_squared * factor;
}

__device__ __forceinline__ f3 brdf_eval(const Shading& sh, f3 l)  // brdfs.glsl:10-38
{
    const float n_dot_light = dot3(sh.normal, l);
    const float n_dot_view = sh.lambert_out;
    if (fmin_(n_dot_light, n_dot_view) < 0.0f) return mk3(0.0f, 0.0f, 0.0f);

    const f3 half_vector = normalize3(l + sh.out_dir);
    const float half_dot_view = dot3(half_vector, sh.out_dir);

    const float f90 = (half_dot_view * half_dot_view) * (2.0f * sh.roughness) + 0.5f;
    const float diffuse_fresnel = mix_(1.0f, f90, schlick_factor(n_dot_view)) * mix_(1.0f, f90, schlick_factor(n_dot_light));
    f3 r = mk3(diffuse_fresnel * sh.diffuse_albedo.x, diffuse_fresnel * sh.diffuse_albedo.y,
               diffuse_fresnel * sh.diffuse_albedo.z);

    const float half_dot_normal = dot3(half_vector, sh.normal);
    const float roughness_sq = sh.roughness * sh.roughness;
    const float denominator = half_dot_normal * (roughness_sq - 1.0f) + 1.0f;  // un-squared n.h, as the reference
    const float distribution = roughness_sq / (denominator * denominator);

    const float masking = n_dot_light * __builtin_sqrtf((n_dot_view - roughness_sq * n_dot_view) * n_dot_view + roughness_sq);
    const float shadowing =
        n_dot_view * __builtin_sqrtf((n_dot_light - roughness_sq * n_dot_light) * n_dot_light + roughness_sq);
    const float geometry = 0.5f / (masking + shadowing);

    const float ff = schlick_factor(fmax_(0.0f, half_dot_view));
    const f3 spec_f = mk3(mix_(sh.fresnel_0.x, 1.0f, ff), mix_(sh.fresnel_0.y, 1.0f, ff), mix_(sh.fresnel_0.z, 1.0f, ff));
    const float dg = distribution * geometry;
    r = r + mk3(dg * spec_f.x, dg * spec_f.y, dg * spec_f.z);
    return r / JPT_PI;
}

__device__ __forceinline__ float diffuse_probability(const Shading& sh)  // brdfs.glsl:107-110
{
    return fmin_(0.5f, dot3(sh.diffuse_albedo, mk3(0.2126f, 0.7152f, 0.0722f)));
}

__device__ __forceinline__ f3 sample_brdf(const Shading& sh, float xi0, float xi1)  // brdfs.glsl:112-128
{
    // get_shading_space (brdfs.glsl:83-93)
    const f3 nrm = sh.normal;
    const float sign = nrm.z > 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + nrm.z);
    const float b = nrm.x * nrm.y * a;
    const f3 c0 = mk3(1.0f + sign * nrm.x * nrm.x * a, sign * b, -sign * nrm.x);
    const f3 c1 = mk3(b, sign + nrm.y * nrm.y * a, -nrm.y);
    const f3 c2 = nrm;

    const float diffuse_prob = diffuse_probability(sh);
    // The two strategies share their azimuth: sin / cos of 2 pi xi0' with xi0' rescaled per strategy.  The lanes of a wave
    // choose at random, so a wave runs both sides of the branch; the 60-instruction sincos_ is kept out of it.
    const bool diffuse = xi0 < diffuse_prob;
    if (diffuse) xi0 = xi0 / diffuse_prob;
    else xi0 = (xi0 - diffuse_prob) / (1.0f - diffuse_prob);
    float sp, cp;
    sincos_((2.0f * JPT_PI) * xi0, sp, cp);
    f3 local;
    if (diffuse) {
        // sample_hemisphere_psa (brdfs.glsl:95-101)
        const float radius = __builtin_sqrtf(xi1);
        const float z = __builtin_sqrtf(1.0f - radius * radius);
        local = mk3(radius * cp, radius * sp, z);
    } else {
        const f3 view = mk3(dot3(c0, sh.out_dir), dot3(c1, sh.out_dir), dot3(c2, sh.out_dir));
        // sample_ggx_vndf (brdfs.glsl:40-54), roughness = vec2(r)
        const float rg = sh.roughness;
        const f3 tv = normalize3(mk3(view.x * rg, view.y * rg, view.z));
        const float z = 1.0f - xi1 * (1.0f + tv.z);
        const float sin_theta = __builtin_sqrtf(fmax_(0.0f, 1.0f - z * z));
        const f3 hs = mk3(sin_theta * cp, sin_theta * sp, z);
        const f3 sum = hs + tv;
        const f3 h = normalize3(mk3(sum.x * rg, sum.y * rg, sum.z));
        // sample_ggx_in_dir: -reflect(view, h) (brdfs.glsl:69-72)
        const float k = 2.0f * dot3(h, view);
        local = -(view - h * k);
    }
    return mk3(c0.x * local.x + c1.x * local.y + c2.x * local.z, c0.y * local.x + c1.y * local.y + c2.y * local.z,
               c0.z * local.x + c1.z * local.y + c2.z * local.z);
}

__device__ __forceinline__ float brdf_density(const Shading& sh, f3 l)  // brdfs.glsl:130-138, :74-81, :56-67, :103-105
{
    const float diffuse_prob = diffuse_probability(sh);
    const f3 half_vector = normalize3(l + sh.out_dir);
    const float half_dot_view = dot3(half_vector, sh.out_dir);
    const float half_dot_normal = dot3(half_vector, sh.normal);
    float vndf = 0.0f;
    if (!(half_dot_normal < 0.0f)) {
        const float n_dot_view = sh.lambert_out;
        const float roughness_sq = sh.roughness * sh.roughness;
        const float inv_roughness_sq = 1.0f - roughness_sq;
        const float denominator = n_dot_view + __builtin_sqrtf(roughness_sq + inv_roughness_sq * n_dot_view * n_dot_view);
        const float d_vis = fmax_(0.0f, half_dot_view) * (2.0f / JPT_PI) / denominator;
        const float m_sq_term = 1.0f - inv_roughness_sq * half_dot_normal * half_dot_normal;
        vndf = d_vis * roughness_sq / (m_sq_term * m_sq_term);
    }
    const float specular_density = vndf / (4.0f * half_dot_view);
    const float diffuse_density = fmax_(0.0f, dot3(sh.normal, l)) / JPT_PI;
    return mix_(specular_density, diffuse_density, diffuse_prob);
}

// One path vertex after a hit (main.glsl:381-394).  Returns false when the path ends
// (lambert_in <= 0); otherwise `ray` is the next segment and `throughput` is updated.
__device__ __forceinline__ bool bounce_step(const Shading& s, uint32_t& sx, uint32_t& sy, Ray& ray, f3& throughput)
{
    ray.o = s.position + s.normal * 0.001f;
    float xi0, xi1;
    pcg2d(sx, sy, xi0, xi1);
    ray.d = sample_brdf(s, xi0, xi1);
    ray.rD = rcp3(ray.d);
    const float density = brdf_density(s, ray.d);
    const float lambert_in = dot3(s.normal, ray.d);
    if (lambert_in <= 0.0f) return false;
    const f3 f = (brdf_eval(s, ray.d) * lambert_in) / density;
    throughput = throughput * f;
    return true;
}

// ---- next-event estimation of the map (JPT_ENV_SAMPLING_MIS) ----------------------------------------------------------------
//
// bounce_step with the BRDF density of the sampled direction handed out: the MIS weight of the next vertex's miss needs it
__device__ __forceinline__ bool bounce_step_pdf(const Shading& s, uint32_t& sx, uint32_t& sy, Ray& ray, f3& throughput, float& density)
{
    ray.o = s.position + s.normal * 0.001f;
    float xi0, xi1;
    pcg2d(sx, sy, xi0, xi1);
    ray.d = sample_brdf(s, xi0, xi1);
    ray.rD = rcp3(ray.d);
    density = brdf_density(s, ray.d);
    const float lambert_in = dot3(s.normal, ray.d);
    if (lambert_in <= 0.0f) return false;
    const f3 f = (brdf_eval(s, ray.d) * lambert_in) / density;
    throughput = throughput * f;
    return true;
}
// The map sample of a path vertex: its randoms come from a COPY of the vertex's seeds (taken before bounce_step draws), hashed by
// one pcg2d round of (sx ^ 0x68bc21eb, sy ^ 0x02e5be93) -- the path's own sequence does not advance.  True when a shadow ray
// is to be cast from s.position + s.normal * 0.001 along `l`: n.l > 0 and a non-zero contribution, which is then
//     ((throughput * (brdf_eval(l) * n.l)) * L_env(l)) * (w_env / p_env),   w_env = p_env^2 / (p_env^2 + p_brdf(l)^2).
__device__ __forceinline__ bool env_nee(const Shading& s, const EnvDev& e, const EnvSampDev& es, uint32_t sx, uint32_t sy, f3 throughput,
                                        f3& l, f3& contrib)
{
    uint32_t hx = sx ^ 0x68bc21ebu, hy = sy ^ 0x02e5be93u;
    float xi0, xi1;
    pcg2d(hx, hy, xi0, xi1);
    float pe;
    l = env_sample(e, es, xi0, xi1, pe);
    if (!(pe > 0.0f)) return false;
    const float ndl = dot3(s.normal, l);
    if (!(ndl > 0.0f)) return false;
    const float pb = brdf_density(s, l);
    const float w = (pe * pe) / (pe * pe + pb * pb);
    contrib = ((throughput * (brdf_eval(s, l) * ndl)) * env_radiance(e, l)) * (w / pe);
    return contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f;
}
// the weight of a BRDF-sampled miss at bounce >= 1 (p_brdf: the previous vertex's density of d): p_brdf^2 / (p_brdf^2 + p_env(d)^2)
__device__ __forceinline__ float env_miss_weight(const EnvDev& e, const EnvSampDev& es, f3 d, float p_brdf)
{
    const float pe = env_pdf(e, es, d);
    if (!(pe > 0.0f)) return 1.0f;
    return (p_brdf * p_brdf) / (p_brdf * p_brdf + pe * pe);
}

// ---- next-event estimation of the emissive triangles (JPT_LIGHT_SAMPLING_MIS) -------------------------------------------------
//
// One emitter and a point on it from four randoms: the block by xi0 on the marginal CDF, the emitter by xi1 on its block's
// conditional CDF (both clamped below 1, first entry > xi), then with s = sqrt(xi2) the point y = (P0 + E1 * (s * (1 - xi3)))
// + E2 * (s * xi3), uniform on the world triangle.
struct LightSample {
    f3 y, e1, e2, le;
};
__device__ __forceinline__ LightSample light_sample(const LightDev& lt, float xi0, float xi1, float xi2, float xi3)
{
    xi0 = xi0 < 0.99999994f ? xi0 : 0.99999994f;
    xi1 = xi1 < 0.99999994f ? xi1 : 0.99999994f;
    const uint32_t b = (uint32_t)env_upper_bound(lt.marg, (int32_t)lt.n_blocks, xi0);
    const uint32_t first = b * kLightBlock;
    const uint32_t cnt = lt.n - first < kLightBlock ? lt.n - first : kLightBlock;
    const uint32_t k = first + (uint32_t)env_upper_bound(lt.cdf + first, (int32_t)cnt, xi1);
    const float4 q0 = lt.tri[3 * (size_t)k], q1 = lt.tri[3 * (size_t)k + 1], q2 = lt.tri[3 * (size_t)k + 2];
    LightSample ls;
    ls.e1 = mk3(q1.x, q1.y, q1.z);
    ls.e2 = mk3(q2.x, q2.y, q2.z);
    ls.le = mk3(q0.w, q1.w, q2.w);
    const float s = __builtin_sqrtf(xi2);
    ls.y = (mk3(q0.x, q0.y, q0.z) + ls.e1 * (s * (1.0f - xi3))) + ls.e2 * (s * xi3);
    return ls;
}
// |cos| between the emitter's geometric normal normalize(E1 x E2) and l (emission is two-sided)
__device__ __forceinline__ float light_cos(f3 e1, f3 e2, f3 l) { return __builtin_fabsf(dot3(normalize3(cross3(e1, e2)), l)); }
// The density per unit solid angle of the point the sampler drew, seen at squared distance d2 under light_cos c:
//     p_L = (lum(Le) * d2) / (total * c)      (the area cancels: power / total picks the emitter, 1 / area the point)
__device__ __forceinline__ float light_pdf(f3 le, float total, float d2, float c) { return (light_lum(le.x, le.y, le.z) * d2) / (total * c); }

constexpr float kLightShadowScale = 0.9999f;   // tmax = |y - o| * (1 - 1e-4): the shadow ray stops short of the emitter

// The emitter sample of a path vertex: randoms from a COPY of the vertex's seeds hashed by two pcg2d rounds of (sx ^ 0x2c1b3c6d,
// sy ^ 0x297a2d39) -- the path's own sequence does not advance.  o = position + normal * 0.001, l = normalize(y - o), d2 =
// |y - o|^2.  True when a shadow ray (o, l, tmax = sqrt(d2) * kLightShadowScale) is to be cast: n.l > 0, light_cos > 0, and a
// contribution that is finite with a component > 0:
//     ((throughput * (brdf_eval(l) * n.l)) * Le) * (w_L / p_L),   w_L = p_L^2 / (p_L^2 + p_brdf(l)^2).
__device__ __forceinline__ bool light_nee(const Shading& s, const LightDev& lt, float total, uint32_t sx, uint32_t sy, f3 throughput,
                                          f3& o, f3& l, float& tmax, f3& contrib)
{
    uint32_t hx = sx ^ 0x2c1b3c6du, hy = sy ^ 0x297a2d39u;
    float xi0, xi1, xi2, xi3;
    pcg2d(hx, hy, xi0, xi1);
    pcg2d(hx, hy, xi2, xi3);
    const LightSample ls = light_sample(lt, xi0, xi1, xi2, xi3);
    o = s.position + s.normal * 0.001f;
    const f3 dv = ls.y - o;
    const float d2 = dot3(dv, dv);
    l = normalize3(dv);
    const float ndl = dot3(s.normal, l);
    if (!(ndl > 0.0f)) return false;
    const float c = light_cos(ls.e1, ls.e2, l);
    if (!(c > 0.0f)) return false;
    const float pl = light_pdf(ls.le, total, d2, c);
    const float pb = brdf_density(s, l);
    const float w = (pl * pl) / (pl * pl + pb * pb);
    contrib = ((throughput * (brdf_eval(s, l) * ndl)) * ls.le) * (w / pl);
    if (!__builtin_isfinite(contrib.x) || !__builtin_isfinite(contrib.y) || !__builtin_isfinite(contrib.z)) return false;
    tmax = __builtin_sqrtf(d2) * kLightShadowScale;
    return contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f;
}
// The weight of the emission a BRDF-sampled ray (origin o, direction d) at bounce >= 1 finds at a hit: 1 unless lum(Le) > 0 and
// total > 0, else p_brdf^2 / (p_brdf^2 + p_L^2) with p_L of the hit point (d2 = |position - o|^2, the hit triangle's world edges
// xform_dir(transform, e1 / e2)); a NaN weight (both densities infinite) is 1.  p_brdf: read only then.
__device__ __forceinline__ float light_hit_weight(const LightDev& lt, float total, const SceneShading& sh, const Hit& h, const Shading& s,
                                                 f3 o, f3 d, const float* p_brdf)
{
    if (!(light_lum(s.emission.x, s.emission.y, s.emission.z) > 0.0f) || !(total > 0.0f)) return 1.0f;
    const WideTri& w = lt.wtris[h.tri];
    const RefInstance& b = sh.instances[h.inst];
    const f3 e1 = xform_dir(b.transform, mk3(w.e1[0], w.e1[1], w.e1[2])), e2 = xform_dir(b.transform, mk3(w.e2[0], w.e2[1], w.e2[2]));
    const f3 dv = s.position - o;
    const float pl = light_pdf(s.emission, total, dot3(dv, dv), light_cos(e1, e2, d));
    const float pb = *p_brdf;
    const float wt = (pb * pb) / (pb * pb + pl * pl);
    return wt == wt ? wt : 1.0f;
}

// ---- the transmission lobe (JPT_MATERIAL_EXT_TRANSMISSION, the *_tx kernels) ---------------------------------------------------
//
// What the lobe reads of the hit's material beside the Shading record: the tint (albedo times its texture, as get_shading_data
// forms it) and the two extension words, sanitised.  The lookup and the texture fetch are get_shading_data's own, written again
// so that its source stays what the other kernel families compile; after inlining the compiler keeps one copy of each.
struct MaterialExt {
    f3 tint;
    float transmission, ior;
};
template <int TEX = 3>
__device__ __forceinline__ MaterialExt material_ext(const SceneShading& sc, const Hit& h, const ShadeTriRegs& tr)
{
    const float4 q2 = tr.q2, q3 = tr.q3;
    const uint32_t slot = __float_as_uint(q3.w);
    const unsigned long long word = (unsigned long long)h.inst * 44ull + 41ull + (unsigned long long)slot;
    uint32_t mat_id = word < (unsigned long long)sc.n_instances * 44ull ? reinterpret_cast<const uint32_t*>(sc.instances)[word] : 0u;
    if (mat_id >= sc.n_materials) mat_id = 0;
    const RefMaterial& material = sc.materials[mat_id];
    const float u = h.u, v = h.v;
    const float w0 = 1.0f - u - v;
    f3 albedo = mk3(material.albedo.x, material.albedo.y, material.albedo.z);
    if (material.albedo_texture_index >= 0) {
        const float uvx = q2.y * w0 + q2.w * u + q3.y * v;
        const float uvy = q2.z * w0 + q3.x * u + q3.z * v;
        albedo = albedo * (TEX == 0 ? mk3(0.0f, 0.0f, 0.0f) : sample_texture<(TEX == 3 ? 0 : TEX)>(sc, uvx, uvy, material.albedo_texture_index));
    }
    return MaterialExt{albedo, material_transmission(material.padding[0]), material_ior(material.padding[1])};
}

// The lobe choice and, when it falls on the lobe, the dielectric vertex.  (xi_t, xi_f): one pcg2d round of a COPY of the vertex's
// seeds hashed as (sx ^ 0x5bd1e995, sy ^ 0x1b873593) -- constants of its own, the path's sequence does not advance.  xi_t >=
// transmission: false, nothing is touched: the vertex is the opaque one (NEE, bounce_step).  Otherwise true: `ray` is the next
// segment (dielectric_event; origin position + normal * 0.001 when reflected, - when refracted), a refracted path's throughput
// is tinted, and the path's own draw for this vertex is taken and discarded: one sequence position per vertex either way.
// The lanes of a wave choose at random: the hashed draw, the tint (fetched with the shading record) and the offset origin are
// made outside the branch on the event.
__device__ __forceinline__ bool transmission_step(const Shading& s, const MaterialExt& me, bool front, uint32_t& sx, uint32_t& sy, Ray& ray,
                                                  f3& throughput)
{
    uint32_t hx = sx ^ 0x5bd1e995u, hy = sy ^ 0x1b873593u;
    float xi_t, xi_f;
    pcg2d(hx, hy, xi_t, xi_f);
    if (!(xi_t < me.transmission)) return false;
    f3 d;
    float fresnel;
    const int event = dielectric_event(s.normal, s.out_dir, me.ior, front, xi_f, d, fresnel);
    const bool refracted = event == 0;
    ray.o = s.position + s.normal * (refracted ? -0.001f : 0.001f);
    ray.d = d;
    ray.rD = rcp3(d);
    const f3 tinted = throughput * me.tint;
    if (refracted) throughput = tinted;
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    return true;
}
// env_miss_weight / light_hit_weight behind a vertex that may have been a dielectric one: its sentinel density means weight 1
__device__ __forceinline__ float env_miss_weight_tx(const EnvDev& e, const EnvSampDev& es, f3 d, float p_brdf)
{
    if (p_brdf == kDeltaDensity) return 1.0f;
    return env_miss_weight(e, es, d, p_brdf);
}
__device__ __forceinline__ float light_hit_weight_tx(const LightDev& lt, float total, const SceneShading& sh, const Hit& h, const Shading& s,
                                                    f3 o, f3 d, const float* p_brdf)
{
    if (!(light_lum(s.emission.x, s.emission.y, s.emission.z) > 0.0f) || !(total > 0.0f)) return 1.0f;
    if (*p_brdf == kDeltaDensity) return 1.0f;
    return light_hit_weight(lt, total, sh, h, s, o, d, p_brdf);
}

__device__ __forceinline__ f3 aces_film(f3 x)  // progressive_rendering.glsl:19-26
{
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    return mk3(clamp_((x.x * (a * x.x + b)) / (x.x * (c * x.x + d) + e), 0.0f, 1.0f),
               clamp_((x.y * (a * x.y + b)) / (x.y * (c * x.y + d) + e), 0.0f, 1.0f),
               clamp_((x.z * (a * x.z + b)) / (x.z * (c * x.z + d) + e), 0.0f, 1.0f));
}

#endif  // __HIPCC__

}  // namespace jpt
