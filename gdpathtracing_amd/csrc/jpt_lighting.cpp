// jpt_lighting.cpp -- what a context's renders see at their misses and sample with shadow rays: the environment map and its sampling
// tables, the emitter list and its tables (LightingState, jpt_ctx.h), the one resolver that turns them into a render's Lighting
// (jpt_kernels.h), and the C entries that set or probe them -- jpt_set_sky and its debug forms among them: the map of a procedural sky
// (jpt_sky.h) made on the device.  Host C++: the kernels are jpt_kernels_post.hip's, jpt_kernels_sky.hip's and jpt_debug.hip's.
#include "jpt_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// The emitters of c->scene.ref, instance-major, each instance's triangles (the leaves under its BLAS root, each triangle once) in
// ascending index: those whose Le (light_emission) has lum(Le) > 0.  True when there is one.
bool light_candidates(jpt_ctx* c)
{
    LightingState& l = c->lighting;
    if (!l.light_cand_stale) return !l.light_cand_h.empty();
    const RefScene& r = c->scene.ref;
    l.light_cand_h.clear();
    l.light_cand_stale = false;
    l.light_cand_uploaded = false;
    if (r.materials.empty()) return false;
    std::vector<uint32_t> tris, stack;
    std::vector<char> emits(r.materials.size(), 0);
    bool any = false;
    for (size_t m = 0; m < r.materials.size(); m++) {   // (a scene none of whose materials emits has no emitter: no walk)
        const Vec4& e = r.materials[m].emission;
        const float em = e.w > 0.0f ? e.w : 0.0f;
        emits[m] = light_lum(e.x * em, e.y * em, e.z * em) > 0.0f;
        any = any || emits[m];
    }
    if (!any) return false;
    const uint32_t n_inst = (uint32_t)r.instances.size(), n_nodes = (uint32_t)r.bvh_nodes.size();
    uint32_t cached_root = 0xffffffffu;
    for (uint32_t i = 0; i < n_inst; i++) {
        const uint32_t root = r.instances[i].blas_index;
        if (root != cached_root) {
            tris.clear();
            stack.assign(1, root);
            size_t visits = 0;
            while (!stack.empty() && visits++ <= n_nodes) {
                const uint32_t k = stack.back();
                stack.pop_back();
                if (k >= n_nodes) continue;
                const RefBvhNode& nd = r.bvh_nodes[k];
                if (nd.tri_count > 0) {
                    for (uint32_t t = 0; t < nd.tri_count; t++)
                        if ((size_t)nd.first_tri_index + t < r.tri_data.size()) tris.push_back(nd.first_tri_index + t);
                } else {
                    stack.push_back(nd.right_child);
                    stack.push_back(nd.left_child);
                }
            }
            std::sort(tris.begin(), tris.end());
            tris.erase(std::unique(tris.begin(), tris.end()), tris.end());
            cached_root = root;
        }
        for (const uint32_t t : tris) {
            float le[3];
            light_emission(r.instances.data(), n_inst, r.materials.data(), (uint32_t)r.materials.size(), i, r.tri_data[t].material_index, le);
            if (light_lum(le[0], le[1], le[2]) > 0.0f) {
                l.light_cand_h.push_back(i);
                l.light_cand_h.push_back(t);
            }
        }
    }
    return !l.light_cand_h.empty();
}

// The emitter tables, built on the context's stream when stale: after every render queued so far (each ends with work there), so
// no render in flight reads them while they change; the next render of every slot waits for the context's stream.
int ensure_light_tables(jpt_ctx* c)
{
    LightingState& l = c->lighting;
    if (!l.light_table_stale && l.light_cand_uploaded) return JPT_OK;
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)(l.light_cand_h.size() / 2), nb = (n + kLightBlock - 1) / kLightBlock;
    if (l.d_light_tri.n != 3 * (size_t)n || l.d_light_marg.n != (size_t)nb + 1 || !l.light_cand_uploaded)
        HIP_TRY(c, hipStreamSynchronize(s));   // (buffers of another size: renders in flight may read the old ones)
    if (!l.light_cand_uploaded) {
        HIP_TRY(c, l.d_light_cand.upload(l.light_cand_h, s));
        l.light_cand_uploaded = true;
    }
    HIP_TRY(c, l.d_light_tri.resize(3 * (size_t)n));
    HIP_TRY(c, l.d_light_cdf.resize(n));
    HIP_TRY(c, l.d_light_marg.resize((size_t)nb + 1));
    LightBuildArgs a;
    a.cand = l.d_light_cand.p;
    a.n = n;
    a.n_blocks = nb;
    a.instances = c->ds.ref_instances;
    a.n_instances = c->ds.n_instances;
    a.n_materials = c->ds.n_materials;
    a.materials = c->ds.ref_materials;
    a.wtris = c->ds.wide_tris;
    a.shade = c->ds.shade_tris;
    a.tri = l.d_light_tri.p;
    a.cdf = l.d_light_cdf.p;
    a.marg = l.d_light_marg.p;
    launch_light_tables(s, a);
    HIP_TRY(c, hipGetLastError());
    c->pipe.workspaces_touched();
    l.light_table_stale = false;
    return JPT_OK;
}

// the emitter tables as the kernels take them (ensure_light_tables makes them current)
LightDev light_tables_view(const jpt_ctx* c)
{
    const LightingState& l = c->lighting;
    const uint32_t n = (uint32_t)(l.light_cand_h.size() / 2);
    return LightDev{l.d_light_tri.p, l.d_light_cdf.p, l.d_light_marg.p, c->ds.wide_tris, n, (n + kLightBlock - 1) / kLightBlock};
}

}  // namespace

namespace jpt {

void lights_stale(jpt_ctx* c, bool listed)
{
    c->lighting.light_table_stale = true;
    if (!listed) return;
    c->lighting.light_cand_stale = true;
    bool any = false;
    for (const RefMaterial& m : c->scene.ref.materials) any = any || material_transmission(m.padding[0]) > 0.0f;
    c->lighting.transmissive_materials = any;
}

Lighting lighting_bound(const jpt_ctx* c)
{
    const LightingState& l = c->lighting;
    Lighting lg;
    if (c->debug_steps) return lg;   // (DEBUG_STEPS counts the audit kernel's steps: its render sees no light)
    // (a black map's MIS render is the BRDF-mode render -- no map samples, every weight 1: the *_env kernels)
    const bool mis = l.env_set && l.env_sampling == JPT_ENV_SAMPLING_MIS && l.env_tables && l.env_total > 0.0f;
    const bool emitters = l.light_sampling == JPT_LIGHT_SAMPLING_MIS && c->device >= 0 && c->scene.device_ready && (l.light_cand_stale || !l.light_cand_h.empty());
    lg.env_mode = mis ? 2 : (l.env_set ? 1 : 0);
    lg.kind = emitters ? Lighting::kEmitters : (mis ? Lighting::kMapMis : (l.env_set ? Lighting::kMap : Lighting::kSky));
    // (the extension words are read only when the flag says so AND some material then transmits: otherwise today's kernels)
    lg.transmissive = (l.material_ext & JPT_MATERIAL_EXT_TRANSMISSION) != 0u && l.transmissive_materials && c->device >= 0 && c->scene.device_ready;
    return lg;
}

int resolve_lighting(jpt_ctx* c, Lighting& lg)
{
    const LightingState& l = c->lighting;
    if (lighting_bound(c).kind == Lighting::kEmitters) (void)light_candidates(c);   // the emitter list, if stale: the bound is then exact
    lg = lighting_bound(c);
    if (lg.env_mode != 0) {
        lg.env = EnvDev{l.d_env.p, l.env_w, l.env_h, {}, l.env_intensity};
        std::memcpy(lg.env.rot, l.env_rot, sizeof lg.env.rot);
    }
    if (lg.env_mode == 2) lg.samp = EnvSampDev{l.d_env_cond.p, l.d_env_marg.p, l.env_total};
    if (lg.kind == Lighting::kEmitters) {
        const int rc = ensure_light_tables(c);   // (on the context's stream, before the render)
        if (rc != JPT_OK) return rc;
        lg.lights = light_tables_view(c);
    }
    return JPT_OK;
}

int check_env_map(const float* rgb, int32_t width, int32_t height, std::string& why)
{
    if (width <= 0 || height <= 0) {
        why = "jpt_set_environment: width and height must be positive";
        return JPT_E_INVALID;
    }
    if (width > kEnvMaxWidth || height > kEnvMaxHeight) {
        why = "jpt_set_environment: the map is larger than 16384 x 8192 texels";
        return JPT_E_LIMIT;
    }
    const size_t n = (size_t)width * (size_t)height * 3u;
    for (size_t i = 0; i < n; i++) {
        const float v = rgb[i];
        if (!(v >= 0.0f) || !std::isfinite(v)) {
            why = "jpt_set_environment: texel value " + std::to_string(i) + " is negative, infinite or NaN";
            return JPT_E_INVALID;
        }
    }
    return JPT_OK;
}

int check_env_params(const float* rotation9, float intensity, std::string& why)
{
    if (rotation9)
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(rotation9[k])) {
                why = "jpt_set_environment_params: the rotation has a non-finite entry";
                return JPT_E_INVALID;
            }
    if (!std::isfinite(intensity) || !(intensity >= 0.0f)) {
        why = "jpt_set_environment_params: the intensity must be finite and >= 0";
        return JPT_E_INVALID;
    }
    return JPT_OK;
}

bool env_rotation_orthonormal(const float* r)
{
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double d = (double)r[3 * a] * r[3 * b] + (double)r[3 * a + 1] * r[3 * b + 1] + (double)r[3 * a + 2] * r[3 * b + 2];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= kEnvOrthoTol)) return false;
        }
    return true;
}

// ---- the procedural sky (jpt_set_sky; the arithmetic: jpt_sky.h) ----

void jpt_sky_default_params(jpt_sky_params& p)
{
    std::memset(&p, 0, sizeof p);
    const float top[3] = {0.385f, 0.454f, 0.55f}, horizon[3] = {0.6463f, 0.6558f, 0.6708f}, bottom[3] = {0.2f, 0.169f, 0.133f};
    for (int k = 0; k < 3; k++) {
        p.sky_top_color[k] = top[k];
        p.sky_horizon_color[k] = horizon[k];
        p.ground_bottom_color[k] = bottom[k];
        p.ground_horizon_color[k] = horizon[k];
    }
    p.sky_curve = 0.15f;
    p.ground_curve = 0.02f;
    p.sun_curve = 0.15f;
    p.sky_energy = p.ground_energy = p.exposure = 1.0f;
    p.sun_angle_max = (float)(30.0 * 3.14159265358979323846 / 180.0);
    p.n_suns = 0;
}

int sky_size_check(int32_t width, int32_t height, int32_t samples, std::string& why)
{
    if (width <= 0 || height <= 0) {
        why = "jpt_set_sky: width and height must be positive";
        return JPT_E_INVALID;
    }
    if (samples < 1 || samples > kSkyMaxSamples) {
        why = "jpt_set_sky: samples must lie in 1..8";
        return JPT_E_INVALID;
    }
    if (width > kEnvMaxWidth || height > kEnvMaxHeight) {
        why = "jpt_set_sky: the map is larger than 16384 x 8192 texels";
        return JPT_E_LIMIT;
    }
    return JPT_OK;
}

int sky_params_dev(const jpt_sky_params* params, SkyDev& out, std::string& why)
{
    jpt_sky_params p;
    if (params) p = *params;
    else jpt_sky_default_params(p);
    auto bad = [&why](const std::string& field, const char* rule) {
        why = "jpt_set_sky: " + field + " " + rule;
        return JPT_E_INVALID;
    };
    auto level = [](float v) { return std::isfinite(v) && v >= 0.0f; };
    const struct { const char* name; const float* v; } colours[4] = {{"sky_top_color", p.sky_top_color}, {"sky_horizon_color", p.sky_horizon_color},
        {"ground_bottom_color", p.ground_bottom_color}, {"ground_horizon_color", p.ground_horizon_color}};
    for (const auto& c : colours)
        for (int k = 0; k < 3; k++)
            if (!level(c.v[k])) return bad(c.name, "must be finite and >= 0");
    const struct { const char* name; float v; } levels[3] = {{"sky_energy", p.sky_energy}, {"ground_energy", p.ground_energy}, {"exposure", p.exposure}};
    for (const auto& e : levels)
        if (!level(e.v)) return bad(e.name, "must be finite and >= 0");
    const struct { const char* name; float v; } curves[3] = {{"sky_curve", p.sky_curve}, {"ground_curve", p.ground_curve}, {"sun_curve", p.sun_curve}};
    for (const auto& c : curves)
        if (!(c.v >= 0.015625f && c.v <= 8.0f)) return bad(c.name, "must lie in [1/64, 8]");
    if (!(p.sun_angle_max >= 0.0f && p.sun_angle_max <= kSkyPi)) return bad("sun_angle_max", "must lie in [0, pi]");
    if (p.n_suns < 0 || p.n_suns > kSkyMaxSuns) return bad("n_suns", "must lie in 0..4");
    SkyDev d;
    std::memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; k++) {
        d.sky_top[k] = p.sky_top_color[k];
        d.sky_horizon[k] = p.sky_horizon_color[k];
        d.ground_bottom[k] = p.ground_bottom_color[k];
        d.ground_horizon[k] = p.ground_horizon_color[k];
    }
    d.sky_energy = p.sky_energy;
    d.ground_energy = p.ground_energy;
    d.exposure = p.exposure;
    d.inv_sky_curve = 1.0f / p.sky_curve;
    d.inv_ground_curve = 1.0f / p.ground_curve;
    d.inv_sun_curve = 1.0f / p.sun_curve;
    d.n_suns = p.n_suns;
    for (int s = 0; s < p.n_suns; s++) {
        const jpt_sky_sun& in = p.suns[s];
        const std::string name = "suns[" + std::to_string(s) + "].";
        const double x = in.direction[0], y = in.direction[1], z = in.direction[2];
        const double len = std::sqrt(x * x + y * y + z * z);
        if (!std::isfinite(in.direction[0]) || !std::isfinite(in.direction[1]) || !std::isfinite(in.direction[2]) || !(len > 0.0))
            return bad(name + "direction", "must be finite and non-zero");
        if (!(in.angular_radius > 0.0f && in.angular_radius <= kSkyHalfPi)) return bad(name + "angular_radius", "must lie in (0, pi/2]");
        for (int k = 0; k < 3; k++)
            if (!level(in.color[k])) return bad(name + "color", "must be finite and >= 0");
        if (!level(in.energy)) return bad(name + "energy", "must be finite and >= 0");
        if (in.mode != JPT_SUN_RADIANCE && in.mode != JPT_SUN_IRRADIANCE) return bad(name + "mode", "must be JPT_SUN_RADIANCE or JPT_SUN_IRRADIANCE");
        SkySunDev& o = d.suns[s];
        o.dir[0] = (float)(x / len);
        o.dir[1] = (float)(y / len);
        o.dir[2] = (float)(z / len);
        o.r = in.angular_radius;
        o.amax = p.sun_angle_max > o.r ? p.sun_angle_max : o.r;
        const float span = o.amax - o.r;
        o.inv_span = span > 0.0f ? 1.0f / span : 0.0f;
        // the cap's solid angle in double: 2 pi (1 - cos r)
        const double cap = 2.0 * 3.14159265358979323846 * (1.0 - std::cos((double)o.r));
        for (int k = 0; k < 3; k++) {
            o.rad[k] = in.mode == JPT_SUN_IRRADIANCE ? (float)((double)in.color[k] * (double)in.energy / cap) : in.color[k] * in.energy;
            if (!std::isfinite(o.rad[k])) return bad(name + "color", "times energy overflows the disk's radiance");
        }
    }
    out = d;
    return JPT_OK;
}

void pack_env_texels(const float* rgb, int32_t width, int32_t height, std::vector<float4>& out)
{
    const size_t n = (size_t)width * (size_t)height;
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
}

}  // namespace jpt

extern "C" {

// the emitter tables for the jpt_debug_light_* entries, whatever the mode: made if stale; out.n == 0 when the scene has no emitter
static int debug_lights(jpt_ctx* c, LightDev& out)
{
    out = LightDev{};
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: the emitter tables are on the device");
    if (!c->scene.device_ready) return fail(c, JPT_E_STATE, "no scene");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!light_candidates(c)) return JPT_OK;
    const int rc = ensure_light_tables(c);
    if (rc != JPT_OK) return rc;
    out = light_tables_view(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return JPT_OK;
}

int jpt_debug_light_tables(jpt_ctx* c, uint32_t capacity, uint32_t* n_out, uint32_t* pairs_out, float* tri_out, float* cdf_out, float* marg_out)
{
    if (!c || !n_out) return JPT_E_INVALID;
    LightDev lt;
    const int rc = debug_lights(c, lt);
    if (rc != JPT_OK) return rc;
    n_out[0] = lt.n;
    n_out[1] = lt.n_blocks;
    if (lt.n == 0 || capacity < lt.n) return JPT_OK;
    if (pairs_out) std::memcpy(pairs_out, c->lighting.light_cand_h.data(), (size_t)lt.n * 2 * sizeof(uint32_t));
    if (tri_out) HIP_TRY(c, hipMemcpy(tri_out, lt.tri, (size_t)lt.n * 3 * sizeof(float4), hipMemcpyDeviceToHost));
    if (cdf_out) HIP_TRY(c, hipMemcpy(cdf_out, lt.cdf, (size_t)lt.n * sizeof(float), hipMemcpyDeviceToHost));
    if (marg_out) HIP_TRY(c, hipMemcpy(marg_out, lt.marg, ((size_t)lt.n_blocks + 1) * sizeof(float), hipMemcpyDeviceToHost));
    return JPT_OK;
}

static int light_probe_call(jpt_ctx* c, int what, const float* xi4, const uint32_t* inst, const uint32_t* tri, const float* points3,
                            const float* origins3, const float* dirs3, uint32_t n, float* points_out, float* dirs_out, float* pdf_out)
{
    if (!c) return JPT_E_INVALID;
    if (n && (!origins3 || !pdf_out || (what == 1 && (!xi4 || !points_out || !dirs_out)) || (what == 2 && (!inst || !tri || !points3 || !dirs3))))
        return fail(c, JPT_E_INVALID, "null argument");
    LightDev lt;
    const int rc = debug_lights(c, lt);
    if (rc != JPT_OK) return rc;
    if (n == 0) return JPT_OK;
    if (lt.n == 0) {   // no emitter: density 0 (and no sample)
        for (uint32_t i = 0; i < n; i++) pdf_out[i] = 0.0f;
        if (what == 1) {
            std::memset(points_out, 0, (size_t)n * 3 * sizeof(float));
            std::memset(dirs_out, 0, (size_t)n * 3 * sizeof(float));
        }
        return JPT_OK;
    }
    if (what == 2)
        for (uint32_t i = 0; i < n; i++)
            if (inst[i] >= c->ds.n_instances || tri[i] >= c->ds.n_tris) return fail(c, JPT_E_INVALID, "no such instance or triangle");
    const size_t n3 = (size_t)n * 3;
    DevBuf<float> d_in, d_o, d_d, d_p, d_po, d_do, d_pdf;
    DevBuf<uint32_t> d_inst, d_tri;
    HIP_TRY(c, d_o.resize(n3));
    HIP_TRY(c, d_pdf.resize(n));
    HIP_TRY(c, hipMemcpy(d_o.p, origins3, n3 * sizeof(float), hipMemcpyHostToDevice));
    if (what == 1) {
        HIP_TRY(c, d_in.resize((size_t)n * 4));
        HIP_TRY(c, d_po.resize(n3));
        HIP_TRY(c, d_do.resize(n3));
        HIP_TRY(c, hipMemcpy(d_in.p, xi4, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice));
    } else {
        HIP_TRY(c, d_d.resize(n3));
        HIP_TRY(c, d_p.resize(n3));
        HIP_TRY(c, d_inst.resize(n));
        HIP_TRY(c, d_tri.resize(n));
        HIP_TRY(c, hipMemcpy(d_d.p, dirs3, n3 * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_p.p, points3, n3 * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_inst.p, inst, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_tri.p, tri, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    launch_light_probe(c->stream, lt, c->ds.shading(), what, d_in.p, d_o.p, d_d.p, d_p.p, d_inst.p, d_tri.p, n, d_po.p, d_do.p, d_pdf.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(pdf_out, d_pdf.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (what == 1) {
        HIP_TRY(c, hipMemcpy(points_out, d_po.p, n3 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(dirs_out, d_do.p, n3 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return JPT_OK;
}

int jpt_debug_light_sample(jpt_ctx* c, const float* xi4, const float* origins3, uint32_t n, float* points_out, float* dirs_out, float* pdf_out)
{
    return light_probe_call(c, 1, xi4, nullptr, nullptr, nullptr, origins3, nullptr, n, points_out, dirs_out, pdf_out);
}

int jpt_debug_light_pdf(jpt_ctx* c, const uint32_t* inst, const uint32_t* tri, const float* points3, const float* origins3, const float* dirs3,
                        uint32_t n, float* pdf_out)
{
    return light_probe_call(c, 2, nullptr, inst, tri, points3, origins3, dirs3, n, nullptr, nullptr, pdf_out);
}

// the sampling tables of the context's map, on its stream (after the renders queued there: none of them reads the tables), and the
// total weight read back -- the one wait of jpt_set_environment_sampling
static int build_env_tables(jpt_ctx* c)
{
    LightingState& l = c->lighting;
    const size_t w = (size_t)l.env_w, h = (size_t)l.env_h;
    HIP_TRY(c, l.d_env_cond.resize(w * h));
    HIP_TRY(c, l.d_env_marg.resize(h + 1));
    launch_env_tables(c->stream, l.d_env.p, l.env_w, l.env_h, l.d_env_cond.p, l.d_env_marg.p, l.d_env_marg.p + h);
    HIP_TRY(c, hipGetLastError());
    float total = 0.0f;
    HIP_TRY(c, hipMemcpyAsync(&total, l.d_env_marg.p + h, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    l.env_total = total;
    l.env_tables = true;
    return JPT_OK;
}

int jpt_set_environment(jpt_ctx* c, const float* rgb, int32_t width, int32_t height)
{
    if (!c) return JPT_E_INVALID;
    LightingState& l = c->lighting;
    std::string why;
    if (rgb) {
        const int rc = check_env_map(rgb, width, height, why);
        if (rc != JPT_OK) return fail(c, rc, why);
    }
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no environment map");
    HIP_TRY(c, hipSetDevice(c->device));
    // the renders already queued read the old map: they finish first (every one of them ends with work on the context's stream)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    l.env_tables = false;
    l.d_env_cond.release();
    l.d_env_marg.release();
    if (!rgb) {
        l.env_set = false;
        l.d_env.release();
        return JPT_OK;
    }
    std::vector<float4> texels;
    pack_env_texels(rgb, width, height, texels);
    l.env_set = false;
    HIP_TRY(c, l.d_env.resize(texels.size()));
    HIP_TRY(c, hipMemcpy(l.d_env.p, texels.data(), texels.size() * sizeof(float4), hipMemcpyHostToDevice));
    l.env_w = width;
    l.env_h = height;
    l.env_set = true;
    if (l.env_sampling == JPT_ENV_SAMPLING_MIS) return build_env_tables(c);
    return JPT_OK;
}

void jpt_sky_defaults(jpt_sky_params* out)
{
    if (out) jpt_sky_default_params(*out);
}

// The map of a procedural sky, written into d_env by the kernel.  A map of this size already there (made by either call): queued on the
// context's stream -- behind every render queued so far, each of which ends with work there -- and the next render of every slot waits
// for that stream (as ensure_light_tables orders its build): no wait on the host.  Otherwise as jpt_set_environment: wait, allocate.
int jpt_set_sky(jpt_ctx* c, const jpt_sky_params* params, int32_t width, int32_t height, int32_t samples)
{
    if (!c) return JPT_E_INVALID;
    LightingState& l = c->lighting;
    std::string why;
    SkyDev P;
    int rc = sky_params_dev(params, P, why);
    if (rc == JPT_OK) rc = sky_size_check(width, height, samples, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_sky: host-only context has no environment map");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * (size_t)height;
    if (!(l.env_set && l.env_w == width && l.env_h == height && l.d_env.n == n)) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (renders in flight read the old buffer)
        l.env_set = false;
        l.d_env_cond.release();
        l.d_env_marg.release();
        HIP_TRY(c, l.d_env.resize(n));
        l.env_w = width;
        l.env_h = height;
    }
    l.env_tables = false;   // (the tables' buffers stay: a rebuild of the same size reuses them, on this stream)
    launch_sky(c->stream, P, width, height, samples, l.d_env.p);
    HIP_TRY(c, hipGetLastError());
    c->pipe.workspaces_touched();
    l.env_set = true;
    if (l.env_sampling == JPT_ENV_SAMPLING_MIS) return build_env_tables(c);
    return JPT_OK;
}

int jpt_read_environment_f32(jpt_ctx* c, float* rgb, int32_t* width, int32_t* height)
{
    if (!c) return JPT_E_INVALID;
    const LightingState& l = c->lighting;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_environment_f32: host-only context has no environment map");
    if (!l.env_set) return fail(c, JPT_E_STATE, "jpt_read_environment_f32: no environment map");
    if (width) *width = l.env_w;
    if (height) *height = l.env_h;
    if (!rgb) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)l.env_w * (size_t)l.env_h, kChunk = (size_t)1 << 20;
    std::vector<float4> part(std::min(n, kChunk));
    for (size_t at = 0; at < n; at += kChunk) {
        const size_t m = std::min(kChunk, n - at);
        HIP_TRY(c, hipMemcpy(part.data(), l.d_env.p + at, m * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++) {
            rgb[3 * (at + i)] = part[i].x;
            rgb[3 * (at + i) + 1] = part[i].y;
            rgb[3 * (at + i) + 2] = part[i].z;
        }
    }
    return JPT_OK;
}

int jpt_debug_sky(int device_id, const jpt_sky_params* params, int32_t width, int32_t height, int32_t samples, float* rgb_out)
{
    std::string why;
    SkyDev P;
    int rc = sky_params_dev(params, P, why);
    if (rc == JPT_OK) rc = sky_size_check(width, height, samples, why);
    if (rc == JPT_OK && !rgb_out) {
        why = "jpt_debug_sky: null argument";
        rc = JPT_E_INVALID;
    }
    if (rc != JPT_OK) {
        set_debug_error(why);
        return rc;
    }
    const size_t n = (size_t)width * (size_t)height;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        for (int32_t j = 0; j < height; j++)
            for (int32_t i = 0; i < width; i++) {
                const f3 t = sky_texel(P, width, height, samples, i, j);
                float* o = rgb_out + 3 * ((size_t)j * (size_t)width + (size_t)i);
                o[0] = t.x;
                o[1] = t.y;
                o[2] = t.z;
            }
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        set_debug_error(std::string(what) + ": " + hipGetErrorString(e));
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    float4* d_map = nullptr;
    if ((e = hipMalloc((void**)&d_map, n * sizeof(float4))) != hipSuccess) return hip_fail(e, "hipMalloc");
    std::vector<float4> texels(n);
    launch_sky(nullptr, P, width, height, samples, d_map);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "sky_kernel");
    if (rc == JPT_OK && (e = hipMemcpy(texels.data(), d_map, n * sizeof(float4), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_map);
    if (rc != JPT_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        rgb_out[3 * i] = texels[i].x;
        rgb_out[3 * i + 1] = texels[i].y;
        rgb_out[3 * i + 2] = texels[i].z;
    }
    return JPT_OK;
}

int jpt_debug_sky_radiance(const jpt_sky_params* params, const float* dirs3, uint32_t n, float* rgb_out)
{
    std::string why;
    SkyDev P;
    int rc = sky_params_dev(params, P, why);
    if (rc == JPT_OK && n && (!dirs3 || !rgb_out)) {
        why = "jpt_debug_sky_radiance: null argument";
        rc = JPT_E_INVALID;
    }
    if (rc != JPT_OK) {
        set_debug_error(why);
        return rc;
    }
    for (uint32_t i = 0; i < n; i++) {
        const f3 d = mk3(dirs3[3 * (size_t)i], dirs3[3 * (size_t)i + 1], dirs3[3 * (size_t)i + 2]);
        const float theta = atan2_(__builtin_sqrtf(d.x * d.x + d.z * d.z), d.y);
        const f3 c = sky_radiance(P, theta, d);
        rgb_out[3 * (size_t)i] = c.x;
        rgb_out[3 * (size_t)i + 1] = c.y;
        rgb_out[3 * (size_t)i + 2] = c.z;
    }
    return JPT_OK;
}

int jpt_debug_pow01(const float* b, const float* e, uint32_t n, float* out)
{
    if (n && (!b || !e || !out)) {
        set_debug_error("jpt_debug_pow01: null argument");
        return JPT_E_INVALID;
    }
    for (uint32_t i = 0; i < n; i++) out[i] = pow01_(b[i], e[i]);
    return JPT_OK;
}

int jpt_set_environment_sampling(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    LightingState& l = c->lighting;
    if (mode != JPT_ENV_SAMPLING_BRDF && mode != JPT_ENV_SAMPLING_MIS) return fail(c, JPT_E_INVALID, "jpt_set_environment_sampling: unknown mode");
    if (mode == JPT_ENV_SAMPLING_MIS && !env_rotation_orthonormal(l.env_rot))
        return fail(c, JPT_E_INVALID, "jpt_set_environment_sampling: the map sampler needs an orthonormal rotation (jpt_set_environment_params)");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no environment map");
    l.env_sampling = mode;
    if (mode == JPT_ENV_SAMPLING_MIS && l.env_set && !l.env_tables) {
        HIP_TRY(c, hipSetDevice(c->device));
        return build_env_tables(c);
    }
    return JPT_OK;
}

int jpt_set_light_sampling(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_LIGHT_SAMPLING_BRDF && mode != JPT_LIGHT_SAMPLING_MIS) return fail(c, JPT_E_INVALID, "jpt_set_light_sampling: unknown mode");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: light sampling runs on the device");
    c->lighting.light_sampling = mode;   // (the tables are made at the first render that samples them)
    return JPT_OK;
}

int jpt_set_material_extensions(jpt_ctx* c, uint32_t flags)
{
    if (!c) return JPT_E_INVALID;
    if ((flags & ~(uint32_t)JPT_MATERIAL_EXT_TRANSMISSION) != 0u) return fail(c, JPT_E_INVALID, "jpt_set_material_extensions: unknown flag");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: material extensions are read on the device");
    c->lighting.material_ext = flags;   // (whether a render takes the *_tx kernels: lighting_bound, from this and the materials)
    return JPT_OK;
}

int jpt_set_environment_params(jpt_ctx* c, const float* rotation9, float intensity)
{
    if (!c) return JPT_E_INVALID;
    LightingState& l = c->lighting;
    std::string why;
    const int rc = check_env_params(rotation9, intensity, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (l.env_sampling == JPT_ENV_SAMPLING_MIS && rotation9 && !env_rotation_orthonormal(rotation9))
        return fail(c, JPT_E_INVALID, "jpt_set_environment_params: with JPT_ENV_SAMPLING_MIS the rotation must be orthonormal");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no environment map");
    static const float kIdentity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    std::memcpy(l.env_rot, rotation9 ? rotation9 : kIdentity, sizeof l.env_rot);
    l.env_intensity = intensity;
    return JPT_OK;
}

}  // extern "C"
