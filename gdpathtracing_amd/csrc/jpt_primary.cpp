// jpt_primary.cpp -- where a context's renders start their paths: the thin lens, the camera model, the bake images, the probes and the reflection probes (PrimaryState,
// jpt_ctx.h), the one resolver that turns them into a render's PrimaryRays (jpt_kernels.h), the view of the entry points that take
// one without rendering, and the C entries that set them.  Host C++: the kernels are jpt_kernels_bake.hip's and jpt_debug.hip's.
#include "jpt_ctx.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jpt_instance_math.h"

int jpt::check_lens(float aperture_radius, float focus_distance, std::string& why)
{
    if (!std::isfinite(aperture_radius) || aperture_radius < 0.0f) {
        why = "jpt_set_lens: aperture_radius must be finite and >= 0";
        return JPT_E_INVALID;
    }
    if (aperture_radius > 0.0f && (!std::isfinite(focus_distance) || !(focus_distance > 0.0f))) {
        why = "jpt_set_lens: focus_distance must be finite and > 0";
        return JPT_E_INVALID;
    }
    if (!std::isfinite(focus_distance) || focus_distance < 0.0f) {   // (not read with radius 0, but never kept as garbage)
        why = "jpt_set_lens: focus_distance must be finite and > 0";
        return JPT_E_INVALID;
    }
    return JPT_OK;
}

static_assert(JPT_CAMERA_PINHOLE == kCamPinhole && JPT_CAMERA_PROJECTIVE == kCamProjective && JPT_CAMERA_EQUIRECT == kCamEquirect,
              "jpt_camera.h restates the enum of jpt.h");

int jpt::make_camera_model(int32_t model, const RefCamera& cam, CamModelDev& out, std::string& why)
{
    out = CamModelDev{};
    if (model != JPT_CAMERA_PINHOLE && model != JPT_CAMERA_PROJECTIVE && model != JPT_CAMERA_EQUIRECT) {
        why = "jpt_set_camera_model: model must be JPT_CAMERA_PINHOLE, JPT_CAMERA_PROJECTIVE or JPT_CAMERA_EQUIRECT";
        return JPT_E_INVALID;
    }
    if (model == JPT_CAMERA_EQUIRECT) {
        LensDev basis;
        if (!lens_basis(cam, basis)) {
            why = "jpt_set_camera_model: the camera basis derived from camera160 (ivp, position) is not finite";
            return JPT_E_STATE;
        }
        out.f = basis.f;
        out.r = basis.r;
        out.u = basis.u;
    }
    if (model == JPT_CAMERA_PROJECTIVE)
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(cam.ivp[k])) {
                why = "jpt_set_camera_model: the ivp of camera160 is not finite";
                return JPT_E_STATE;
            }
    out.model = model;
    return JPT_OK;
}

// One decision, in this order: DEBUG_STEPS, the reflection probes, the bake images, the probes, the lens, the model.  The sources exclude one another, and a
// refusal names the first of them in that order: a bake render with a lens is refused as a bake and not for the lens's own reasons,
// and probes beside bake images are refused (or rendered) as a bake.  Reflection probes beside bake images or probes are refused:
// neither image layout is the other's.
int jpt::resolve_primary(jpt_ctx* c, PrimaryRays& out)
{
    const PrimaryState& p = c->primary;
    out = PrimaryRays{};
    if (c->debug_steps) return JPT_OK;   // (DEBUG_STEPS ignores the images, the lens and the model, as it ignores lighting)
    const bool lens = p.lens_radius > 0.0f, model = p.camera_model != JPT_CAMERA_PINHOLE, temporal = c->denoise == JPT_DENOISE_TEMPORAL;
    if (p.has_cubes()) {
        if (p.has_bake())
            return fail(c, JPT_E_STATE, "the context holds reflection probes and bake images: free one of them (jpt_set_reflection_probes, jpt_set_bake_texels)");
        if (p.has_probes()) return fail(c, JPT_E_STATE, "the context holds reflection probes and light probes: free one of them (jpt_set_reflection_probes, jpt_set_probes)");
        if (p.cube_w != c->width || p.cube_h != c->height)
            return fail(c, JPT_E_STATE, "the reflection probes' strips make an image of " + std::to_string(p.cube_w) + " x " + std::to_string(p.cube_h) +
                                            " pixels but jpt_set_params says " + std::to_string(c->width) + " x " + std::to_string(c->height) +
                                            ": a cube render has one path per face texel (jpt_set_reflection_probes)");
        if (lens) return fail(c, JPT_E_STATE, "a cube render has no lens: set the lens radius to 0 (jpt_set_lens) or free the reflection probes (jpt_set_reflection_probes)");
        if (model)
            return fail(c, JPT_E_STATE, "a cube render has no camera model: set JPT_CAMERA_PINHOLE (jpt_set_camera_model) or free the reflection probes (jpt_set_reflection_probes)");
        if (temporal) return fail(c, JPT_E_STATE, "temporal reprojection assumes a camera: set another denoising mode or free the reflection probes (jpt_set_reflection_probes)");
        out.kind = PrimaryRays::kCube;
        out.cube = p.cube_dev();
    } else if (p.has_bake()) {
        if (p.bake_w != c->width || p.bake_h != c->height)
            return fail(c, JPT_E_STATE, "the bake images are " + std::to_string(p.bake_w) + " x " + std::to_string(p.bake_h) + " texels but jpt_set_params says " +
                                            std::to_string(c->width) + " x " + std::to_string(c->height) + ": a bake render has one path per texel (jpt_set_bake_texels)");
        if (lens) return fail(c, JPT_E_STATE, "a bake render has no lens: set the lens radius to 0 (jpt_set_lens) or free the bake images (jpt_set_bake_texels)");
        if (model)
            return fail(c, JPT_E_STATE, "a bake render has no camera model: set JPT_CAMERA_PINHOLE (jpt_set_camera_model) or free the bake images (jpt_set_bake_texels)");
        if (temporal) return fail(c, JPT_E_STATE, "temporal reprojection assumes a camera: set another denoising mode or free the bake images (jpt_set_bake_texels)");
        out.kind = PrimaryRays::kBake;
        out.bake.position = p.d_bake_pos.p;
        out.bake.normal = p.d_bake_nrm.p;
    } else if (p.has_probes()) {
        if (p.probe_w != c->width || p.probe_h != c->height)
            return fail(c, JPT_E_STATE, "the probe tiles make an image of " + std::to_string(p.probe_w) + " x " + std::to_string(p.probe_h) + " pixels but jpt_set_params says " +
                                            std::to_string(c->width) + " x " + std::to_string(c->height) + ": a probe render has one path per tile cell (jpt_set_probes)");
        if (lens) return fail(c, JPT_E_STATE, "a probe render has no lens: set the lens radius to 0 (jpt_set_lens) or free the probes (jpt_set_probes)");
        if (model) return fail(c, JPT_E_STATE, "a probe render has no camera model: set JPT_CAMERA_PINHOLE (jpt_set_camera_model) or free the probes (jpt_set_probes)");
        if (temporal) return fail(c, JPT_E_STATE, "temporal reprojection assumes a camera: set another denoising mode or free the probes (jpt_set_probes)");
        out.kind = PrimaryRays::kProbe;
        out.probe = p.probe_dev();
    } else if (lens) {
        if (temporal)
            return fail(c, JPT_E_STATE, "temporal reprojection assumes one centre of projection: set the lens radius to 0 (jpt_set_lens) or another denoising mode");
        LensDev l;
        l.radius = p.lens_radius;
        l.focus = p.lens_focus;
        if (!lens_basis(c->camera, l)) return fail(c, JPT_E_STATE, "jpt_set_lens: the camera basis derived from camera160 (ivp, position) is not finite");
        if (model)
            return fail(c, JPT_E_STATE, "the lens disk is defined around one centre of projection: set the lens radius to 0 (jpt_set_lens) or JPT_CAMERA_PINHOLE (jpt_set_camera_model)");
        out.kind = PrimaryRays::kLens;
        out.lens = l;
    } else if (model) {
        if (temporal) return fail(c, JPT_E_STATE, "temporal reprojection assumes the pinhole: set JPT_CAMERA_PINHOLE (jpt_set_camera_model) or another denoising mode");
        std::string why;
        const int rc = make_camera_model(p.camera_model, c->camera, out.cam_model, why);
        if (rc != JPT_OK) return fail(c, rc, why);
        out.kind = PrimaryRays::kCamModel;
    }
    return JPT_OK;
}

int jpt::view_now(jpt_ctx* c, const char* call, const char* rays, CamModelDev& out)
{
    if (c->primary.has_bake())
        return fail(c, JPT_E_STATE, std::string(call) + ": " + rays + " are camera rays, and the context holds bake images (jpt_set_bake_texels)");
    if (c->primary.has_probes()) return fail(c, JPT_E_STATE, std::string(call) + ": " + rays + " are camera rays, and the context holds probes (jpt_set_probes)");
    if (c->primary.has_cubes())
        return fail(c, JPT_E_STATE, std::string(call) + ": " + rays + " are camera rays, and the context holds reflection probes (jpt_set_reflection_probes)");
    std::string why;
    const int rc = make_camera_model(c->primary.camera_model, c->camera, out, why);
    return rc == JPT_OK ? JPT_OK : fail(c, rc, why);
}

// ---- the checks of the bake entry points, also run by the jpt_debug_bake_* ones -------------------------------------------------

int jpt::check_bake_size(const char* call, int32_t width, int32_t height, std::string& why)
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

int jpt::check_bake_texels(const char* call, const float* position4, const float* normal4, size_t n, std::string& why)
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

int jpt::check_bake_surface(const char* call, const float* vertices, const float* normals, const int32_t* indices, int32_t n_vertices, int32_t n_indices,
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

// ---- the checks of jpt_set_probes, also run by the jpt_debug_probe_* entry points, and the quadrature table -------------------------

int jpt::check_probes(const char* call, const float* position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    if (tile_w < kProbeTileWMin || tile_w > kProbeTileWMax) {
        why = who + "tile_w must be in [4, 64]";
        return JPT_E_INVALID;
    }
    if (tile_h < kProbeTileHMin || tile_h > kProbeTileHMax) {
        why = who + "tile_h must be in [2, 32]";
        return JPT_E_INVALID;
    }
    if (tile_w * tile_h > kProbeMaxCells) {
        why = who + "tile_w * tile_h must be at most 1024";
        return JPT_E_INVALID;
    }
    if (n_probes < 1 || n_probes > kProbeMaxProbes) {
        why = who + "n_probes must be in [1, 2^20]";
        return JPT_E_LIMIT;
    }
    if (probes_per_row < 1) {
        why = who + "probes_per_row must be >= 1";
        return JPT_E_INVALID;
    }
    uint64_t w, h;
    probe_image_size(n_probes, tile_w, tile_h, probes_per_row, w, h);
    if (w > kProbeMaxPixels || w * h > kProbeMaxPixels) {
        why = who + "the image of the tiles has more than 2^26 pixels";
        return JPT_E_LIMIT;
    }
    if (position3)
        for (size_t k = 0; k < 3 * (size_t)n_probes; k++)
            if (!std::isfinite(position3[k])) {
                why = who + "probe " + std::to_string(k / 3) + " has a non-finite position component";
                return JPT_E_INVALID;
            }
    return JPT_OK;
}

// Cell means of the basis of jpt_probe.h: with z the polar coordinate (world y), r = sqrt(1 - z^2) and phi the map's azimuth the nine
// functions are k0; k1 r sin; k1 z; k1 r cos; k2 r^2 sin 2phi / 2; k2 z r sin; k3 (3 z^2 - 1); k2 z r cos; k4 r^2 cos 2phi -- a product
// of a mean over the cell's z interval and one over its phi interval, each an antiderivative's difference over the interval's length.
void jpt::probe_basis_table(int32_t tile_w, int32_t tile_h, int32_t flags, std::vector<float>& out)
{
    const double pi = 3.14159265358979323846;
    const double k0 = 0.28209479177387814, k1 = 0.4886025119029199, k2 = 1.0925484305920792, k3 = 0.31539156525252005, k4 = 0.5462742152960396;
    const int cells = tile_w * tile_h;
    std::vector<double> mz(tile_h), mz2(tile_h), mr(tile_h), mzr(tile_h), mr2(tile_h), ms(tile_w), mc(tile_w), ms2(tile_w), mc2(tile_w);
    auto fr = [](double z) {
        const double q = 1.0 - z * z, r = std::sqrt(q > 0.0 ? q : 0.0);
        return 0.5 * (z * r + std::asin(z < -1.0 ? -1.0 : (z > 1.0 ? 1.0 : z)));
    };
    auto fzr = [](double z) {
        const double q = 1.0 - z * z, qq = q > 0.0 ? q : 0.0;
        return -(qq * std::sqrt(qq)) / 3.0;
    };
    for (int j = 0; j < tile_h; j++) {
        const double z0 = 1.0 - 2.0 * (double)j / (double)tile_h, z1 = 1.0 - 2.0 * (double)(j + 1) / (double)tile_h, dz = z0 - z1;
        mz[j] = (z0 * z0 / 2.0 - z1 * z1 / 2.0) / dz;
        mz2[j] = (z0 * z0 * z0 / 3.0 - z1 * z1 * z1 / 3.0) / dz;
        mr[j] = (fr(z0) - fr(z1)) / dz;
        mzr[j] = (fzr(z0) - fzr(z1)) / dz;
        mr2[j] = 1.0 - mz2[j];
    }
    for (int i = 0; i < tile_w; i++) {
        const double p0 = ((double)i / (double)tile_w - 0.5) * 2.0 * pi, p1 = ((double)(i + 1) / (double)tile_w - 0.5) * 2.0 * pi, dp = p1 - p0;
        ms[i] = (-std::cos(p1) - -std::cos(p0)) / dp;
        mc[i] = (std::sin(p1) - std::sin(p0)) / dp;
        ms2[i] = (-std::cos(2.0 * p1) / 2.0 - -std::cos(2.0 * p0) / 2.0) / dp;
        mc2[i] = (std::sin(2.0 * p1) / 2.0 - std::sin(2.0 * p0) / 2.0) / dp;
    }
    std::vector<double> y((size_t)cells * 9);
    double gram[9] = {};
    const double w = 4.0 * pi / (double)cells;
    for (int j = 0; j < tile_h; j++)
        for (int i = 0; i < tile_w; i++) {
            double* t = &y[((size_t)j * tile_w + i) * 9];
            t[0] = k0;
            t[1] = k1 * (mr[j] * ms[i]);
            t[2] = k1 * mz[j];
            t[3] = k1 * (mr[j] * mc[i]);
            t[4] = k2 * (mr2[j] * (ms2[i] * 0.5));
            t[5] = k2 * (mzr[j] * ms[i]);
            t[6] = k3 * (3.0 * mz2[j] - 1.0);
            t[7] = k2 * (mzr[j] * mc[i]);
            t[8] = k4 * (mr2[j] * mc2[i]);
        }
    for (int c = 0; c < cells; c++)
        for (int k = 0; k < 9; k++) gram[k] += w * (y[(size_t)c * 9 + k] * y[(size_t)c * 9 + k]);
    const double band[3] = {pi, 2.0 * pi / 3.0, pi / 4.0};
    out.resize((size_t)cells * 9);
    for (int c = 0; c < cells; c++)
        for (int k = 0; k < 9; k++) {
            // A function whose cell means all vanish on this grid cannot be resolved by it, and its column is zero: Y6 with tile_h = 2
            // (the mean of z^2 over either half is 1/3) and Y8 with tile_w = 4 (the mean of cos 2 phi over a quarter turn is 0) -- G_kk
            // is then 0 or rounding noise (~ 1e-34) against 0.2 .. 1 for every column a grid resolves (kProbeGramMin, jpt_probe.h)
            double v = gram[k] < kProbeGramMin ? 0.0 : w * y[(size_t)c * 9 + k] / gram[k];
            if (flags & JPT_PROBE_IRRADIANCE) v = v * band[k == 0 ? 0 : (k < 4 ? 1 : 2)];
            out[(size_t)c * 9 + k] = (float)v;
        }
}

// ---- the checks of jpt_set_reflection_probes / jpt_set_reflection_params, also run by the debug entry points, and the sample tables ----

int jpt::check_reflection_probes(const char* call, const float* position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    if (face_size < kCubeFaceMin || face_size > kCubeFaceMax || (face_size & (face_size - 1)) != 0) {
        why = who + "face_size must be a power of two in [4, 256]";
        return JPT_E_INVALID;
    }
    if (n_probes < 1 || n_probes > kCubeMaxProbes) {
        why = who + "n_probes must be in [1, 2^20]";
        return JPT_E_LIMIT;
    }
    if (probes_per_row < 1) {
        why = who + "probes_per_row must be >= 1";
        return JPT_E_INVALID;
    }
    uint64_t w, h;
    cube_image_size(n_probes, face_size, probes_per_row, w, h);
    if (w > kCubeMaxPixels || w * h > kCubeMaxPixels) {
        why = who + "the image of the strips has more than 2^26 pixels";
        return JPT_E_LIMIT;
    }
    if (position3)
        for (size_t k = 0; k < 3 * (size_t)n_probes; k++)
            if (!std::isfinite(position3[k])) {
                why = who + "probe " + std::to_string(k / 3) + " has a non-finite position component";
                return JPT_E_INVALID;
            }
    return JPT_OK;
}

int jpt::check_reflection_params(const char* call, int32_t n_levels, int32_t samples, int32_t face_size, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    const int32_t most = face_size ? cube_log2(face_size) + 1 : kReflLevelsMax;
    if (n_levels != 0 && (n_levels < kReflLevelsMin || n_levels > most)) {
        why = who + "n_levels must be 0 (every level down to 1 x 1) or in [2, " + std::to_string(most) + "]" +
              (face_size ? ": log2(face_size) + 1 of the face size " + std::to_string(face_size) : "");
        return JPT_E_INVALID;
    }
    if (samples < kReflSamplesMin || samples > kReflSamplesMax) {
        why = who + "samples must be in [8, 256]";
        return JPT_E_INVALID;
    }
    return JPT_OK;
}

// The construction of jpt_reflection.h, in double; an entry is rounded to float once.
void jpt::reflection_sample_table(int32_t face_size, int32_t n_levels, int32_t samples, std::vector<float4>& table, std::vector<uint8_t>& levels,
                                  uint32_t count[kReflLevelsMax])
{
    const double pi = 3.14159265358979323846;
    const int K = samples, top = cube_log2(face_size);
    table.assign((size_t)n_levels * K, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    levels.assign((size_t)n_levels * K, kReflNoSample);
    for (int l = 0; l < kReflLevelsMax; l++) count[l] = 0;
    const double omega0 = 4.0 * pi / (6.0 * (double)face_size * (double)face_size);
    std::vector<double> lx(K), ly(K), lz(K);
    std::vector<int> lv(K);
    for (int l = 1; l < n_levels; l++) {
        const double alpha = (double)l / (double)(n_levels - 1), a2 = alpha * alpha;
        double sum = 0.0;
        for (int k = 0; k < K; k++) {
            const double u1 = ((double)k + 0.5) / (double)K;
            double u2 = 0.0, digit = 0.5;
            for (int b = k; b; b >>= 1, digit *= 0.5)
                if (b & 1) u2 += digit;
            const double ct = std::sqrt((1.0 - u1) / (1.0 + (a2 - 1.0) * u1));
            const double st = std::sqrt(1.0 - ct * ct);
            const double phi = 2.0 * pi * u2;
            const double hx = st * std::cos(phi), hy = st * std::sin(phi), hz = ct;
            lx[k] = 2.0 * hz * hx;
            ly[k] = 2.0 * hz * hy;
            lz[k] = 2.0 * hz * hz - 1.0;
            const double den = hz * hz * (a2 - 1.0) + 1.0;
            const double ndf = a2 / (pi * den * den);
            const double omega_s = 4.0 / ((double)K * ndf);
            double m = std::floor(0.5 * std::log2(omega_s / omega0) + 0.5) + 1.0;
            m = m < 0.0 ? 0.0 : (m > (double)top ? (double)top : m);
            lv[k] = (int)m;
            if (lz[k] > 0.0) sum += lz[k];
        }
        uint32_t kept = 0;
        for (int k = 0; k < K; k++) {
            if (!(lz[k] > 0.0)) continue;
            table[(size_t)l * K + kept] = make_float4((float)lx[k], (float)ly[k], (float)lz[k], (float)(lz[k] / sum));
            levels[(size_t)l * K + kept] = (uint8_t)lv[k];
            kept++;
        }
        count[l] = kept;
    }
}

namespace {

// the renders (and a jpt_bake_finish) already queued read the old images: they finish first (every one of them ends with work on the
// context's stream); jpt_bake_finish's own images go with them
int bake_wait(jpt_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->post.lightmap_release();   // (every caller goes on to write the images: a jpt_bake_finish of the old ones is no longer the lightmap)
    return JPT_OK;
}

void bake_release(jpt_ctx* c)
{
    PrimaryState& p = c->primary;
    p.d_bake_pos.release();
    p.d_bake_nrm.release();
    p.d_bake_winner.release();
    p.d_bake_in.release();
    p.bake_w = p.bake_h = 0;
    c->post.bake_dir_release();   // (jpt_set_bake_directional's planes exist only beside the images; every caller has waited: bake_wait)
}

int bake_alloc(jpt_ctx* c, int32_t width, int32_t height)
{
    const size_t n = (size_t)width * (size_t)height;
    hipError_t e = c->primary.d_bake_pos.resize(n);
    if (e == hipSuccess) e = c->primary.d_bake_nrm.resize(n);
    if (e != hipSuccess) {
        bake_release(c);
        return hip_fail(c, e, "hipMalloc of the bake images");
    }
    c->primary.bake_w = width;
    c->primary.bake_h = height;
    return JPT_OK;
}

}  // namespace

extern "C" {

int jpt_set_lens(jpt_ctx* c, float aperture_radius, float focus_distance)
{
    if (!c) return JPT_E_INVALID;
    std::string why;
    const int rc = check_lens(aperture_radius, focus_distance, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: the lens is a property of device renders");
    c->primary.lens_radius = aperture_radius;   // (each render takes them by value: resolve_primary)
    c->primary.lens_focus = focus_distance;
    return JPT_OK;
}

int jpt_set_camera_model(jpt_ctx* c, int32_t model)
{
    if (!c) return JPT_E_INVALID;
    if (model != JPT_CAMERA_PINHOLE && model != JPT_CAMERA_PROJECTIVE && model != JPT_CAMERA_EQUIRECT)
        return fail(c, JPT_E_INVALID, "jpt_set_camera_model: model must be JPT_CAMERA_PINHOLE, JPT_CAMERA_PROJECTIVE or JPT_CAMERA_EQUIRECT");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: the camera model is a property of device renders");
    c->primary.camera_model = model;   // (each render takes it by value: resolve_primary)
    return JPT_OK;
}

// ---- lightmap baking: the context's texel images (jpt_bake.h) -------------------------------------------------------------------

int jpt_set_bake_texels(jpt_ctx* c, const float* position4, const float* normal4, int32_t width, int32_t height)
{
    if (!c) return JPT_E_INVALID;
    const bool freeing = !position4 && !normal4 && width == 0 && height == 0;
    if (!freeing) {
        if (!position4 || !normal4) return fail(c, JPT_E_INVALID, "jpt_set_bake_texels: position4 and normal4 are both given, or (NULL, NULL, 0, 0) frees the images");
        std::string why;
        int rc = check_bake_size("jpt_set_bake_texels", width, height, why);
        if (rc == JPT_OK) rc = check_bake_texels("jpt_set_bake_texels", position4, normal4, (size_t)width * (size_t)height, why);
        if (rc != JPT_OK) return fail(c, rc, why);
    }
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_bake_texels: host-only context has no bake images");
    int rc = bake_wait(c);
    if (rc != JPT_OK) return rc;
    if (freeing) {
        bake_release(c);
        return JPT_OK;
    }
    if ((rc = bake_alloc(c, width, height)) != JPT_OK) return rc;
    const size_t bytes = (size_t)width * (size_t)height * sizeof(float4);
    HIP_TRY(c, hipMemcpy(c->primary.d_bake_pos.p, position4, bytes, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->primary.d_bake_nrm.p, normal4, bytes, hipMemcpyHostToDevice));
    return JPT_OK;
}

int jpt_bake_begin(jpt_ctx* c, int32_t width, int32_t height)
{
    if (!c) return JPT_E_INVALID;
    std::string why;
    int rc = check_bake_size("jpt_bake_begin", width, height, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_bake_begin: host-only context has no bake images");
    if ((rc = bake_wait(c)) != JPT_OK) return rc;
    if ((rc = bake_alloc(c, width, height)) != JPT_OK) return rc;
    const size_t bytes = (size_t)width * (size_t)height * sizeof(float4);
    HIP_TRY(c, hipMemsetAsync(c->primary.d_bake_pos.p, 0, bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->primary.d_bake_nrm.p, 0, bytes, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return JPT_OK;
}

int jpt_bake_add_surface(jpt_ctx* c, const jpt_surface* surface, const float* uv2, const float* transform12)
{
    if (!c) return JPT_E_INVALID;
    if (!surface) return fail(c, JPT_E_INVALID, "jpt_bake_add_surface: null surface");
    std::string why;
    int rc = check_bake_surface("jpt_bake_add_surface", surface->vertices, surface->normals, surface->indices, surface->n_vertices, surface->n_indices, uv2,
                                transform12, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_bake_add_surface: host-only context has no bake images");
    if (!c->primary.has_bake()) return fail(c, JPT_E_STATE, "jpt_bake_add_surface: no bake images (jpt_bake_begin or jpt_set_bake_texels first)");
    if ((rc = bake_wait(c)) != JPT_OK) return rc;
    const uint32_t n_tris = (uint32_t)(surface->n_indices / 3);
    if (n_tris == 0) return JPT_OK;
    // the surface staged in one device buffer: vertices, normals, uv2, indices (each a multiple of 4 bytes)
    const size_t nv = (size_t)surface->n_vertices;
    const size_t b_v = nv * 3 * sizeof(float), b_uv = nv * 2 * sizeof(float), b_i = (size_t)n_tris * 3 * sizeof(int32_t);
    const size_t need = 2 * b_v + b_uv + b_i;
    if (c->primary.d_bake_in.n < need) HIP_TRY(c, c->primary.d_bake_in.resize(need));
    const size_t npx = (size_t)c->primary.bake_w * (size_t)c->primary.bake_h;
    if (c->primary.d_bake_winner.n < npx) HIP_TRY(c, c->primary.d_bake_winner.resize(npx));
    char* base = c->primary.d_bake_in.p;
    HIP_TRY(c, hipMemcpy(base, surface->vertices, b_v, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(base + b_v, surface->normals, b_v, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(base + 2 * b_v, uv2, b_uv, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(base + 2 * b_v + b_uv, surface->indices, b_i, hipMemcpyHostToDevice));
    BakeSurfaceDev sd;
    sd.vertices = reinterpret_cast<const float*>(base);
    sd.normals = reinterpret_cast<const float*>(base + b_v);
    sd.uv2 = reinterpret_cast<const float*>(base + 2 * b_v);
    sd.indices = reinterpret_cast<const int32_t*>(base + 2 * b_v + b_uv);
    sd.n_tris = n_tris;
    transform12_to_mat16(transform12, sd.transform);
    launch_bake_raster(c->stream, sd, c->primary.bake_w, c->primary.bake_h, c->primary.d_bake_winner.p, c->primary.d_bake_pos.p, c->primary.d_bake_nrm.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return JPT_OK;
}

int jpt_read_bake_texels(jpt_ctx* c, float* position4, float* normal4)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_bake_texels: host-only context has no bake images");
    if (!c->primary.has_bake()) return fail(c, JPT_E_STATE, "jpt_read_bake_texels: no bake images (jpt_bake_begin or jpt_set_bake_texels first)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->primary.bake_w * (size_t)c->primary.bake_h * sizeof(float4);
    float* const out[2] = {position4, normal4};
    const float4* const src[2] = {c->primary.d_bake_pos.p, c->primary.d_bake_nrm.p};
    for (int k = 0; k < 2; k++) {
        if (!out[k]) continue;
        const int rc = read_out(c, src[k], bytes, out[k]);
        if (rc != JPT_OK) return rc;
    }
    return JPT_OK;
}

// ---- light probes: the context's positions (jpt_probe.h) and their projection -------------------------------------------------------

int jpt_set_probes(jpt_ctx* c, const float* position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row)
{
    if (!c) return JPT_E_INVALID;
    const bool freeing = !position3 && n_probes == 0 && tile_w == 0 && tile_h == 0 && probes_per_row == 0;
    if (!freeing) {
        if (!position3) return fail(c, JPT_E_INVALID, "jpt_set_probes: position3 is given, or (NULL, 0, 0, 0, 0) frees the probes");
        std::string why;
        const int rc = check_probes("jpt_set_probes", position3, n_probes, tile_w, tile_h, probes_per_row, why);
        if (rc != JPT_OK) return fail(c, rc, why);
    }
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_probes: host-only context has no probes");
    // the renders (and a jpt_probe_project) already queued read the old positions: they finish first
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PrimaryState& p = c->primary;
    p.sh_valid = false;
    if (freeing) {
        p.d_probe_pos.release();
        p.d_probe_sh.release();
        p.d_probe_table.release();
        p.table_flags = -1;
        p.probe_n = p.probe_tw = p.probe_th = p.probe_per_row = p.probe_w = p.probe_h = 0;
        return JPT_OK;
    }
    const hipError_t e = p.d_probe_pos.resize(3 * (size_t)n_probes);
    if (e != hipSuccess) {
        p.probe_n = p.probe_tw = p.probe_th = p.probe_per_row = p.probe_w = p.probe_h = 0;
        return hip_fail(c, e, "hipMalloc of the probe positions");
    }
    uint64_t w, h;
    probe_image_size(n_probes, tile_w, tile_h, probes_per_row, w, h);
    p.probe_n = n_probes;
    p.probe_tw = tile_w;
    p.probe_th = tile_h;
    p.probe_per_row = probes_per_row;
    p.probe_w = (int32_t)w;
    p.probe_h = (int32_t)h;
    const hipError_t ec = hipMemcpy(p.d_probe_pos.p, position3, 3 * (size_t)n_probes * sizeof(float), hipMemcpyHostToDevice);
    if (ec != hipSuccess) {   // (no probes rather than probes at positions nobody wrote)
        p.d_probe_pos.release();
        p.probe_n = p.probe_tw = p.probe_th = p.probe_per_row = p.probe_w = p.probe_h = 0;
        return hip_fail(c, ec, "hipMemcpy of the probe positions");
    }
    return JPT_OK;
}

int jpt_get_probe_image_size(jpt_ctx* c, int32_t* width, int32_t* height)
{
    if (!c) return JPT_E_INVALID;
    if (!width || !height) return fail(c, JPT_E_INVALID, "jpt_get_probe_image_size: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_get_probe_image_size: host-only context has no probes");
    if (!c->primary.has_probes()) return fail(c, JPT_E_STATE, "jpt_get_probe_image_size: no probes (jpt_set_probes first)");
    *width = c->primary.probe_w;
    *height = c->primary.probe_h;
    return JPT_OK;
}

int jpt_read_probes(jpt_ctx* c, float* position3)
{
    if (!c) return JPT_E_INVALID;
    if (!position3) return fail(c, JPT_E_INVALID, "jpt_read_probes: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_probes: host-only context has no probes");
    if (!c->primary.has_probes()) return fail(c, JPT_E_STATE, "jpt_read_probes: no probes (jpt_set_probes first)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 3 * (size_t)c->primary.probe_n * sizeof(float);
    return read_out(c, c->primary.d_probe_pos.p, bytes, position3);
}

int jpt_probe_project(jpt_ctx* c, int32_t flags)
{
    if (!c) return JPT_E_INVALID;
    if (flags != JPT_PROBE_RADIANCE && flags != JPT_PROBE_IRRADIANCE) return fail(c, JPT_E_INVALID, "jpt_probe_project: flags must be JPT_PROBE_RADIANCE or JPT_PROBE_IRRADIANCE");
    const int rc = reads_sum(c, "jpt_probe_project", " projects the progressive accumulation", "jpt_probe_project: host-only context: it runs on the device",
                             ": the gathering context projects");
    if (rc != JPT_OK) return rc;
    PrimaryState& p = c->primary;
    if (!p.has_probes()) return fail(c, JPT_E_STATE, "jpt_probe_project: no probes (jpt_set_probes first)");
    if (p.has_cubes())
        return fail(c, JPT_E_STATE, "jpt_probe_project: the context also holds reflection probes (jpt_set_reflection_probes), and no render of it is a probe render");
    if (!c->params_set || p.probe_w != c->width || p.probe_h != c->height)
        return fail(c, JPT_E_STATE, "jpt_probe_project: the probe tiles make an image of " + std::to_string(p.probe_w) + " x " + std::to_string(p.probe_h) +
                                        " pixels but jpt_set_params says " + std::to_string(c->width) + " x " + std::to_string(c->height));
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, "jpt_probe_project: no frame accumulated since the last reset");
    HIP_TRY(c, hipSetDevice(c->device));
    if (p.table_tw != p.probe_tw || p.table_th != p.probe_th || p.table_flags != flags || !p.d_probe_table.p) {
        // (an earlier projection on the stream may still read the old table)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<float> table;
        probe_basis_table(p.probe_tw, p.probe_th, flags, table);
        p.table_flags = -1;
        HIP_TRY(c, p.d_probe_table.resize(table.size()));
        HIP_TRY(c, hipMemcpy(p.d_probe_table.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
        p.table_tw = p.probe_tw;
        p.table_th = p.probe_th;
        p.table_flags = flags;
    }
    if (p.d_probe_sh.n != 9 * (size_t)p.probe_n || !p.d_probe_sh.p) {
        p.sh_valid = false;
        HIP_TRY(c, p.d_probe_sh.resize(9 * (size_t)p.probe_n));
    }
    // On the context's stream, as jpt_bake_finish: behind the accumulation of every render queued so far, and the accumulation of every
    // later render waits for what it reads.
    launch_probe_project(c->stream, p.probe_dev(), c->image.d_accum.p, (float)c->frame_count, p.d_probe_table.p, p.d_probe_sh.p);
    HIP_TRY(c, hipGetLastError());
    p.sh_valid = true;
    return JPT_OK;
}

int jpt_read_probe_sh_f32(jpt_ctx* c, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_probe_sh_f32: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_probe_sh_f32: host-only context: jpt_probe_project runs on the device");
    if (!c->primary.sh_valid) return fail(c, JPT_E_STATE, "jpt_read_probe_sh_f32: no jpt_probe_project of the current probes and size yet");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 9 * (size_t)c->primary.probe_n * sizeof(float4);
    return read_out(c, c->primary.d_probe_sh.p, bytes, out);
}

// ---- reflection probes: the context's positions (jpt_cube.h) and their prefiltered mip chain (jpt_reflection.h) ---------------------

namespace {

void forget_cubes(PrimaryState& p)
{
    p.d_cube_pos.release();
    p.d_refl_chain.release();
    p.d_refl_out.release();
    p.d_refl_table.release();
    p.d_refl_lvl.release();
    p.table_face = p.table_levels = p.table_samples = 0;
    p.cube_n = p.cube_face = p.cube_per_row = p.cube_w = p.cube_h = 0;
    p.refl_made = 0;
}

}  // namespace

int jpt_set_reflection_probes(jpt_ctx* c, const float* position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row)
{
    if (!c) return JPT_E_INVALID;
    const bool freeing = !position3 && n_probes == 0 && face_size == 0 && probes_per_row == 0;
    if (!freeing) {
        if (!position3) return fail(c, JPT_E_INVALID, "jpt_set_reflection_probes: position3 is given, or (NULL, 0, 0, 0) frees the reflection probes");
        std::string why;
        const int rc = check_reflection_probes("jpt_set_reflection_probes", position3, n_probes, face_size, probes_per_row, why);
        if (rc != JPT_OK) return fail(c, rc, why);
    }
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_reflection_probes: host-only context has no reflection probes");
    // the renders (and a jpt_reflection_prefilter) already queued read the old positions and images: they finish first
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PrimaryState& p = c->primary;
    p.refl_valid = false;
    if (freeing) {
        forget_cubes(p);
        return JPT_OK;
    }
    const hipError_t e = p.d_cube_pos.resize(3 * (size_t)n_probes);
    if (e != hipSuccess) {
        forget_cubes(p);
        return hip_fail(c, e, "hipMalloc of the reflection probes' positions");
    }
    uint64_t w, h;
    cube_image_size(n_probes, face_size, probes_per_row, w, h);
    p.cube_n = n_probes;
    p.cube_face = face_size;
    p.cube_per_row = probes_per_row;
    p.cube_w = (int32_t)w;
    p.cube_h = (int32_t)h;
    const hipError_t ec = hipMemcpy(p.d_cube_pos.p, position3, 3 * (size_t)n_probes * sizeof(float), hipMemcpyHostToDevice);
    if (ec != hipSuccess) {   // (no probes rather than probes at positions nobody wrote)
        forget_cubes(p);
        return hip_fail(c, ec, "hipMemcpy of the reflection probes' positions");
    }
    return JPT_OK;
}

int jpt_get_reflection_image_size(jpt_ctx* c, int32_t* width, int32_t* height)
{
    if (!c) return JPT_E_INVALID;
    if (!width || !height) return fail(c, JPT_E_INVALID, "jpt_get_reflection_image_size: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_get_reflection_image_size: host-only context has no reflection probes");
    if (!c->primary.has_cubes()) return fail(c, JPT_E_STATE, "jpt_get_reflection_image_size: no reflection probes (jpt_set_reflection_probes first)");
    *width = c->primary.cube_w;
    *height = c->primary.cube_h;
    return JPT_OK;
}

int jpt_read_reflection_probes(jpt_ctx* c, float* position3)
{
    if (!c) return JPT_E_INVALID;
    if (!position3) return fail(c, JPT_E_INVALID, "jpt_read_reflection_probes: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_reflection_probes: host-only context has no reflection probes");
    if (!c->primary.has_cubes()) return fail(c, JPT_E_STATE, "jpt_read_reflection_probes: no reflection probes (jpt_set_reflection_probes first)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 3 * (size_t)c->primary.cube_n * sizeof(float);
    return read_out(c, c->primary.d_cube_pos.p, bytes, position3);
}

int jpt_set_reflection_params(jpt_ctx* c, const jpt_reflection_params* params)
{
    if (!c) return JPT_E_INVALID;
    jpt_reflection_params q;
    q.n_levels = 0;
    q.samples = kReflSamplesDefault;
    if (params) q = *params;
    std::string why;
    const int rc = check_reflection_params("jpt_set_reflection_params", q.n_levels, q.samples, c->primary.cube_face, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_reflection_params: host-only context: jpt_reflection_prefilter runs on the device");
    c->primary.refl_valid = false;   // (no jpt_reflection_prefilter with these parameters yet)
    c->primary.refl_levels = q.n_levels;
    c->primary.refl_samples = q.samples;
    return JPT_OK;
}

int jpt_reflection_prefilter(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    const int rc = reads_sum(c, "jpt_reflection_prefilter", " filters the progressive accumulation", "jpt_reflection_prefilter: host-only context: it runs on the device",
                             ": the gathering context filters");
    if (rc != JPT_OK) return rc;
    PrimaryState& p = c->primary;
    if (!p.has_cubes()) return fail(c, JPT_E_STATE, "jpt_reflection_prefilter: no reflection probes (jpt_set_reflection_probes first)");
    if (p.has_bake() || p.has_probes())
        return fail(c, JPT_E_STATE, "jpt_reflection_prefilter: the context also holds bake images or light probes, and no render of it is a cube render");
    if (!c->params_set || p.cube_w != c->width || p.cube_h != c->height)
        return fail(c, JPT_E_STATE, "jpt_reflection_prefilter: the reflection probes' strips make an image of " + std::to_string(p.cube_w) + " x " +
                                        std::to_string(p.cube_h) + " pixels but jpt_set_params says " + std::to_string(c->width) + " x " + std::to_string(c->height));
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, "jpt_reflection_prefilter: no frame accumulated since the last reset");
    if (p.refl_levels > cube_log2(p.cube_face) + 1)   // (the parameters were set before these probes: checked against no face size)
        return fail(c, JPT_E_STATE, "jpt_reflection_prefilter: n_levels is " + std::to_string(p.refl_levels) + " (jpt_set_reflection_params) but a face of " +
                                        std::to_string(p.cube_face) + " texels has " + std::to_string(cube_log2(p.cube_face) + 1) + " levels");
    HIP_TRY(c, hipSetDevice(c->device));
    const int32_t n_levels = p.refl_levels_now(), K = p.refl_samples;
    if (p.table_face != p.cube_face || p.table_levels != n_levels || p.table_samples != K || !p.d_refl_table.p) {
        // (an earlier prefilter on the stream may still read the old tables)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<float4> table;
        std::vector<uint8_t> levels;
        reflection_sample_table(p.cube_face, n_levels, K, table, levels, p.refl_count);
        p.table_face = 0;
        HIP_TRY(c, p.d_refl_table.resize(table.size()));
        HIP_TRY(c, p.d_refl_lvl.resize(levels.size()));
        HIP_TRY(c, hipMemcpy(p.d_refl_table.p, table.data(), table.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(p.d_refl_lvl.p, levels.data(), levels.size(), hipMemcpyHostToDevice));
        p.table_face = p.cube_face;
        p.table_levels = n_levels;
        p.table_samples = K;
    }
    ReflDev rd;
    rd.n = (uint32_t)p.cube_n;
    rd.per_row = (uint32_t)p.cube_per_row;
    rd.shift = (uint32_t)cube_log2(p.cube_face);
    rd.n_levels = (uint32_t)n_levels;
    rd.samples = (uint32_t)K;
    for (int l = 0; l < kReflLevelsMax; l++) rd.count[l] = p.refl_count[l];
    const size_t n_chain = (size_t)((uint64_t)rd.n * refl_probe_texels(rd.shift)), n_out = (size_t)refl_out_texels(rd.n, rd.shift, rd.n_levels);
    if (p.d_refl_chain.n != n_chain || !p.d_refl_chain.p || p.d_refl_out.n != n_out || !p.d_refl_out.p) {
        p.refl_valid = false;
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (an earlier prefilter may still write the old images)
        HIP_TRY(c, p.d_refl_chain.resize(n_chain));
        HIP_TRY(c, p.d_refl_out.resize(n_out));
    }
    const bool timed = c->kernel_timing;
    if (timed)
        for (hipEvent_t& e : p.refl_ev)
            if (!e) HIP_TRY(c, hipEventCreate(&e));
    // On the context's stream, as jpt_probe_project: behind the accumulation of every render queued so far, and the accumulation of
    // every later render waits for what it reads.
    if (timed) HIP_TRY(c, hipEventRecord(p.refl_ev[0], c->stream));
    launch_reflection_chain(c->stream, rd, c->image.d_accum.p, (float)c->frame_count, p.d_refl_chain.p);
    if (timed) HIP_TRY(c, hipEventRecord(p.refl_ev[1], c->stream));
    launch_reflection_prefilter(c->stream, rd, p.d_refl_chain.p, p.d_refl_table.p, p.d_refl_lvl.p, p.d_refl_out.p);
    if (timed) HIP_TRY(c, hipEventRecord(p.refl_ev[2], c->stream));
    HIP_TRY(c, hipGetLastError());
    p.refl_timed = timed;
    p.refl_made = n_levels;
    p.refl_valid = true;
    return JPT_OK;
}

int jpt_get_reflection_chain_size(jpt_ctx* c, int32_t level, int32_t* face_size, uint64_t* offset_texels)
{
    if (!c) return JPT_E_INVALID;
    if (!face_size || !offset_texels) return fail(c, JPT_E_INVALID, "jpt_get_reflection_chain_size: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_get_reflection_chain_size: host-only context has no reflection probes");
    const PrimaryState& p = c->primary;
    if (!p.has_cubes()) return fail(c, JPT_E_STATE, "jpt_get_reflection_chain_size: no reflection probes (jpt_set_reflection_probes first)");
    const int32_t most = cube_log2(p.cube_face) + 1;
    const int32_t n_levels = p.refl_valid ? p.refl_made : (p.refl_levels_now() < most ? p.refl_levels_now() : most);
    if (level < 0 || level >= n_levels)
        return fail(c, JPT_E_INVALID, "jpt_get_reflection_chain_size: level must be in [0, " + std::to_string(n_levels) + ")");
    const uint32_t shift = (uint32_t)cube_log2(p.cube_face);
    *face_size = p.cube_face >> level;
    *offset_texels = refl_out_offset((uint32_t)p.cube_n, shift, (uint32_t)level);
    return JPT_OK;
}

int jpt_read_reflection_f32(jpt_ctx* c, int32_t level, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_reflection_f32: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_reflection_f32: host-only context: jpt_reflection_prefilter runs on the device");
    const PrimaryState& p = c->primary;
    if (!p.refl_valid) return fail(c, JPT_E_STATE, "jpt_read_reflection_f32: no jpt_reflection_prefilter of the current reflection probes and size yet");
    if (level < 0 || level >= p.refl_made) return fail(c, JPT_E_INVALID, "jpt_read_reflection_f32: level must be in [0, " + std::to_string(p.refl_made) + ")");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t shift = (uint32_t)cube_log2(p.cube_face);
    const size_t s = (size_t)(p.cube_face >> level), bytes = (size_t)p.cube_n * 6u * s * s * sizeof(float4);
    return read_out(c, p.d_refl_out.p + refl_out_offset((uint32_t)p.cube_n, shift, (uint32_t)level), bytes, out);
}

int jpt_get_reflection_timing(jpt_ctx* c, float* chain_ms, float* prefilter_ms)
{
    if (!c) return JPT_E_INVALID;
    if (!chain_ms || !prefilter_ms) return fail(c, JPT_E_INVALID, "jpt_get_reflection_timing: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_get_reflection_timing: host-only context: jpt_reflection_prefilter runs on the device");
    PrimaryState& p = c->primary;
    if (!p.refl_valid || !p.refl_timed)
        return fail(c, JPT_E_STATE, "jpt_get_reflection_timing: the last jpt_reflection_prefilter did not run under jpt_set_kernel_timing");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(p.refl_ev[2]));
    HIP_TRY(c, hipEventElapsedTime(chain_ms, p.refl_ev[0], p.refl_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(prefilter_ms, p.refl_ev[1], p.refl_ev[2]));
    return JPT_OK;
}

}  // extern "C"
