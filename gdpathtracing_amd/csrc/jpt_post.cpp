// jpt_post.cpp -- the post stages of include/jpt.h: the calls that read the progressive sum on the context's stream and keep what they make
// in buffers of their own (PostState, jpt_ctx.h) -- jpt_denoise, jpt_bake_finish, the directional planes and jpt_bake_finish_directional,
// jpt_display, jpt_meter, the variance plane and jpt_noise_estimate, jpt_render_converge -- with their parameters and read-backs, and the
// refusals every such call opens with (reads_sum: also jpt_probe_project, jpt_reflection_prefilter and jpt_encode's mean).
#include "jpt_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

namespace jpt {

void PostState::lightmap_release()
{
    for (DevBuf<float4>* b : {&d_lm_xg, &d_lm_ng, &d_lm_ping, &d_lm_pong}) b->release();
    lm_result = nullptr;
    lmd_release();
}

void PostState::lmd_release()
{
    for (DevBuf<float4>* b : {&d_lmd_xg, &d_lmd_ng, &d_lmd_ping, &d_lmd_pong, &d_lmd_out}) b->release();
    lmd_valid = false;
}

void PostState::framebuffers_remade(bool resized)
{
    variance_valid = noise_valid = false;   // (jpt_set_variance's plane is of the frames before; the next render overwrites it)
    if (!resized) return;
    // the images of jpt_denoise and its history, jpt_bake_finish, jpt_bake_finish_directional and jpt_display are of the old size, the metering state and
    // what the directional planes hold too (the planes themselves, like the variance plane, are re-made by the next render: ensure_bake_dir)
    bake_dir_valid = false;
    for (DevBuf<float4>* b : {&d_dn_pos, &d_dn_nrm, &d_dn_alb, &d_dn_ping, &d_dn_pong, &d_disp_f32, &d_disp_pyramid}) b->release();
    d_dn_ldr.release();
    d_dn_var.release();
    for (auto& set : d_dh_set)
        for (DevBuf<float4>& b : set) b.release();
    d_dh_iv.release();
    history_drop();
    d_disp_ldr.release();
    lightmap_release();
    dn_valid = dn_var_valid = disp_valid = meter_valid = false;
}

int reads_sum(jpt_ctx* c, const char* call, const char* what, const char* host_only, const char* whole, const char* steps)
{
    const std::string who = call;
    if (c->denoise != JPT_DENOISE_PROGRESSIVE) return fail(c, JPT_E_STATE, who + what + ": the denoising mode must be JPT_DENOISE_PROGRESSIVE");
    if (c->debug_steps) return fail(c, JPT_E_STATE, who + (steps ? steps : ": the accumulation holds DEBUG_STEPS counts, not radiance (jpt_set_debug_steps)"));
    if (c->rank != 0 || c->world != 1) return fail(c, JPT_E_STATE, who + " needs the whole image on one context (world == 1)" + whole);
    if (host_only && c->device < 0) return fail(c, JPT_E_DEVICE, host_only);
    return JPT_OK;
}

int sum_ready(jpt_ctx* c, const char* call)
{
    if (!c->params_set) return fail(c, JPT_E_STATE, std::string(call) + ": jpt_set_params not called");
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, std::string(call) + ": no frame accumulated since the last reset");
    return JPT_OK;
}

int check_denoise_params(const AtrousParams& p, std::string& why)
{
    if (p.passes < 1 || p.passes > kAtrousMaxPasses) why = "jpt_denoise_params: passes must be in [1, 6]";
    else if (p.normal_power_log2 < 0 || p.normal_power_log2 > 8) why = "jpt_denoise_params: normal_power_log2 must be in [0, 8]";
    else if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) why = "jpt_denoise_params: sigma_plane must be finite and > 0";
    else if (!std::isfinite(p.sigma_color) || !(p.sigma_color > 0.0f)) why = "jpt_denoise_params: sigma_color must be finite and > 0";
    else return JPT_OK;
    return JPT_E_INVALID;
}

int check_bake_finish_params(const char* call, const LightmapParams& p, std::string& why)
{
    const std::string who = std::string(call) + ": ";
    if (p.passes < 0 || p.passes > kLightmapMaxPasses) why = who + "passes must be in [0, 6]";
    else if (p.normal_power_log2 < 0 || p.normal_power_log2 > 8) why = who + "normal_power_log2 must be in [0, 8]";
    else if (p.dilate < 0 || p.dilate > kLightmapMaxDilate) why = who + "dilate must be in [0, 64]";
    else if (!std::isfinite(p.sigma_distance) || !(p.sigma_distance > 0.0f)) why = who + "sigma_distance must be finite and > 0";
    else if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) why = who + "sigma_plane must be finite and > 0";
    else if (!std::isfinite(p.sigma_color) || !(p.sigma_color > 0.0f)) why = who + "sigma_color must be finite and > 0";
    else return JPT_OK;
    return JPT_E_INVALID;
}

// jpt_set_bake_directional: what a render with the switch on and bake images present refuses -- the moment kernel reads the per-frame
// values the wavefront route keeps, of radiance, summed progressively.  Without bake images the switch has no effect.
int check_bake_directional(jpt_ctx* c)
{
    if (!c->post.bake_dir || !c->primary.has_bake()) return JPT_OK;
    if (c->kernel_variant != JPT_KERNEL_WAVEFRONT)
        return fail(c, JPT_E_STATE, "jpt_set_bake_directional: the reference-layout kernel adds frame by frame and keeps no per-frame values: set "
                                    "JPT_KERNEL_WAVEFRONT (jpt_set_kernel) or switch the directional planes off");
    if (c->denoise != JPT_DENOISE_PROGRESSIVE)
        return fail(c, JPT_E_STATE, "jpt_set_bake_directional: the moments follow the progressive accumulation: the denoising mode must be JPT_DENOISE_PROGRESSIVE "
                                    "(temporal reprojection and JPT_DENOISE_NONE keep no sum)");
    if (c->debug_steps) return fail(c, JPT_E_STATE, "jpt_set_bake_directional: a DEBUG_STEPS render holds step counts, not radiance (jpt_set_debug_steps)");
    return JPT_OK;
}

// the three moment planes at the size of the context's rows, made (and zeroed, so that a sum continued without a reset starts from
// +0) when they are missing or of another size
int ensure_bake_dir(jpt_ctx* c)
{
    PostState& q = c->post;
    const size_t need = 3u * (size_t)c->width * (size_t)c->local_rows;
    if (q.d_bake_dir.p && q.d_bake_dir.n == need) return JPT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (renders in flight may write the old planes: every one ends with work on the stream)
    q.bake_dir_valid = false;
    HIP_TRY(c, q.d_bake_dir.resize(need));
    if (need) HIP_TRY(c, hipMemsetAsync(q.d_bake_dir.p, 0, need * sizeof(float4), c->stream));
    return JPT_OK;
}

// jpt_set_variance: what a render with the switch on refuses -- the moment kernel reads the per-frame values the wavefront route
// keeps, of radiance, summed progressively
int check_variance(jpt_ctx* c)
{
    if (!c->post.variance) return JPT_OK;
    if (c->kernel_variant != JPT_KERNEL_WAVEFRONT)
        return fail(c, JPT_E_STATE, "jpt_set_variance: the reference-layout kernel adds frame by frame and keeps no per-frame values: set "
                                    "JPT_KERNEL_WAVEFRONT (jpt_set_kernel) or switch the variance plane off");
    if (c->denoise != JPT_DENOISE_PROGRESSIVE)
        return fail(c, JPT_E_STATE, "jpt_set_variance: the moment follows the progressive accumulation: the denoising mode must be JPT_DENOISE_PROGRESSIVE "
                                    "(temporal reprojection and JPT_DENOISE_NONE keep no sum)");
    if (c->debug_steps) return fail(c, JPT_E_STATE, "jpt_set_variance: a DEBUG_STEPS render holds step counts, not radiance (jpt_set_debug_steps)");
    return JPT_OK;
}

// the plane at the size of the context's rows, made (and zeroed) when it is missing or of another size
int ensure_variance(jpt_ctx* c)
{
    PostState& q = c->post;
    const size_t need = (size_t)c->width * (size_t)c->local_rows;
    if (q.d_variance.p && q.d_variance.n == need) return JPT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (renders in flight may write the old plane: every one ends with work on the stream)
    q.variance_valid = q.noise_valid = false;
    HIP_TRY(c, q.d_variance.resize(need));
    if (need) HIP_TRY(c, hipMemsetAsync(q.d_variance.p, 0, need * sizeof(float4), c->stream));
    return JPT_OK;
}

}  // namespace jpt

namespace {

// what a read-back of a stage's result opens with (`stage`: the call that makes it; `valid`, or `none`)
int read_common(jpt_ctx* c, bool have_out, const char* stage, bool valid, const char* none)
{
    if (!c) return JPT_E_INVALID;
    if (!have_out) return fail(c, JPT_E_INVALID, "null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, std::string("host-only context: ") + stage + " runs on the device");
    if (!valid) return fail(c, JPT_E_STATE, none);
    HIP_TRY(c, hipSetDevice(c->device));
    return JPT_OK;
}
int read_denoise_common(jpt_ctx* c, bool have_out) { return read_common(c, have_out, "jpt_denoise", c && c->post.dn_valid, "no jpt_denoise at the current resolution yet"); }
int read_display_common(jpt_ctx* c, bool have_out) { return read_common(c, have_out, "jpt_display", c && c->post.disp_valid, "no jpt_display at the current resolution yet"); }

// the planes of a read: JPT_OK, or the refusal
int bake_directional_ready(jpt_ctx* c, const char* call)
{
    const PostState& q = c->post;
    const std::string who = std::string(call) + ": ";
    if (c->device < 0) return fail(c, JPT_E_DEVICE, who + "host-only context: the moments are made on the device");
    if (!q.bake_dir) return fail(c, JPT_E_STATE, who + "the directional planes are switched off (jpt_set_bake_directional)");
    if (!c->primary.has_bake()) return fail(c, JPT_E_STATE, who + "no bake images (jpt_bake_begin or jpt_set_bake_texels first)");
    if (!q.d_bake_dir.p || !q.bake_dir_valid || q.d_bake_dir.n != 3u * (size_t)c->width * (size_t)c->local_rows)
        return fail(c, JPT_E_STATE, who + "no bake render with the switch on at the current size yet");
    return JPT_OK;
}

// the plane of a read or of an estimate: JPT_OK, or the refusal
int variance_ready(jpt_ctx* c, const char* call)
{
    const PostState& q = c->post;
    const std::string who = std::string(call) + ": ";
    if (c->device < 0) return fail(c, JPT_E_DEVICE, who + "host-only context: the moment is made on the device");
    if (!q.variance) return fail(c, JPT_E_STATE, who + "the variance plane is switched off (jpt_set_variance)");
    if (!q.d_variance.p || !q.variance_valid || q.d_variance.n != (size_t)c->width * (size_t)c->local_rows)
        return fail(c, JPT_E_STATE, who + "no render with the switch on at the current size yet");
    return JPT_OK;
}

// what jpt_bake_finish and jpt_bake_finish_directional ask of the bake images and the sum, in their order (`switched`: the directional form)
int lightmap_source_ready(jpt_ctx* c, const std::string& who, bool switched)
{
    const PrimaryState& p = c->primary;
    if (switched && !c->post.bake_dir) return fail(c, JPT_E_STATE, who + ": the directional planes are switched off (jpt_set_bake_directional)");
    if (!p.has_bake()) return fail(c, JPT_E_STATE, who + ": no bake images (jpt_bake_begin or jpt_set_bake_texels first)");
    if (p.has_probes()) return fail(c, JPT_E_STATE, who + ": the lightmap is made of texel images, and the context holds probes (jpt_set_probes)");
    if (p.has_cubes())
        return fail(c, JPT_E_STATE, who + ": the lightmap is made of texel images, and the context holds reflection probes (jpt_set_reflection_probes)");
    if (!c->params_set || p.bake_w != c->width || p.bake_h != c->height)
        return fail(c, JPT_E_STATE, who + ": the bake images are " + std::to_string(p.bake_w) + " x " + std::to_string(p.bake_h) + " texels but jpt_set_params says " +
                                        std::to_string(c->width) + " x " + std::to_string(c->height));
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, who + ": no frame accumulated since the last reset");
    return JPT_OK;
}

}  // namespace

extern "C" {

int jpt_set_denoise_params(jpt_ctx* c, const jpt_denoise_params* params)
{
    if (!c) return JPT_E_INVALID;
    const AtrousParams p = denoise_params_of(params);
    std::string why;
    const int rc = check_denoise_params(p, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_denoise runs on the device");
    c->post.dn_params = p;
    return JPT_OK;
}

int jpt_denoise(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    const int rc = reads_sum(c, "jpt_denoise", " filters the progressive accumulation", "host-only context: jpt_denoise runs on the device");
    if (rc != JPT_OK) return rc;
    if (!c->scene.device_ready) return fail(c, JPT_E_STATE, "jpt_denoise: no scene");
    if (!c->params_set || !c->camera_set) return fail(c, JPT_E_STATE, "jpt_denoise: jpt_set_params / jpt_set_camera not called");
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, "jpt_denoise: no frame accumulated since the last reset");
    CamModelDev cm;   // (the guides are the first hits of the view the renders took: jpt_set_camera_model)
    const int rc_cm = view_now(c, "jpt_denoise", "the guides", cm);
    if (rc_cm != JPT_OK) return rc_cm;
    PostState& q = c->post;
    const bool history = q.dn_hist.enable != 0;
    if (history) {   // (jpt_set_denoise_history: bake images, probes and reflection probes are view_now's refusals)
        if (c->primary.lens_radius > 0.0f)
            return fail(c, JPT_E_STATE, "jpt_denoise with jpt_set_denoise_history on: the lens radius is > 0 (jpt_set_lens): the history is reprojected through a pinhole");
        if (c->primary.camera_model != JPT_CAMERA_PINHOLE)
            return fail(c, JPT_E_STATE, "jpt_denoise with jpt_set_denoise_history on: the camera model must be JPT_CAMERA_PINHOLE (jpt_set_camera_model)");
        if (q.dh_called && q.dh_restarts == c->image.accum_restarts)
            return fail(c, JPT_E_STATE, "jpt_denoise with jpt_set_denoise_history on: the history already holds the frames accumulated since the last reset, and a "
                                        "second call would count them twice (jpt_accum_reset or jpt_denoise_history_reset first)");
    }
    const bool guided = !history && q.dn_var.enable != 0;
    if (guided) {   // (jpt_set_denoise_variance: refused, never filtered with the fixed tolerance instead)
        const int rc_v = variance_ready(c, "jpt_denoise with jpt_set_denoise_variance on");
        if (rc_v != JPT_OK) return rc_v;
        if (c->frame_count < 2)
            return fail(c, JPT_E_STATE, "jpt_denoise with jpt_set_denoise_variance on: one frame accumulated since the last reset, and a variance needs two");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->width * c->height;
    if (q.d_dn_ping.n != npx || !q.d_dn_ping.p) {
        for (DevBuf<float4>* b : {&q.d_dn_pos, &q.d_dn_nrm, &q.d_dn_alb, &q.d_dn_ping, &q.d_dn_pong}) HIP_TRY(c, b->resize(npx));
        HIP_TRY(c, q.d_dn_ldr.resize(npx));
    }
    if (guided || history) HIP_TRY(c, q.d_dn_var.resize(npx));
    if (history && (q.d_dh_iv.n != npx || !q.d_dh_iv.p)) {
        q.history_drop();
        for (auto& set : q.d_dh_set)
            for (DevBuf<float4>& b : set) HIP_TRY(c, b.resize(npx));
        HIP_TRY(c, q.d_dh_iv.resize(npx));
    }
    // On the context's stream: it is ordered behind the accumulation of every render queued so far (launch_render) and behind the
    // device refits (queue_instance_refit), and the accumulation of every later render waits for what it holds.
    hipStream_t s = c->stream;
    if (npx) {
        launch_guides(s, c->ds, c->camera, cm, c->width, c->height, q.d_dn_pos.p, q.d_dn_nrm.p, q.d_dn_alb.p);
        if (history) {
            // the previous set seen from the previous call's view; a view that is bit for bit this one reprojects every pixel onto itself
            DevBuf<float4>* prev = q.d_dh_set[q.dh_cur];
            DevBuf<float4>* next = q.d_dh_set[q.dh_cur ^ 1];
            const bool same_view = q.dh_have && std::memcmp(q.dh_camera.vp, c->camera.vp, sizeof c->camera.vp) == 0 &&
                                   std::memcmp(&q.dh_camera.position, &c->camera.position, sizeof c->camera.position) == 0;
            HistoryView view;
            std::memcpy(view.vp, q.dh_camera.vp, sizeof view.vp);
            launch_denoise_history(s, q.dn_hist, q.dn_params.normal_power_log2, c->width, c->height, c->image.d_accum.p, c->frame_count, q.d_dn_pos.p, q.d_dn_nrm.p,
                                   q.d_dn_alb.p, view, same_view, q.dh_have ? prev[0].p : nullptr, q.dh_have ? prev[1].p : nullptr,
                                   q.dh_have ? prev[2].p : nullptr, next[0].p, next[1].p, next[2].p, q.d_dh_iv.p);
            launch_atrous_history(s, q.dn_params, q.dn_var, c->width, c->height, q.d_dh_iv.p, q.d_dn_pos.p, q.d_dn_nrm.p, q.d_dn_alb.p, q.d_dn_ping.p,
                                  q.d_dn_pong.p, q.d_dn_ldr.p, q.d_dn_var.p);
        } else if (guided)
            launch_atrous_variance(s, q.dn_params, q.dn_var, c->width, c->height, 0, c->image.d_accum.p, q.d_variance.p, c->frame_count, q.d_dn_pos.p, q.d_dn_nrm.p,
                                   q.d_dn_alb.p, q.d_dn_ping.p, q.d_dn_pong.p, q.d_dn_ldr.p, q.d_dn_var.p);
        else
            launch_atrous(s, q.dn_params, c->width, c->height, c->image.d_accum.p, (float)c->frame_count, q.d_dn_pos.p, q.d_dn_nrm.p, q.d_dn_alb.p, q.d_dn_ping.p,
                          q.d_dn_pong.p, q.d_dn_ldr.p);
        HIP_TRY(c, hipGetLastError());
    }
    if (history) {
        q.dh_cur ^= 1;
        q.dh_have = q.dh_called = q.dh_read = true;
        q.dh_restarts = c->image.accum_restarts;
        q.dh_camera = c->camera;
    }
    q.dn_valid = true;
    q.dn_var_valid = guided || history;
    return JPT_OK;
}

int jpt_set_denoise_history(jpt_ctx* c, const jpt_denoise_history_params* params)
{
    if (!c) return JPT_E_INVALID;
    HistoryParams p;
    int32_t reserved[4] = {0, 0, 0, 0};
    if (params) {
        p.enable = params->enable;
        p.max_history = params->max_history;
        p.min_history = params->min_history;
        p.sigma_plane = params->sigma_plane;
        for (int k = 0; k < 4; k++) reserved[k] = params->reserved[k];
    }
    std::string why;
    const int rc = check_denoise_history_params(p, reserved, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_denoise runs on the device");
    if (p.enable != c->post.dn_hist.enable) {   // switching drops the history, and the frames of this accumulation are no longer counted
        c->post.history_drop();
        c->post.dh_called = false;
    }
    c->post.dn_hist = p;
    return JPT_OK;
}

int jpt_denoise_history_reset(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_denoise runs on the device");
    c->post.history_drop();
    c->post.dh_called = false;   // (nothing is left that could count the frames of this accumulation twice)
    return JPT_OK;
}

int jpt_read_denoise_history_f32(jpt_ctx* c, float* integrated4, float* length)
{
    int rc = read_denoise_common(c, true);
    if (rc) return rc;
    const PostState& q = c->post;
    if (!q.dh_read) return fail(c, JPT_E_STATE, "jpt_read_denoise_history_f32: no jpt_denoise with jpt_set_denoise_history on since the history was dropped");
    const size_t npx = (size_t)c->width * c->height;
    if (integrated4 && (rc = read_out(c, q.d_dh_iv.p, npx * sizeof(float4), integrated4)) != JPT_OK) return rc;
    if (length) {   // the .w of the (m, N) plane
        if ((rc = staged_read(c, q.d_dh_set[q.dh_cur][0].p, npx * sizeof(float4))) != JPT_OK) return rc;
        const float4* mn = c->image.h_read_pinned.as<float4>();
        for (size_t i = 0; i < npx; i++) length[i] = mn[i].w;
    }
    return JPT_OK;
}

int jpt_set_denoise_variance(jpt_ctx* c, const jpt_denoise_variance_params* params)
{
    if (!c) return JPT_E_INVALID;
    int32_t reserved = 0;
    const AtrousVarParams p = denoise_variance_params_of(params, reserved);
    std::string why;
    const int rc = check_denoise_variance_params(p, reserved, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_denoise runs on the device");
    c->post.dn_var = p;
    return JPT_OK;
}

int jpt_read_denoised_variance_f32(jpt_ctx* c, float* out)
{
    int rc = read_denoise_common(c, out != nullptr);
    if (rc) return rc;
    if (!c->post.dn_var_valid) return fail(c, JPT_E_STATE, "jpt_read_denoised_variance_f32: the last jpt_denoise ran without jpt_set_denoise_variance");
    return read_out(c, c->post.d_dn_var.p, (size_t)c->width * c->height * sizeof(float), out);
}

int jpt_read_denoised_f32(jpt_ctx* c, float* out)
{
    const int rc = read_denoise_common(c, out != nullptr);
    return rc ? rc : read_out(c, c->post.d_dn_ping.p, (size_t)c->width * c->height * sizeof(float4), out);
}

int jpt_read_denoised_rgba8(jpt_ctx* c, uint8_t* out)
{
    const int rc = read_denoise_common(c, out != nullptr);
    return rc ? rc : read_out(c, c->post.d_dn_ldr.p, (size_t)c->width * c->height * sizeof(uint32_t), out);
}

int jpt_read_guides_f32(jpt_ctx* c, float* position_t, float* normal, float* albedo)
{
    int rc = read_denoise_common(c, true);
    if (rc) return rc;
    const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
    float* outs[3] = {position_t, normal, albedo};
    const float4* src[3] = {c->post.d_dn_pos.p, c->post.d_dn_nrm.p, c->post.d_dn_alb.p};
    for (int k = 0; k < 3; k++)
        if (outs[k] && (rc = read_out(c, src[k], bytes, outs[k])) != JPT_OK) return rc;
    return JPT_OK;
}

// ---- jpt_bake_finish: the chart-aware filter and the dilation of a baked lightmap (jpt_lightmap.h) -----------------------------

int jpt_set_bake_finish_params(jpt_ctx* c, const jpt_bake_finish_params* params)
{
    if (!c) return JPT_E_INVALID;
    LightmapParams p;
    if (params) {
        p.passes = params->passes;
        p.normal_power_log2 = params->normal_power_log2;
        p.dilate = params->dilate;
        p.sigma_distance = params->sigma_distance;
        p.sigma_plane = params->sigma_plane;
        p.sigma_color = params->sigma_color;
    }
    std::string why;
    const int rc = check_bake_finish_params("jpt_set_bake_finish_params", p, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_bake_finish_params: host-only context: jpt_bake_finish runs on the device");
    c->post.lm_params = p;
    return JPT_OK;
}

int jpt_bake_finish(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    int rc = reads_sum(c, "jpt_bake_finish", " filters the progressive accumulation", "jpt_bake_finish: host-only context: it runs on the device");
    if (rc == JPT_OK) rc = lightmap_source_ready(c, "jpt_bake_finish", false);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    PostState& q = c->post;
    const PrimaryState& p = c->primary;
    const size_t npx = (size_t)c->width * c->height;   // (>= 1: the images have at least one texel)
    if (q.d_lm_ping.n != npx || !q.d_lm_ping.p) {
        q.lm_result = nullptr;
        for (DevBuf<float4>* b : {&q.d_lm_xg, &q.d_lm_ng, &q.d_lm_ping, &q.d_lm_pong}) HIP_TRY(c, b->resize(npx));
    }
    // On the context's stream, as jpt_denoise: behind the accumulation of every render queued so far, and the accumulation of every
    // later render waits for what it holds.
    q.lm_result = launch_lightmap_finish(c->stream, q.lm_params, c->width, c->height, c->image.d_accum.p, (float)c->frame_count, p.d_bake_pos.p, p.d_bake_nrm.p,
                                         q.d_lm_xg.p, q.d_lm_ng.p, q.d_lm_ping.p, q.d_lm_pong.p);
    HIP_TRY(c, hipGetLastError());
    return JPT_OK;
}

int jpt_read_lightmap_f32(jpt_ctx* c, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_lightmap_f32: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_lightmap_f32: host-only context: jpt_bake_finish runs on the device");
    if (!c->post.lm_result) return fail(c, JPT_E_STATE, "jpt_read_lightmap_f32: no jpt_bake_finish at the current size and bake images yet");
    HIP_TRY(c, hipSetDevice(c->device));
    return read_out(c, c->post.lm_result, (size_t)c->width * c->height * sizeof(float4), out);
}

// ---- directional lightmaps: the first moments of the incoming light per texel (jpt_bake_dir.h, jpt_kernels_bake_dir.hip) ----------

int jpt_set_bake_directional(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_bake_directional: host-only context: the moments are made on the device");
    PostState& q = c->post;
    const bool on = enable != 0;
    if (on == q.bake_dir) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the renders queued so far add to the planes: they finish first, then the planes and what was finished from them go
    if (q.d_bake_dir.p || q.d_lmd_out.p) HIP_TRY(c, hipStreamSynchronize(c->stream));
    q.bake_dir_release();
    q.lmd_release();
    q.bake_dir = on;
    return jpt_accum_reset(c);   // the sum and the moments are of the same frames: both start over
}

int jpt_read_bake_directional_f32(jpt_ctx* c, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_bake_directional_f32: null output");
    const int rc = bake_directional_ready(c, "jpt_read_bake_directional_f32");
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the renders queued so far, as jpt_read_accum_f32)
    return read_out(c, c->post.d_bake_dir.p, c->post.d_bake_dir.n * sizeof(float4), out);
}

void* jpt_device_bake_directional(jpt_ctx* c, int32_t finished, size_t* bytes_out)
{
    if (bytes_out) *bytes_out = 0;
    if (!c || c->device < 0 || !c->post.bake_dir) return nullptr;
    const PostState& q = c->post;
    const DevBuf<float4>& planes = finished ? q.d_lmd_out : q.d_bake_dir;
    if (!planes.p || !(finished ? q.lmd_valid : q.bake_dir_valid)) return nullptr;
    if (bytes_out) *bytes_out = planes.n * sizeof(float4);
    return planes.p;
}

int jpt_bake_finish_directional(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    const char* who = "jpt_bake_finish_directional";
    int rc = reads_sum(c, who, " filters the progressive moments", "jpt_bake_finish_directional: host-only context: it runs on the device", "",
                       ": DEBUG_STEPS renders make no moments (jpt_set_debug_steps)");
    if (rc == JPT_OK) rc = lightmap_source_ready(c, who, true);
    if (rc == JPT_OK) rc = bake_directional_ready(c, who);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    PostState& q = c->post;
    const PrimaryState& p = c->primary;
    const size_t npx = (size_t)c->width * c->height;   // (>= 1; world == 1: the planes are npx texels each)
    if (q.d_lmd_out.n != 3 * npx || !q.d_lmd_out.p) {
        q.lmd_valid = false;
        for (DevBuf<float4>* b : {&q.d_lmd_xg, &q.d_lmd_ng, &q.d_lmd_ping, &q.d_lmd_pong}) HIP_TRY(c, b->resize(npx));
        HIP_TRY(c, q.d_lmd_out.resize(3 * npx));
    }
    // On the context's stream, as jpt_bake_finish: each plane is the "accumulation" of one run of the same filter and dilation, with
    // the same frame count, images and parameters; the planes are filtered independently of one another and of the L0 map.
    for (int k = 0; k < 3; k++) {
        const float4* res = launch_lightmap_finish(c->stream, q.lm_params, c->width, c->height, q.d_bake_dir.p + (size_t)k * npx, (float)c->frame_count,
                                                   p.d_bake_pos.p, p.d_bake_nrm.p, q.d_lmd_xg.p, q.d_lmd_ng.p, q.d_lmd_ping.p, q.d_lmd_pong.p);
        HIP_TRY(c, hipMemcpyAsync(q.d_lmd_out.p + (size_t)k * npx, res, npx * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    q.lmd_valid = true;
    return JPT_OK;
}

int jpt_read_lightmap_directional_f32(jpt_ctx* c, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_lightmap_directional_f32: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_read_lightmap_directional_f32: host-only context: jpt_bake_finish_directional runs on the device");
    if (!c->post.lmd_valid || !c->post.d_lmd_out.p)
        return fail(c, JPT_E_STATE, "jpt_read_lightmap_directional_f32: no jpt_bake_finish_directional at the current size and bake images yet");
    HIP_TRY(c, hipSetDevice(c->device));
    return read_out(c, c->post.d_lmd_out.p, c->post.d_lmd_out.n * sizeof(float4), out);
}

// ---- jpt_display ------------------------------------------------------------------------------------------------------------
int jpt_set_display_params(jpt_ctx* c, const jpt_display_params* params)
{
    if (!c) return JPT_E_INVALID;
    DisplayParams p;
    if (params) {
        p.source = params->source;
        p.tonemap = params->tonemap;
        p.transfer = params->transfer;
        p.bloom_levels = params->bloom_levels;
        p.exposure = params->exposure;
        p.white = params->white;
        p.bloom_threshold = params->bloom_threshold;
        p.bloom_strength = params->bloom_strength;
    }
    std::string why;
    const int rc = check_display_params(p, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_display runs on the device");
    c->post.disp_params = p;
    return JPT_OK;
}

int jpt_display(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    int rc = reads_sum(c, "jpt_display", " grades the progressive accumulation", "host-only context: jpt_display runs on the device",
                       ": the bloom reads rows a partition does not hold");
    if (rc == JPT_OK) rc = sum_ready(c, "jpt_display");
    if (rc != JPT_OK) return rc;
    PostState& q = c->post;
    const DisplayParams prm = q.disp_params;
    const bool denoised = prm.source == JPT_DISPLAY_SOURCE_DENOISED;
    if (denoised && !q.dn_valid) return fail(c, JPT_E_STATE, "jpt_display: JPT_DISPLAY_SOURCE_DENOISED and no jpt_denoise at the current resolution yet");
    if (q.auto_exposure && !q.meter_valid)
        return fail(c, JPT_E_STATE, "jpt_display: auto-exposure is on (jpt_set_auto_exposure) and no jpt_meter ran since the metering state was reset");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->width * c->height;
    HIP_TRY(c, q.d_disp_f32.resize(npx));
    HIP_TRY(c, q.d_disp_ldr.resize(npx));
    if (prm.bloom_levels > 0) HIP_TRY(c, q.d_disp_pyramid.resize(display_pyramid_elems(c->width, c->height, kDisplayMaxLevels, nullptr)));
    // On the context's stream, as jpt_denoise: behind the accumulation of every render queued so far and behind a jpt_denoise queued
    // before it; the accumulation of every later render (and a later jpt_denoise) waits for what it holds.
    if (npx) {
        launch_display(c->stream, prm, c->width, c->height, denoised ? q.d_dn_ping.p : c->image.d_accum.p, denoised ? 1.0f : (float)c->frame_count,
                       q.d_disp_pyramid.p, q.d_disp_f32.p, q.d_disp_ldr.p, q.auto_exposure ? &q.d_meter_state.p->exposure : nullptr);
        HIP_TRY(c, hipGetLastError());
    }
    q.disp_valid = true;
    return JPT_OK;
}

int jpt_read_display_rgba8(jpt_ctx* c, uint8_t* out)
{
    const int rc = read_display_common(c, out != nullptr);
    return rc ? rc : read_out(c, c->post.d_disp_ldr.p, (size_t)c->width * c->height * sizeof(uint32_t), out);
}

int jpt_read_display_f32(jpt_ctx* c, float* out)
{
    const int rc = read_display_common(c, out != nullptr);
    return rc ? rc : read_out(c, c->post.d_disp_f32.p, (size_t)c->width * c->height * sizeof(float4), out);
}

// ---- jpt_meter ----------------------------------------------------------------------------------------------------------------
int jpt_set_meter_params(jpt_ctx* c, const jpt_meter_params* params)
{
    if (!c) return JPT_E_INVALID;
    MeterParams p;
    if (params) {
        p.source = params->source;
        p.mode = params->mode;
        p.low_permille = params->low_permille;
        p.high_permille = params->high_permille;
        p.key = params->key;
        p.min_exposure = params->min_exposure;
        p.max_exposure = params->max_exposure;
        p.adapt = params->adapt;
    }
    std::string why;
    const int rc = check_meter_params(p, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_meter runs on the device");
    c->post.meter_params = p;
    return JPT_OK;
}

int jpt_set_auto_exposure(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    if (enable != 0 && enable != 1) return fail(c, JPT_E_INVALID, "jpt_set_auto_exposure: enable must be 0 or 1");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_meter runs on the device");
    c->post.auto_exposure = enable != 0;
    return JPT_OK;
}

int jpt_meter_reset(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_meter runs on the device");
    c->post.meter_valid = false;
    return JPT_OK;
}

int jpt_meter(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    int rc = reads_sum(c, "jpt_meter", " meters the progressive accumulation", "host-only context: jpt_meter runs on the device");
    if (rc == JPT_OK) rc = sum_ready(c, "jpt_meter");
    if (rc != JPT_OK) return rc;
    PostState& q = c->post;
    const MeterParams prm = q.meter_params;
    const bool denoised = prm.source == JPT_DISPLAY_SOURCE_DENOISED;
    if (denoised && !q.dn_valid) return fail(c, JPT_E_STATE, "jpt_meter: JPT_DISPLAY_SOURCE_DENOISED and no jpt_denoise at the current resolution yet");
    if (c->width <= 0 || c->height <= 0) return fail(c, JPT_E_STATE, "jpt_meter: the image has no pixels");
    if ((uint64_t)c->width * (uint64_t)c->height > (1ull << 30))
        return fail(c, JPT_E_LIMIT, "jpt_meter: more than 2^30 pixels (a weight is at most 4 and a bin is a uint32)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, q.d_meter_bins.resize(kMeterBinWords));
    HIP_TRY(c, q.d_meter_state.resize(1));
    // On the context's stream, as jpt_display: behind the accumulation of every render, a jpt_denoise and a jpt_display queued before
    // it; a later jpt_display with auto-exposure reads the state record behind the resolve.
    const bool first = !q.meter_valid;
    launch_meter(c->stream, prm, c->width, c->height, denoised ? q.d_dn_ping.p : c->image.d_accum.p, denoised ? 1.0f : (float)c->frame_count, first, q.d_meter_bins.p,
                 q.d_meter_state.p);
    HIP_TRY(c, hipGetLastError());
    q.meter_valid = true;
    return JPT_OK;
}

int jpt_read_meter(jpt_ctx* c, jpt_meter_result* out, uint32_t* hist256)
{
    int rc = read_common(c, out != nullptr, "jpt_meter", c && c->post.meter_valid, "no jpt_meter since the metering state was reset");
    if (rc) return rc;
    static_assert(sizeof(jpt_meter_result) == sizeof(MeterState), "the state record is jpt_meter_result");
    if ((rc = read_out(c, c->post.d_meter_state.p, sizeof(MeterState), out)) != JPT_OK) return rc;
    return hist256 ? read_out(c, c->post.d_meter_bins.p, kMeterBins * sizeof(uint32_t), hist256) : JPT_OK;
}

// ---- jpt_set_variance, jpt_noise_estimate, jpt_render_converge (jpt_variance.h, jpt_kernels_variance.hip) -------------------------

int jpt_set_variance(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_set_variance: host-only context: the moment is made on the device");
    PostState& q = c->post;
    const bool on = enable != 0;
    if (on == q.variance) return JPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the renders queued so far add to the plane: they finish first, then the plane and the tile map go
    if (q.d_variance.p || q.d_noise_tiles.p) HIP_TRY(c, hipStreamSynchronize(c->stream));
    q.variance_release();
    q.variance = on;
    return jpt_accum_reset(c);   // the sum and the moment are of the same frames: both start over
}

int jpt_read_variance_f32(jpt_ctx* c, float* out)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_read_variance_f32: null output");
    const int rc = variance_ready(c, "jpt_read_variance_f32");
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the renders queued so far, as jpt_read_accum_f32)
    return read_rows_out(c, c->post.d_variance.p, sizeof(float), 4, false, out);
}

void* jpt_device_variance(jpt_ctx* c, size_t* bytes_out)
{
    if (bytes_out) *bytes_out = 0;
    if (!c || c->device < 0 || !c->post.variance || !c->post.d_variance.p || !c->post.variance_valid) return nullptr;
    if (bytes_out) *bytes_out = c->post.d_variance.n * sizeof(float4);
    return c->post.d_variance.p;
}

int jpt_set_noise_params(jpt_ctx* c, const jpt_noise_params* params)
{
    if (!c) return JPT_E_INVALID;
    NoiseParams p;
    if (params) {
        p.threshold = params->threshold;
        p.floor = params->floor;
        p.percentile_permille = params->percentile_permille;
        p.allowed_permille = params->allowed_permille;
    }
    std::string why;
    const int rc = check_noise_params(p, why);
    if (rc != JPT_OK) return fail(c, rc, why);
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_noise_estimate runs on the device");
    c->post.noise_params = p;
    return JPT_OK;
}

int jpt_noise_estimate(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    int rc = reads_sum(c, "jpt_noise_estimate", " reads the progressive accumulation", "host-only context: jpt_noise_estimate runs on the device");
    if (rc != JPT_OK) return rc;
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_noise_estimate: jpt_set_params not called");
    if ((rc = variance_ready(c, "jpt_noise_estimate")) != JPT_OK) return rc;
    if (c->frame_count == 0) return fail(c, JPT_E_STATE, "jpt_noise_estimate: no frame accumulated since the last reset");
    if ((uint64_t)c->width * (uint64_t)c->height > (1ull << 30)) return fail(c, JPT_E_LIMIT, "jpt_noise_estimate: more than 2^30 pixels (a bin is a uint32)");
    HIP_TRY(c, hipSetDevice(c->device));
    PostState& q = c->post;
    const size_t n_tiles = (size_t)((c->width + 7) / 8) * (size_t)((c->height + 7) / 8);
    if (q.d_noise_tiles.n != n_tiles || !q.d_noise_tiles.p) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (an estimate in flight may write the old map)
        q.noise_valid = false;
        HIP_TRY(c, q.d_noise_tiles.resize(n_tiles));
    }
    if (!q.d_noise_bins.p) {
        // the resolve leaves the working sets cleared: only fresh buffers are cleared here
        HIP_TRY(c, q.d_noise_bins.resize(kNoiseBinWords));
        HIP_TRY(c, q.d_noise_result.resize(1));
        HIP_TRY(c, hipMemsetAsync(q.d_noise_bins.p, 0, kNoiseBinWords * sizeof(uint32_t), c->stream));
    }
    // On the context's stream, as jpt_meter: behind the accumulation of every render queued before it.  In a bake render a texel
    // without a surface is not counted.
    const PrimaryState& p = c->primary;
    const float4* normal = p.has_bake() && !p.has_cubes() && p.bake_w == c->width && p.bake_h == c->height ? p.d_bake_nrm.p : nullptr;   // (resolve_primary's bake render)
    launch_noise_estimate(c->stream, q.noise_params, c->width, c->height, c->image.d_accum.p, q.d_variance.p, c->frame_count, normal, q.d_noise_bins.p, q.d_noise_tiles.p,
                          q.d_noise_result.p);
    HIP_TRY(c, hipGetLastError());
    q.noise_valid = true;
    return JPT_OK;
}

// what a read-back of the estimate opens with
static int read_noise_common(jpt_ctx* c, const char* call, bool have_out)
{
    if (!c) return JPT_E_INVALID;
    if (!have_out) return fail(c, JPT_E_INVALID, std::string(call) + ": null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context: jpt_noise_estimate runs on the device");
    if (!c->post.noise_valid) return fail(c, JPT_E_STATE, std::string(call) + ": no jpt_noise_estimate at the current size yet");
    HIP_TRY(c, hipSetDevice(c->device));
    return JPT_OK;
}

int jpt_read_noise(jpt_ctx* c, jpt_noise_result* out, uint32_t* hist256)
{
    int rc = read_noise_common(c, "jpt_read_noise", out != nullptr);
    if (rc) return rc;
    static_assert(sizeof(jpt_noise_result) == sizeof(NoiseResult), "the record is jpt_noise_result");
    if ((rc = read_out(c, c->post.d_noise_result.p, sizeof(NoiseResult), out)) != JPT_OK) return rc;
    return hist256 ? read_out(c, c->post.d_noise_bins.p, kMeterBins * sizeof(uint32_t), hist256) : JPT_OK;
}

int jpt_read_noise_tiles_f32(jpt_ctx* c, float* out)
{
    const int rc = read_noise_common(c, "jpt_read_noise_tiles_f32", out != nullptr);
    return rc ? rc : read_out(c, c->post.d_noise_tiles.p, c->post.d_noise_tiles.n * sizeof(float), out);
}

void* jpt_device_noise_tiles(jpt_ctx* c, size_t* bytes_out)
{
    if (bytes_out) *bytes_out = 0;
    if (!c || c->device < 0 || !c->post.noise_valid || !c->post.d_noise_tiles.p) return nullptr;
    if (bytes_out) *bytes_out = c->post.d_noise_tiles.n * sizeof(float);
    return c->post.d_noise_tiles.p;
}

// the loop a caller would write: render a step, estimate, read 32 bytes, until converged or max_frames
int jpt_render_converge(jpt_ctx* c, int32_t frames_per_step, int32_t max_frames, uint32_t first_frame_index, int32_t* frames_done, jpt_noise_result* last)
{
    if (!c) return JPT_E_INVALID;
    if (frames_done) *frames_done = 0;
    if (frames_per_step <= 0 || max_frames <= 0) return fail(c, JPT_E_INVALID, "jpt_render_converge: frames_per_step and max_frames must be > 0");
    if (!c->post.variance && c->device >= 0) return fail(c, JPT_E_STATE, "jpt_render_converge: the variance plane is switched off (jpt_set_variance)");
    jpt_noise_result res;
    std::memset(&res, 0, sizeof res);
    res.flags = JPT_NOISE_EMPTY;
    int32_t done = 0;
    while (done < max_frames) {
        const int32_t step = std::min(frames_per_step, max_frames - done);   // (the last step is shortened to land on max_frames)
        int rc = jpt_render_async(c, step, first_frame_index + (uint32_t)done);
        if (rc != JPT_OK) return rc;
        done += step;
        if (frames_done) *frames_done = done;
        if ((rc = jpt_noise_estimate(c)) != JPT_OK) return rc;
        if ((rc = jpt_read_noise(c, &res, nullptr)) != JPT_OK) return rc;   // the one wait of the step, for 32 bytes
        if (last) *last = res;
        if (res.flags & JPT_NOISE_CONVERGED) break;
    }
    return JPT_OK;
}

}  // extern "C"
