// jpt_debug.hip -- audit entry points of the C ABI (include/jpt.h, jpt_debug_*): pieces of the native walk run on
// caller-made inputs, so that properties the images only sample can be tested directly.
//
// jpt_debug_node_step4: the four-child record step of the native walk (Traversal<.., W4>::node_step4, jpt_trace_core.h) on
// (record, ray, distance bound) triples -- which of the four children does the walk keep?  The step's box tests are
// CONSERVATIVE tests on quantised planes (jpt_nodeq.h) with reciprocals from v_rcp_f32; what the tests must never do is
// drop a child whose box holds a triangle that Moller-Trumbore as written accepts (tests/test_quantized_walk.py feeds
// adversarial triples: axis-parallel rays, flat nodes, far ray origins, slivers, planes on grid steps).  On a device the
// kernel below runs the very function the tracing kernels inline; with JPT_DEVICE_HOST_ONLY a host restatement of the same
// arithmetic runs, its reciprocals perturbed by a chosen number of ulps (v_rcp_f32 is accurate to 1 ulp).
#include "../../include/jpt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jpt_encode.h"
#include "jpt_atrous_pass.h"
#include "jpt_builder.h"
#include "jpt_instance_math.h"
#include "jpt_kernels.h"
#include "jpt_lightmap.h"
#include "jpt_mesh_rebuild.h"
#include "jpt_nodeq.h"
#include "jpt_primary_ray.h"
#include "jpt_tlas_rebuild.h"
#include "jpt_trace_core.h"

using namespace jpt;

namespace {

thread_local std::string g_debug_error;

struct StepCase {   // 32 bytes
    float o[3], d[3];
    float t_max;    // hitInfo.t when the record is expanded
    uint32_t node;  // which record
};
static_assert(sizeof(StepCase) == 32, "StepCase");

__global__ void node_step4_probe(const WideNodeQ* __restrict__ nodes, const StepCase* __restrict__ cases, uint32_t n, uint8_t* __restrict__ taken)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const StepCase c = cases[i];
    WideSceneDev sc;
    std::memset(&sc, 0, sizeof sc);
    sc.nodesq = nodes;
    sc.n_instances = 1;
    Traversal<false, true> tr;
    tr.begin(sc, mk3(c.o[0], c.o[1], c.o[2]), mk3(c.d[0], c.d[1], c.d[2]));   // (sets the slab constants the way a walk does)
    tr.hit.t = c.t_max;
    tr.cur = (int32_t)c.node;
    tr.in_blas = true;
    tr.have = true;
    int32_t pushed[4] = {0, 0, 0, 0};
    const Traversal<false, true>::Stack st{nullptr, pushed, 0, 0, 4};   // every push lands in `pushed`
    DevCounters cnt = {};
    tr.node_step4(sc, st, cnt);
    // the children the walk keeps: the one it descends into and the ones it pushed.  The probe's records name child k
    // as reference k + 1 (never dereferenced).
    uint32_t mask = 0;
    if (tr.have && tr.cur >= 1 && tr.cur <= 4) mask |= 1u << (tr.cur - 1);
    for (int k = 0; k < tr.sp && k < 4; k++)
        if (pushed[k] >= 1 && pushed[k] <= 4) mask |= 1u << (pushed[k] - 1);
    taken[i] = (uint8_t)mask;
}

float step_ulps(float x, int ulps)
{
    for (int k = 0; k < (ulps < 0 ? -ulps : ulps); k++) x = std::nextafterf(x, ulps > 0 ? INFINITY : -INFINITY);
    return x;
}

// the arithmetic of node_step4's box tests, restated for the host (same operations in the same order; std::fmaf is the
// fused multiply-add, std::fmaxf / fminf ignore a NaN operand like v_max_f32 / v_min_f32)
uint8_t node_step4_host(const WideNodeQ& q, const StepCase& c, int rcp_ulps)
{
    float rD[3], ood[3], a[3], nb[3], fb[3];
    const float origin[3] = {q.ox, q.oy, q.oz}, scale[3] = {q.sx, q.sy, q.sz};
    const uint32_t lo[3] = {q.lo_x, q.lo_y, q.lo_z}, hi[3] = {q.hi_x, q.hi_y, q.hi_z};
    uint32_t nw[3], fw[3];
    for (int k = 0; k < 3; k++) {
        float r = 1.0f / c.d[k];
        if (std::isfinite(r) && r != 0.0f) r = step_ulps(r, r > 0.0f ? rcp_ulps : -rcp_ulps);   // |r| larger for ulps > 0
        r = r > kRcpClamp ? kRcpClamp : (r < -kRcpClamp ? -kRcpClamp : r);                         // (set_level keeps them finite)
        rD[k] = r;
        ood[k] = -(c.o[k] * rD[k]);
        a[k] = scale[k] * rD[k];
        const float b = std::fmaf(origin[k], rD[k], ood[k]);
        const float m = std::fmaf(kWalkSlackOverEps, std::fabs(a[k]), std::fabs(b)) + std::fabs(ood[k]);
        nb[k] = std::fmaf(-kWalkEps, m, b);
        fb[k] = std::fmaf(kWalkEps, m, b);
        uint32_t bits;
        std::memcpy(&bits, &c.d[k], 4);
        const bool neg = (int32_t)bits < 0;
        nw[k] = neg ? hi[k] : lo[k];
        fw[k] = neg ? lo[k] : hi[k];
    }
    uint32_t mask = 0;
    for (int k = 0; k < 4; k++) {
        float t_in = 0.0f, t_out = c.t_max;
        float tin_axes[3], tout_axes[3];
        for (int ax = 0; ax < 3; ax++) {
            tin_axes[ax] = std::fmaf((float)((nw[ax] >> (8 * k)) & 255u), a[ax], nb[ax]);
            tout_axes[ax] = std::fmaf((float)((fw[ax] >> (8 * k)) & 255u), a[ax], fb[ax]);
        }
        t_in = std::fmax(std::fmax(std::fmax(tin_axes[0], tin_axes[1]), tin_axes[2]), 0.0f);
        t_out = std::fmin(std::fmin(std::fmin(tout_axes[0], tout_axes[1]), tout_axes[2]), c.t_max);
        if (t_in <= t_out && q.child[k] != kEmptyChild) mask |= 1u << k;
    }
    return (uint8_t)mask;
}

// jpt_debug_env_lookup: the environment lookup the tracing kernels inline (env_radiance, jpt_shade.h), one direction per thread
__global__ void env_lookup_probe(EnvDev env, const float* __restrict__ dirs3, uint32_t n, float* __restrict__ rgb_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 c = env_radiance(env, mk3(dirs3[3 * (size_t)i], dirs3[3 * (size_t)i + 1], dirs3[3 * (size_t)i + 2]));
    rgb_out[3 * (size_t)i] = c.x;
    rgb_out[3 * (size_t)i + 1] = c.y;
    rgb_out[3 * (size_t)i + 2] = c.z;
}

// jpt_debug_dielectric: the dielectric event the *_tx kernels inline (dielectric_event, jpt_shade.h), one case per thread
__global__ void dielectric_probe(const float* __restrict__ normals3, const float* __restrict__ out_dirs3, const float* __restrict__ ior,
                                 const uint8_t* __restrict__ front, const float* __restrict__ xi_f, uint32_t n, float* __restrict__ dirs_out,
                                 float* __restrict__ fresnel_out, uint8_t* __restrict__ event_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 d;
    float fresnel;
    const int ev = dielectric_event(f3{normals3[3 * (size_t)i], normals3[3 * (size_t)i + 1], normals3[3 * (size_t)i + 2]},
                                    f3{out_dirs3[3 * (size_t)i], out_dirs3[3 * (size_t)i + 1], out_dirs3[3 * (size_t)i + 2]}, ior[i], front[i] != 0,
                                    xi_f[i], d, fresnel);
    dirs_out[3 * (size_t)i] = d.x;
    dirs_out[3 * (size_t)i + 1] = d.y;
    dirs_out[3 * (size_t)i + 2] = d.z;
    fresnel_out[i] = fresnel;
    event_out[i] = (uint8_t)ev;
}

// jpt_debug_lens_rays / _camera_rays / _bake_rays / _probe_rays / _cube_rays: the first rays of a render under `p` (first_ray, jpt_primary_ray.h), one pixel per
// thread; `valid` may be null
__global__ void primary_rays_probe(PrimaryRays p, RefCamera cam, int width, int height, uint32_t frame, float* __restrict__ origins_out,
                                   float* __restrict__ dirs_out, uint8_t* __restrict__ valid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)width * (uint32_t)height) return;
    Ray ray;
    const bool ok = first_ray(p, cam, width, height, (int)(i % (uint32_t)width), (int)(i / (uint32_t)width), frame, ray);
    origins_out[3 * (size_t)i] = ray.o.x;
    origins_out[3 * (size_t)i + 1] = ray.o.y;
    origins_out[3 * (size_t)i + 2] = ray.o.z;
    dirs_out[3 * (size_t)i] = ray.d.x;
    dirs_out[3 * (size_t)i + 1] = ray.d.y;
    dirs_out[3 * (size_t)i + 2] = ray.d.z;
    if (valid) valid[i] = ok ? 1 : 0;
}

}  // namespace

// jpt_debug_light_sample / jpt_debug_light_pdf (entry points in jpt_lighting.cpp, beside the context's tables): the emitter sampler and
// density the light-sampling kernels inline (light_sample / light_cos / light_pdf, jpt_shade.h), one item per thread
__global__ void light_probe(LightDev lt, SceneShading sh, int what, const float* __restrict__ xi4, const float* __restrict__ origins,
                            const float* __restrict__ dirs, const float* __restrict__ points, const uint32_t* __restrict__ inst,
                            const uint32_t* __restrict__ tri, uint32_t n, float* __restrict__ points_out, float* __restrict__ dirs_out,
                            float* __restrict__ pdf_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float total = lt.marg[lt.n_blocks];
    const f3 o = mk3(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]);
    if (what == 1) {
        const LightSample ls = light_sample(lt, xi4[4 * (size_t)i], xi4[4 * (size_t)i + 1], xi4[4 * (size_t)i + 2], xi4[4 * (size_t)i + 3]);
        const f3 dv = ls.y - o;
        const float d2 = dot3(dv, dv);
        const f3 l = normalize3(dv);
        const float c = light_cos(ls.e1, ls.e2, l);
        points_out[3 * (size_t)i] = ls.y.x;
        points_out[3 * (size_t)i + 1] = ls.y.y;
        points_out[3 * (size_t)i + 2] = ls.y.z;
        dirs_out[3 * (size_t)i] = l.x;
        dirs_out[3 * (size_t)i + 1] = l.y;
        dirs_out[3 * (size_t)i + 2] = l.z;
        pdf_out[i] = (c > 0.0f && total > 0.0f) ? light_pdf(ls.le, total, d2, c) : 0.0f;
    } else {
        float le[3];
        light_emission(sh.instances, sh.n_instances, sh.materials, sh.n_materials, inst[i], sh.tri_data[tri[i]].material_index, le);
        const WideTri& w = lt.wtris[tri[i]];
        const RefInstance& b = sh.instances[inst[i]];
        const f3 e1 = xform_dir(b.transform, mk3(w.e1[0], w.e1[1], w.e1[2])), e2 = xform_dir(b.transform, mk3(w.e2[0], w.e2[1], w.e2[2]));
        const f3 dv = mk3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]) - o;
        const f3 d = mk3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
        const bool emits = light_lum(le[0], le[1], le[2]) > 0.0f && total > 0.0f;
        pdf_out[i] = emits ? light_pdf(mk3(le[0], le[1], le[2]), total, dot3(dv, dv), light_cos(e1, e2, d)) : 0.0f;
    }
}

namespace jpt {
void launch_light_probe(hipStream_t stream, const LightDev& lt, const SceneShading& sh, int what, const float* xi4, const float* origins,
                        const float* dirs, const float* points, const uint32_t* inst, const uint32_t* tri, uint32_t n, float* points_out,
                        float* dirs_out, float* pdf_out)
{
    if (n == 0) return;
    hipLaunchKernelGGL(light_probe, dim3((n + 63u) / 64u), dim3(64), 0, stream, lt, sh, what, xi4, origins, dirs, points, inst, tri, n,
                       points_out, dirs_out, pdf_out);
}
}  // namespace jpt

namespace {

// jpt_debug_env_sample / jpt_debug_env_pdf: the sampler the MIS kernels inline (env_sample / env_pdf, jpt_shade.h), one item per thread
__global__ void env_sample_probe(EnvDev env, EnvSampDev es, const float* __restrict__ in, uint32_t n, int sample, float* __restrict__ dirs_out,
                                 float* __restrict__ pdf_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (sample) {
        float pdf;
        const f3 d = env_sample(env, es, in[2 * (size_t)i], in[2 * (size_t)i + 1], pdf);
        dirs_out[3 * (size_t)i] = d.x;
        dirs_out[3 * (size_t)i + 1] = d.y;
        dirs_out[3 * (size_t)i + 2] = d.z;
        pdf_out[i] = pdf;
    } else {
        pdf_out[i] = env_pdf(env, es, mk3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]));
    }
}

// The three env-sampling audit entries: the map's tables built on the device (launch_env_tables) or on the host (env_build_row /
// env_build_marginal), then `what` = 0 nothing more, 1 env_sample of n (xi0, xi1) pairs, 2 env_pdf of n directions
int env_sampling_debug(int device_id, const float* rgb, int32_t width, int32_t height, const float* rotation9, int what, const float* in,
                       uint32_t n, float* dirs_out, float* pdf_out, float* cond_out, float* marg_out, float* total_out)
{
    if (!rgb || (n && (!in || !pdf_out || (what == 1 && !dirs_out)))) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    int rc = check_env_map(rgb, width, height, g_debug_error);
    if (rc == JPT_OK) rc = check_env_params(rotation9, 1.0f, g_debug_error);
    if (rc != JPT_OK) return rc;
    if (rotation9 && !env_rotation_orthonormal(rotation9)) {
        g_debug_error = "the map sampler needs an orthonormal rotation";
        return JPT_E_INVALID;
    }
    std::vector<float4> texels;
    pack_env_texels(rgb, width, height, texels);
    EnvDev env;
    env.w = width;
    env.h = height;
    static const float kIdentity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    std::memcpy(env.rot, rotation9 ? rotation9 : kIdentity, sizeof env.rot);
    env.intensity = 1.0f;
    const size_t wh = (size_t)width * (size_t)height;
    const size_t in_floats = (size_t)n * (what == 1 ? 2u : 3u);
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        std::vector<float> cond(wh), marg(height);
        for (int32_t i = 0; i < height; i++) marg[i] = env_build_row(texels.data(), width, height, i, cond.data() + (size_t)i * width);
        const float total = env_build_marginal(marg.data(), height);
        if (cond_out) std::memcpy(cond_out, cond.data(), wh * sizeof(float));
        if (marg_out) std::memcpy(marg_out, marg.data(), (size_t)height * sizeof(float));
        if (total_out) *total_out = total;
        env.texels = texels.data();
        const EnvSampDev es{cond.data(), marg.data(), total};
        for (uint32_t i = 0; i < n && what == 1; i++) {
            const f3 d = env_sample(env, es, in[2 * (size_t)i], in[2 * (size_t)i + 1], pdf_out[i]);
            dirs_out[3 * (size_t)i] = d.x;
            dirs_out[3 * (size_t)i + 1] = d.y;
            dirs_out[3 * (size_t)i + 2] = d.z;
        }
        for (uint32_t i = 0; i < n && what == 2; i++)
            pdf_out[i] = env_pdf(env, es, f3{in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]});
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* w) {
        g_debug_error = std::string(w) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    float4* d_tex = nullptr;
    float *d_cond = nullptr, *d_marg = nullptr, *d_in = nullptr, *d_dirs = nullptr, *d_pdf = nullptr;
    if ((e = hipMalloc((void**)&d_tex, wh * sizeof(float4))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMalloc((void**)&d_cond, wh * sizeof(float))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMalloc((void**)&d_marg, ((size_t)height + 1) * sizeof(float))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && n && (e = hipMalloc((void**)&d_in, in_floats * sizeof(float))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && n && (e = hipMalloc((void**)&d_dirs, (size_t)n * 3u * sizeof(float))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && n && (e = hipMalloc((void**)&d_pdf, (size_t)n * sizeof(float))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMemcpy(d_tex, texels.data(), wh * sizeof(float4), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && n && (e = hipMemcpy(d_in, in, in_floats * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    float total = 0.0f;
    if (rc == JPT_OK) {
        launch_env_tables(nullptr, d_tex, width, height, d_cond, d_marg, d_marg + height);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "launch_env_tables");
    }
    if (rc == JPT_OK && (e = hipMemcpy(&total, d_marg + height, sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && n && what) {
        env.texels = d_tex;
        const EnvSampDev es{d_cond, d_marg, total};
        hipLaunchKernelGGL(env_sample_probe, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, env, es, d_in, n, what == 1 ? 1 : 0, d_dirs, d_pdf);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "env_sample_probe");
    }
    if (rc == JPT_OK && cond_out && (e = hipMemcpy(cond_out, d_cond, wh * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && marg_out && (e = hipMemcpy(marg_out, d_marg, (size_t)height * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && total_out) *total_out = total;
    if (rc == JPT_OK && n && what == 1 && (e = hipMemcpy(dirs_out, d_dirs, (size_t)n * 3u * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && n && what && (e = hipMemcpy(pdf_out, d_pdf, (size_t)n * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    for (void* p : {(void*)d_tex, (void*)d_cond, (void*)d_marg, (void*)d_in, (void*)d_dirs, (void*)d_pdf})
        if (p) (void)hipFree(p);
    return rc;
}

// The first rays of one frame under `p`, every pixel in raster order: the host loop with JPT_DEVICE_HOST_ONLY, else primary_rays_probe
// on `device_id` -- one allocation for the bake images or the probe positions (host memory in `p`, uploaded here), the origins, the directions and the
// valid bytes (valid_out may be null).  `what` names the probe in a device error.
int primary_rays_debug(int device_id, const char* what, PrimaryRays p, const RefCamera& cam, int32_t width, int32_t height, uint32_t frame,
                       float* origins3_out, float* dirs3_out, uint8_t* valid_out)
{
    const size_t n = (size_t)width * (size_t)height;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        for (size_t i = 0; i < n; i++) {
            Ray ray;
            const bool ok = first_ray(p, cam, width, height, (int)(i % (size_t)width), (int)(i / (size_t)width), frame, ray);
            origins3_out[3 * i] = ray.o.x;
            origins3_out[3 * i + 1] = ray.o.y;
            origins3_out[3 * i + 2] = ray.o.z;
            dirs3_out[3 * i] = ray.d.x;
            dirs3_out[3 * i + 1] = ray.d.y;
            dirs3_out[3 * i + 2] = ray.d.z;
            if (valid_out) valid_out[i] = ok ? 1 : 0;
        }
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    const size_t b_img = p.kind == PrimaryRays::kBake ? n * sizeof(float4) : 0, b_ray = n * 3u * sizeof(float);
    // (a probe or cube render's positions, at the front: 4-byte data)
    const size_t b_pos = p.kind == PrimaryRays::kProbe ? (size_t)p.probe.n * 3u * sizeof(float) : (p.kind == PrimaryRays::kCube ? (size_t)p.cube.n * 3u * sizeof(float) : 0);
    char* d_all = nullptr;   // position4, normal4 (16-byte images first) or the probe positions, origins, directions, valid
    if ((e = hipMalloc((void**)&d_all, 2 * b_img + b_pos + 2 * b_ray + (valid_out ? n : 0))) != hipSuccess) return hip_fail(e, "hipMalloc");
    float *d_o = reinterpret_cast<float*>(d_all + 2 * b_img + b_pos), *d_d = reinterpret_cast<float*>(d_all + 2 * b_img + b_pos + b_ray);
    uint8_t* d_valid = valid_out ? reinterpret_cast<uint8_t*>(d_all + 2 * b_img + b_pos + 2 * b_ray) : nullptr;
    int rc = JPT_OK;
    if (b_pos && p.kind == PrimaryRays::kCube) {
        if ((e = hipMemcpy(d_all, p.cube.position, b_pos, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
        p.cube.position = reinterpret_cast<const float*>(d_all);
    } else if (b_pos) {
        if ((e = hipMemcpy(d_all, p.probe.position, b_pos, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
        p.probe.position = reinterpret_cast<const float*>(d_all);
    }
    if (b_img) {
        if ((e = hipMemcpy(d_all, p.bake.position, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
        if (rc == JPT_OK && (e = hipMemcpy(d_all + b_img, p.bake.normal, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
        p.bake.position = reinterpret_cast<const float4*>(d_all);
        p.bake.normal = reinterpret_cast<const float4*>(d_all + b_img);
    }
    if (rc == JPT_OK) {
        hipLaunchKernelGGL(primary_rays_probe, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, nullptr, p, cam, width, height, frame, d_o, d_d, d_valid);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, what);
    }
    if (rc == JPT_OK && (e = hipMemcpy(origins3_out, d_o, b_ray, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(dirs3_out, d_d, b_ray, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && valid_out && (e = hipMemcpy(valid_out, d_valid, n, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

}  // namespace

void jpt::set_debug_error(const std::string& why) { g_debug_error = why; }

extern "C" {

const char* jpt_debug_last_error(void) { return g_debug_error.c_str(); }

int jpt_debug_quantize_nodes4(const void* nodes4, uint32_t n_nodes, void* nodesq_out)
{
    if ((n_nodes && !nodes4) || !nodesq_out) return JPT_E_INVALID;
    const WideNode4* in = static_cast<const WideNode4*>(nodes4);
    WideNodeQ* out = static_cast<WideNodeQ*>(nodesq_out);
    for (uint32_t i = 0; i < n_nodes; i++) {
        WideNode4 n;
        std::memcpy(&n, reinterpret_cast<const char*>(in) + (size_t)i * sizeof(WideNode4), sizeof n);
        WideNodeQ q;
        quantize_node4(n, q);
        std::memcpy(reinterpret_cast<char*>(out) + (size_t)i * sizeof(WideNodeQ), &q, sizeof q);
    }
    return JPT_OK;
}

int jpt_debug_node_step4(int device_id, const void* nodes4, uint32_t n_nodes, const void* cases32, uint32_t n_cases, int32_t host_rcp_ulps,
                         uint8_t* taken_out)
{
    if (!nodes4 || !cases32 || !taken_out || n_nodes == 0) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    std::vector<WideNodeQ> q(n_nodes);
    if (jpt_debug_quantize_nodes4(nodes4, n_nodes, q.data()) != JPT_OK) return JPT_E_INVALID;
    const StepCase* cases = static_cast<const StepCase*>(cases32);
    for (uint32_t i = 0; i < n_cases; i++)
        if (cases[i].node >= n_nodes) {
            g_debug_error = "a case names a record that does not exist";
            return JPT_E_INVALID;
        }
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        for (uint32_t i = 0; i < n_cases; i++) taken_out[i] = node_step4_host(q[cases[i].node], cases[i], host_rcp_ulps);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    WideNodeQ* d_nodes = nullptr;
    StepCase* d_cases = nullptr;
    uint8_t* d_taken = nullptr;
    int rc = JPT_OK;
    if ((e = hipMalloc((void**)&d_nodes, (size_t)n_nodes * sizeof(WideNodeQ))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && n_cases && (e = hipMalloc((void**)&d_cases, (size_t)n_cases * sizeof(StepCase))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && n_cases && (e = hipMalloc((void**)&d_taken, n_cases)) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMemcpy(d_nodes, q.data(), (size_t)n_nodes * sizeof(WideNodeQ), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && n_cases) {
        if ((e = hipMemcpy(d_cases, cases, (size_t)n_cases * sizeof(StepCase), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
        if (rc == JPT_OK) {
            hipLaunchKernelGGL(node_step4_probe, dim3((n_cases + 255u) / 256u), dim3(256), 0, nullptr, d_nodes, d_cases, n_cases, d_taken);
            if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "node_step4_probe");
        }
        if (rc == JPT_OK && (e = hipMemcpy(taken_out, d_taken, n_cases, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    }
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_cases) (void)hipFree(d_cases);
    if (d_taken) (void)hipFree(d_taken);
    return rc;
}

int jpt_debug_env_lookup(int device_id, const float* rgb, int32_t width, int32_t height, const float* rotation9, float intensity,
                         const float* dirs3, uint32_t n, float* rgb_out)
{
    if (!rgb || (n && (!dirs3 || !rgb_out))) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    int rc = check_env_map(rgb, width, height, g_debug_error);
    if (rc == JPT_OK) rc = check_env_params(rotation9, intensity, g_debug_error);
    if (rc != JPT_OK) return rc;
    std::vector<float4> texels;
    pack_env_texels(rgb, width, height, texels);
    EnvDev env;
    env.w = width;
    env.h = height;
    static const float kIdentity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    std::memcpy(env.rot, rotation9 ? rotation9 : kIdentity, sizeof env.rot);
    env.intensity = intensity;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        env.texels = texels.data();
        for (uint32_t i = 0; i < n; i++) {
            const f3 c = env_radiance(env, f3{dirs3[3 * (size_t)i], dirs3[3 * (size_t)i + 1], dirs3[3 * (size_t)i + 2]});
            rgb_out[3 * (size_t)i] = c.x;
            rgb_out[3 * (size_t)i + 1] = c.y;
            rgb_out[3 * (size_t)i + 2] = c.z;
        }
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (n == 0) return JPT_OK;
    float4* d_tex = nullptr;
    float *d_dirs = nullptr, *d_out = nullptr;
    const size_t vec_bytes = (size_t)n * 3u * sizeof(float);
    if ((e = hipMalloc((void**)&d_tex, texels.size() * sizeof(float4))) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMalloc((void**)&d_dirs, vec_bytes)) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMalloc((void**)&d_out, vec_bytes)) != hipSuccess) rc = hip_fail(e, "hipMalloc");
    if (rc == JPT_OK && (e = hipMemcpy(d_tex, texels.data(), texels.size() * sizeof(float4), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_dirs, dirs3, vec_bytes, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        env.texels = d_tex;
        hipLaunchKernelGGL(env_lookup_probe, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, env, d_dirs, n, d_out);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "env_lookup_probe");
    }
    if (rc == JPT_OK && (e = hipMemcpy(rgb_out, d_out, vec_bytes, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (d_tex) (void)hipFree(d_tex);
    if (d_dirs) (void)hipFree(d_dirs);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

int jpt_debug_dielectric(int device_id, const float* normals3, const float* out_dirs3, const float* ior, const uint8_t* front, const float* xi_f,
                         uint32_t n, float* dirs_out, float* fresnel_out, uint8_t* event_out)
{
    if (n && (!normals3 || !out_dirs3 || !ior || !front || !xi_f || !dirs_out || !fresnel_out || !event_out)) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        for (uint32_t i = 0; i < n; i++) {
            f3 d;
            const int ev = dielectric_event(f3{normals3[3 * (size_t)i], normals3[3 * (size_t)i + 1], normals3[3 * (size_t)i + 2]},
                                            f3{out_dirs3[3 * (size_t)i], out_dirs3[3 * (size_t)i + 1], out_dirs3[3 * (size_t)i + 2]}, ior[i],
                                            front[i] != 0, xi_f[i], d, fresnel_out[i]);
            dirs_out[3 * (size_t)i] = d.x;
            dirs_out[3 * (size_t)i + 1] = d.y;
            dirs_out[3 * (size_t)i + 2] = d.z;
            event_out[i] = (uint8_t)ev;
        }
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (n == 0) return JPT_OK;
    // one allocation: normals, out directions, directions out (3 n floats each), ior, xi_f, fresnel out (n each), front, event out (n bytes each)
    const size_t f = (size_t)n * sizeof(float);
    char* d_all = nullptr;
    int rc = JPT_OK;
    if ((e = hipMalloc((void**)&d_all, 12 * f + 2 * (size_t)n)) != hipSuccess) return hip_fail(e, "hipMalloc");
    float *d_n = (float*)d_all, *d_v = d_n + 3 * (size_t)n, *d_d = d_v + 3 * (size_t)n, *d_ior = d_d + 3 * (size_t)n, *d_xi = d_ior + n, *d_f = d_xi + n;
    uint8_t *d_front = (uint8_t*)(d_f + n), *d_ev = d_front + n;
    if ((e = hipMemcpy(d_n, normals3, 3 * f, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_v, out_dirs3, 3 * f, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_ior, ior, f, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_xi, xi_f, f, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_front, front, n, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        hipLaunchKernelGGL(dielectric_probe, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, d_n, d_v, d_ior, d_front, d_xi, n, d_d, d_f, d_ev);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "dielectric_probe");
    }
    if (rc == JPT_OK && (e = hipMemcpy(dirs_out, d_d, 3 * f, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(fresnel_out, d_f, f, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(event_out, d_ev, n, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_lens_rays(int device_id, const void* camera160, int32_t width, int32_t height, uint32_t frame_index, float aperture_radius,
                        float focus_distance, float* origins3_out, float* dirs3_out)
{
    if (!camera160 || !origins3_out || !dirs3_out) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) {
        g_debug_error = "jpt_debug_lens_rays: width and height must be in 1..65535";
        return JPT_E_INVALID;
    }
    const int rc0 = check_lens(aperture_radius, focus_distance, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    RefCamera cam;
    std::memcpy(&cam, camera160, sizeof cam);
    PrimaryRays p;
    if (aperture_radius > 0.0f) {
        p.kind = PrimaryRays::kLens;
        p.lens.radius = aperture_radius;
        p.lens.focus = focus_distance;
        if (!lens_basis(cam, p.lens)) {
            g_debug_error = "the camera basis derived from camera160 is not finite";
            return JPT_E_STATE;
        }
    }
    return primary_rays_debug(device_id, "lens_rays_probe", p, cam, width, height, frame_index, origins3_out, dirs3_out, nullptr);
}

int jpt_debug_camera_rays(int device_id, const void* camera160, int32_t width, int32_t height, uint32_t frame_index, int32_t model,
                          float* origins3_out, float* dirs3_out)
{
    if (!camera160 || !origins3_out || !dirs3_out) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) {
        g_debug_error = "jpt_debug_camera_rays: width and height must be in 1..65535";
        return JPT_E_INVALID;
    }
    RefCamera cam;
    std::memcpy(&cam, camera160, sizeof cam);
    PrimaryRays p;
    const int rc0 = make_camera_model(model, cam, p.cam_model, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    if (p.cam_model.model != kCamPinhole) p.kind = PrimaryRays::kCamModel;
    return primary_rays_debug(device_id, "camera_rays_probe", p, cam, width, height, frame_index, origins3_out, dirs3_out, nullptr);
}

int jpt_debug_bake_rays(int device_id, const float* position4, const float* normal4, int32_t width, int32_t height, uint32_t frame_index,
                        float* origins3_out, float* dirs3_out, uint8_t* valid_out)
{
    if (!position4 || !normal4 || !origins3_out || !dirs3_out || !valid_out) {
        g_debug_error = "jpt_debug_bake_rays: null argument";
        return JPT_E_INVALID;
    }
    const int rc0 = check_bake_size("jpt_debug_bake_rays", width, height, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    PrimaryRays p;   // (the images are host memory here: primary_rays_debug uploads them for a device)
    p.kind = PrimaryRays::kBake;
    p.bake.position = reinterpret_cast<const float4*>(position4);
    p.bake.normal = reinterpret_cast<const float4*>(normal4);
    return primary_rays_debug(device_id, "bake_rays_probe", p, RefCamera{}, width, height, frame_index, origins3_out, dirs3_out, valid_out);
}

int jpt_debug_probe_rays(int device_id, const float* position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row,
                         uint32_t frame_index, float* origins3_out, float* dirs3_out, uint8_t* valid_out)
{
    if (!position3 || !origins3_out || !dirs3_out || !valid_out) {
        g_debug_error = "jpt_debug_probe_rays: null argument";
        return JPT_E_INVALID;
    }
    const int rc0 = check_probes("jpt_debug_probe_rays", position3, n_probes, tile_w, tile_h, probes_per_row, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    uint64_t w, h;
    probe_image_size(n_probes, tile_w, tile_h, probes_per_row, w, h);
    PrimaryRays p;   // (the positions are host memory here: primary_rays_debug uploads them for a device)
    p.kind = PrimaryRays::kProbe;
    p.probe = make_probe_dev(position3, n_probes, tile_w, tile_h, probes_per_row);
    return primary_rays_debug(device_id, "probe_rays_probe", p, RefCamera{}, (int32_t)w, (int32_t)h, frame_index, origins3_out, dirs3_out, valid_out);
}

int jpt_debug_probe_basis(int32_t tile_w, int32_t tile_h, int32_t flags, float* table_out)
{
    if (!table_out) {
        g_debug_error = "jpt_debug_probe_basis: null argument";
        return JPT_E_INVALID;
    }
    if (flags != JPT_PROBE_RADIANCE && flags != JPT_PROBE_IRRADIANCE) {
        g_debug_error = "jpt_debug_probe_basis: flags must be JPT_PROBE_RADIANCE or JPT_PROBE_IRRADIANCE";
        return JPT_E_INVALID;
    }
    const int rc0 = check_probes("jpt_debug_probe_basis", nullptr, 1, tile_w, tile_h, 1, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    std::vector<float> table;
    probe_basis_table(tile_w, tile_h, flags, table);
    std::memcpy(table_out, table.data(), table.size() * sizeof(float));
    return JPT_OK;
}

int jpt_debug_probe_project(int device_id, const float* accum4, uint32_t frame_count, int32_t n_probes, int32_t tile_w, int32_t tile_h,
                            int32_t probes_per_row, const float* table, float* sh_out)
{
    if (!accum4 || !table || !sh_out) {
        g_debug_error = "jpt_debug_probe_project: null argument";
        return JPT_E_INVALID;
    }
    if (frame_count == 0) {
        g_debug_error = "jpt_debug_probe_project: frame_count must be >= 1";
        return JPT_E_INVALID;
    }
    int rc = check_probes("jpt_debug_probe_project", nullptr, n_probes, tile_w, tile_h, probes_per_row, g_debug_error);
    if (rc != JPT_OK) return rc;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        probe_project_host(accum4, frame_count, n_probes, tile_w, tile_h, probes_per_row, table, sh_out);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    uint64_t w, h;
    probe_image_size(n_probes, tile_w, tile_h, probes_per_row, w, h);
    const size_t b_img = (size_t)(w * h) * sizeof(float4), b_sh = (size_t)n_probes * 9 * sizeof(float4), b_tab = (size_t)tile_w * tile_h * 9 * sizeof(float);
    char* d_all = nullptr;   // the accumulation image, the coefficients (16-byte data first), the table
    if ((e = hipMalloc((void**)&d_all, b_img + b_sh + b_tab)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = hipMemcpy(d_all, accum4, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_all + b_img + b_sh, table, b_tab, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_probe_project(nullptr, make_probe_dev(nullptr, n_probes, tile_w, tile_h, probes_per_row), reinterpret_cast<const float4*>(d_all), (float)frame_count,
                             reinterpret_cast<const float*>(d_all + b_img + b_sh), reinterpret_cast<float4*>(d_all + b_img));
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "probe_project_kernel");
    }
    if (rc == JPT_OK && (e = hipMemcpy(sh_out, d_all + b_img, b_sh, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_cube_rays(int device_id, const float* position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row, uint32_t frame_index,
                        float* rays_out)
{
    if (!position3 || !rays_out) {
        g_debug_error = "jpt_debug_cube_rays: null argument";
        return JPT_E_INVALID;
    }
    const int rc0 = check_reflection_probes("jpt_debug_cube_rays", position3, n_probes, face_size, probes_per_row, g_debug_error);
    if (rc0 != JPT_OK) return rc0;
    uint64_t w, h;
    cube_image_size(n_probes, face_size, probes_per_row, w, h);
    PrimaryRays p;   // (the positions are host memory here: primary_rays_debug uploads them for a device)
    p.kind = PrimaryRays::kCube;
    p.cube = make_cube_dev(position3, n_probes, face_size, probes_per_row);
    const size_t n = (size_t)(w * h);
    std::vector<float> o(3 * n), d(3 * n);
    const int rc = primary_rays_debug(device_id, "cube_rays_probe", p, RefCamera{}, (int32_t)w, (int32_t)h, frame_index, o.data(), d.data(), nullptr);
    if (rc != JPT_OK) return rc;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            rays_out[6 * i + k] = o[3 * i + k];
            rays_out[6 * i + 3 + k] = d[3 * i + k];
        }
    return JPT_OK;
}

int jpt_debug_reflection_samples(int32_t face_size, int32_t n_levels, int32_t samples, int32_t level, float* table_out, uint8_t* src_level_out)
{
    if (!table_out || !src_level_out) {
        g_debug_error = "jpt_debug_reflection_samples: null argument";
        return JPT_E_INVALID;
    }
    int rc = check_reflection_probes("jpt_debug_reflection_samples", nullptr, 1, face_size, 1, g_debug_error);
    if (rc == JPT_OK) rc = check_reflection_params("jpt_debug_reflection_samples", n_levels, samples, face_size, g_debug_error);
    if (rc != JPT_OK) return rc;
    if (n_levels == 0) n_levels = cube_log2(face_size) + 1;
    if (level < 1 || level >= n_levels) {
        g_debug_error = "jpt_debug_reflection_samples: level must be in [1, n_levels): level 0 is a copy and has no samples";
        return JPT_E_INVALID;
    }
    std::vector<float4> table;
    std::vector<uint8_t> levels;
    uint32_t count[kReflLevelsMax];
    reflection_sample_table(face_size, n_levels, samples, table, levels, count);
    std::memcpy(table_out, &table[(size_t)level * samples], (size_t)samples * sizeof(float4));
    std::memcpy(src_level_out, &levels[(size_t)level * samples], (size_t)samples);
    return JPT_OK;
}

int jpt_debug_reflection_prefilter(int device_id, const float* accum4, uint32_t frame_count, int32_t n_probes, int32_t face_size, int32_t probes_per_row,
                                   const jpt_reflection_params* params, int32_t level, float* out)
{
    if (!accum4 || !out) {
        g_debug_error = "jpt_debug_reflection_prefilter: null argument";
        return JPT_E_INVALID;
    }
    if (frame_count == 0) {
        g_debug_error = "jpt_debug_reflection_prefilter: frame_count must be >= 1";
        return JPT_E_INVALID;
    }
    int rc = check_reflection_probes("jpt_debug_reflection_prefilter", nullptr, n_probes, face_size, probes_per_row, g_debug_error);
    if (rc != JPT_OK) return rc;
    int32_t n_levels = params ? params->n_levels : 0;
    const int32_t samples = params ? params->samples : kReflSamplesDefault;
    rc = check_reflection_params("jpt_debug_reflection_prefilter", n_levels, samples, face_size, g_debug_error);
    if (rc != JPT_OK) return rc;
    if (n_levels == 0) n_levels = cube_log2(face_size) + 1;
    if (level < 0 || level >= n_levels) {
        g_debug_error = "jpt_debug_reflection_prefilter: level must be in [0, n_levels)";
        return JPT_E_INVALID;
    }
    ReflDev rd;
    rd.n = (uint32_t)n_probes;
    rd.per_row = (uint32_t)probes_per_row;
    rd.shift = (uint32_t)cube_log2(face_size);
    rd.n_levels = (uint32_t)n_levels;
    rd.samples = (uint32_t)samples;
    std::vector<float4> table;
    std::vector<uint8_t> levels;
    reflection_sample_table(face_size, n_levels, samples, table, levels, rd.count);
    const size_t n_chain = (size_t)((uint64_t)rd.n * refl_probe_texels(rd.shift)), n_out = (size_t)refl_out_texels(rd.n, rd.shift, rd.n_levels);
    const size_t s = (size_t)(face_size >> level), n_level = (size_t)n_probes * 6u * s * s, at = (size_t)refl_out_offset(rd.n, rd.shift, (uint32_t)level);
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        std::vector<float4> chain(n_chain), all(n_out);
        reflection_prefilter_host(accum4, frame_count, rd, table.data(), levels.data(), chain.data(), all.data());
        std::memcpy(out, &all[at], n_level * sizeof(float4));
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    uint64_t w, h;
    cube_image_size(n_probes, face_size, probes_per_row, w, h);
    const size_t b_img = (size_t)(w * h) * sizeof(float4), b_chain = n_chain * sizeof(float4), b_out = n_out * sizeof(float4), b_tab = table.size() * sizeof(float4);
    char* d_all = nullptr;   // the accumulation image, the source chain, the output chain, the entries (16-byte data first), the level bytes
    if ((e = hipMalloc((void**)&d_all, b_img + b_chain + b_out + b_tab + levels.size())) != hipSuccess) return hip_fail(e, "hipMalloc");
    float4* d_chain = reinterpret_cast<float4*>(d_all + b_img);
    float4* d_out = reinterpret_cast<float4*>(d_all + b_img + b_chain);
    float4* d_tab = reinterpret_cast<float4*>(d_all + b_img + b_chain + b_out);
    uint8_t* d_lvl = reinterpret_cast<uint8_t*>(d_all + b_img + b_chain + b_out + b_tab);
    if ((e = hipMemcpy(d_all, accum4, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_tab, table.data(), b_tab, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_lvl, levels.data(), levels.size(), hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_reflection_chain(nullptr, rd, reinterpret_cast<const float4*>(d_all), (float)frame_count, d_chain);
        launch_reflection_prefilter(nullptr, rd, d_chain, d_tab, d_lvl, d_out);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "refl_prefilter_kernel");
    }
    if (rc == JPT_OK && (e = hipMemcpy(out, d_out + at, n_level * sizeof(float4), hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_skin(int device_id, const float* bind_positions3, const float* bind_normals3, uint32_t n_vertices, const int32_t* bones, const float* weights,
                   int32_t influences, const float* position_deltas, const float* normal_deltas, int32_t n_blend_shapes, const float* bone_transforms12,
                   uint32_t n_bones, const float* blend_weights, float* positions3_out, float* normals3_out)
{
    if (!bind_positions3 || !positions3_out || (bind_normals3 && !normals3_out) || n_vertices == 0 || n_vertices > 0x7fffffffu) {
        g_debug_error = "jpt_debug_skin: null argument or no vertices";
        return JPT_E_INVALID;
    }
    SkinPiece piece;
    piece.n_vertices = (int32_t)n_vertices;
    piece.positions = bind_positions3;
    piece.normals = bind_normals3;
    piece.bones = bones;
    piece.weights = weights;
    piece.dpos = position_deltas;
    piece.dnrm = normal_deltas;
    SkinRigInfo info;
    int rc = check_skin_rig("jpt_debug_skin", &piece, 1, influences, n_blend_shapes, bind_normals3 != nullptr, info, g_debug_error);
    if (rc != JPT_OK) return rc;
    std::vector<SkinShape> active;
    rc = check_skin_pose("jpt_debug_skin", info, bone_transforms12, n_bones, blend_weights, (uint32_t)n_blend_shapes, active, g_debug_error);
    if (rc != JPT_OK) return rc;
    std::vector<char> block(info.bytes);
    pack_skin_rig(info, &piece, 1, block.data());
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        skin_host(skin_rig_view(info, block.data()), influences, active.data(), (uint32_t)active.size(), bone_transforms12, positions3_out, normals3_out);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    // one block: the rig, the palette, the active shapes, the outputs -- every part 16-byte aligned
    auto up16 = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
    const uint32_t n_pal = influences ? n_bones : 0u;
    const size_t b_pal = (size_t)n_pal * 48, b_act = up16(active.size() * sizeof(SkinShape)), b_out = up16((size_t)n_vertices * 3 * sizeof(float));
    const size_t o_pal = info.bytes, o_act = o_pal + b_pal, o_pos = o_act + b_act, o_nrm = o_pos + b_out, total = o_nrm + (bind_normals3 ? b_out : 0);
    char* d_all = nullptr;
    if ((e = hipMalloc((void**)&d_all, total)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = hipMemcpy(d_all, block.data(), info.bytes, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && b_pal && (e = hipMemcpy(d_all + o_pal, bone_transforms12, b_pal, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && !active.empty() && (e = hipMemcpy(d_all + o_act, active.data(), active.size() * sizeof(SkinShape), hipMemcpyHostToDevice)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        SkinArgs a;
        a.rig = skin_rig_view(info, d_all);
        a.influences = influences;
        a.palette = reinterpret_cast<const float*>(d_all + o_pal);
        a.n_bones = n_pal;
        a.active = reinterpret_cast<const SkinShape*>(d_all + o_act);
        a.n_active = (uint32_t)active.size();
        a.verts_out = reinterpret_cast<float*>(d_all + o_pos);
        a.normals_out = bind_normals3 ? reinterpret_cast<float*>(d_all + o_nrm) : nullptr;
        launch_mesh_skin(nullptr, a);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "mesh_skin_kernel");
    }
    if (rc == JPT_OK && (e = hipMemcpy(positions3_out, d_all + o_pos, (size_t)n_vertices * 3 * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && bind_normals3 && (e = hipMemcpy(normals3_out, d_all + o_nrm, (size_t)n_vertices * 3 * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_encode(int device_id, const float* src4, uint64_t n_texels, float divisor, int32_t alpha_one, int32_t format, void* out)
{
    if (!encode_format_known(format)) {
        g_debug_error = "jpt_debug_encode: format must be JPT_ENCODE_RGBA16F, _RGB9E5 or _RGBE8";
        return JPT_E_INVALID;
    }
    if (!std::isfinite(divisor) || !(divisor > 0.0f)) {
        g_debug_error = "jpt_debug_encode: divisor must be finite and > 0";
        return JPT_E_INVALID;
    }
    if (n_texels == 0) return JPT_OK;
    if (!src4 || !out) {
        g_debug_error = "jpt_debug_encode: null argument";
        return JPT_E_INVALID;
    }
    if (n_texels > (1ull << 30)) {
        g_debug_error = "jpt_debug_encode: more than 2^30 texels";
        return JPT_E_LIMIT;
    }
    const float4* src = reinterpret_cast<const float4*>(src4);
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        encode_host(format, src, n_texels, divisor, alpha_one != 0, out);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    const size_t b_in = (size_t)n_texels * sizeof(float4), b_out = (size_t)n_texels * encode_texel_bytes(format);
    char* d_all = nullptr;   // the texels, then the encoded texels (both 16-byte aligned)
    if ((e = hipMalloc((void**)&d_all, b_in + b_out)) != hipSuccess) return hip_fail(e, "hipMalloc");
    int rc = JPT_OK;
    if ((e = hipMemcpy(d_all, src4, b_in, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_encode(nullptr, format, reinterpret_cast<const float4*>(d_all), n_texels, divisor, alpha_one != 0, d_all + b_in);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "encode_kernel");
    }
    if (rc == JPT_OK && (e = hipMemcpy(out, d_all + b_in, b_out, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_bake_raster(int device_id, const jpt_surface* surface, const float* uv2, const float* transform12, int32_t width, int32_t height,
                          float* position4_out, float* normal4_out)
{
    if (!surface || !position4_out || !normal4_out) {
        g_debug_error = "jpt_debug_bake_raster: null argument";
        return JPT_E_INVALID;
    }
    int rc = check_bake_size("jpt_debug_bake_raster", width, height, g_debug_error);
    if (rc == JPT_OK)
        rc = check_bake_surface("jpt_debug_bake_raster", surface->vertices, surface->normals, surface->indices, surface->n_vertices, surface->n_indices, uv2,
                                transform12, g_debug_error);
    if (rc != JPT_OK) return rc;
    const size_t n = (size_t)width * (size_t)height, b_img = n * sizeof(float4);
    std::memset(position4_out, 0, b_img);
    std::memset(normal4_out, 0, b_img);
    BakeSurfaceDev sd;
    sd.n_tris = (uint32_t)(surface->n_indices / 3);
    transform12_to_mat16(transform12, sd.transform);
    if (sd.n_tris == 0) return JPT_OK;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        sd.vertices = surface->vertices;
        sd.normals = surface->normals;
        sd.uv2 = uv2;
        sd.indices = surface->indices;
        bake_raster_host(sd, width, height, reinterpret_cast<float4*>(position4_out), reinterpret_cast<float4*>(normal4_out));
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    const size_t nv = (size_t)surface->n_vertices;
    const size_t b_v = nv * 3 * sizeof(float), b_uv = nv * 2 * sizeof(float), b_i = (size_t)sd.n_tris * 3 * sizeof(int32_t), b_win = n * sizeof(uint32_t);
    char* d_all = nullptr;   // position4, normal4, winner, vertices, normals, uv2, indices (16-byte images first)
    if ((e = hipMalloc((void**)&d_all, 2 * b_img + b_win + 2 * b_v + b_uv + b_i)) != hipSuccess) return hip_fail(e, "hipMalloc");
    char* d_in = d_all + 2 * b_img + b_win;
    if ((e = hipMemset(d_all, 0, 2 * b_img)) != hipSuccess) rc = hip_fail(e, "hipMemset");
    if (rc == JPT_OK && (e = hipMemcpy(d_in, surface->vertices, b_v, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_in + b_v, surface->normals, b_v, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_in + 2 * b_v, uv2, b_uv, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(d_in + 2 * b_v + b_uv, surface->indices, b_i, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        sd.vertices = reinterpret_cast<const float*>(d_in);
        sd.normals = reinterpret_cast<const float*>(d_in + b_v);
        sd.uv2 = reinterpret_cast<const float*>(d_in + 2 * b_v);
        sd.indices = reinterpret_cast<const int32_t*>(d_in + 2 * b_v + b_uv);
        launch_bake_raster(nullptr, sd, width, height, reinterpret_cast<uint32_t*>(d_all + 2 * b_img), reinterpret_cast<float4*>(d_all),
                           reinterpret_cast<float4*>(d_all + b_img));
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "bake raster kernels");
    }
    if (rc == JPT_OK && (e = hipMemcpy(position4_out, d_all, b_img, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(normal4_out, d_all + b_img, b_img, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

// the whole transform on the host (jpt_debug_bake_finish with JPT_DEVICE_HOST_ONLY): out = (r, g, b, coverage)
static void lightmap_finish_host(int32_t width, int32_t height, const LightmapParams& prm, const float4* mean4, const float4* position4,
                                 const float4* normal4, float4* out)
{
    const size_t n = (size_t)width * height;
    std::vector<float4> xg(n), ng(n), i0(n), scratch(n);
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const size_t ip = (size_t)y * width + x;
            lightmap_guides(position4, normal4, width, height, x, y, xg[ip], ng[ip]);
            i0[ip] = lightmap_colour0(mean4[ip], 1.0f, xg[ip]);
        }
    float sc = prm.sigma_color;
    float4* a = atrous_passes_host(prm.passes, width, height, xg.data(), ng.data(), i0.data(), scratch.data(), [&](int k) {
        const LightmapTaps taps{{1 << k, prm.normal_power_log2, prm.sigma_distance * prm.sigma_distance, prm.sigma_plane * prm.sigma_plane, sc * sc}};
        sc = sc * 0.5f;
        return taps;
    });
    float4* b = a == i0.data() ? scratch.data() : i0.data();
    for (int k = 0; k < prm.dilate; k++) {
        for (int32_t y = 0; y < height; y++)
            for (int32_t x = 0; x < width; x++) b[(size_t)y * width + x] = lightmap_dilate(a, width, height, x, y);
        float4* t = a;
        a = b;
        b = t;
    }
    for (size_t i = 0; i < n; i++) out[i] = a[i];
}

int jpt_debug_bake_finish(int device_id, int32_t width, int32_t height, const jpt_bake_finish_params* params, const float* mean4,
                          const float* position4, const float* normal4, float* out)
{
    if (!mean4 || !position4 || !normal4 || !out) {
        g_debug_error = "jpt_debug_bake_finish: null argument";
        return JPT_E_INVALID;
    }
    LightmapParams prm;
    if (params) {
        prm.passes = params->passes;
        prm.normal_power_log2 = params->normal_power_log2;
        prm.dilate = params->dilate;
        prm.sigma_distance = params->sigma_distance;
        prm.sigma_plane = params->sigma_plane;
        prm.sigma_color = params->sigma_color;
    }
    int rc = check_bake_finish_params("jpt_debug_bake_finish", prm, g_debug_error);
    if (rc == JPT_OK) rc = check_bake_size("jpt_debug_bake_finish", width, height, g_debug_error);
    const size_t n = (size_t)width * (size_t)height, b_img = n * sizeof(float4);
    if (rc == JPT_OK) rc = check_bake_texels("jpt_debug_bake_finish", position4, normal4, n, g_debug_error);
    if (rc != JPT_OK) return rc;
    if (device_id == JPT_DEVICE_HOST_ONLY) {
        lightmap_finish_host(width, height, prm, reinterpret_cast<const float4*>(mean4), reinterpret_cast<const float4*>(position4),
                             reinterpret_cast<const float4*>(normal4), reinterpret_cast<float4*>(out));
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    float4* buf = nullptr;   // mean, position4, normal4, xg, ng, ping, pong
    if ((e = hipMalloc((void**)&buf, 7 * b_img)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = hipMemcpy(buf, mean4, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(buf + n, position4, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(buf + 2 * n, normal4, b_img, hipMemcpyHostToDevice)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        const float4* result = launch_lightmap_finish(nullptr, prm, width, height, buf, 1.0f, buf + n, buf + 2 * n, buf + 3 * n, buf + 4 * n, buf + 5 * n, buf + 6 * n);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "bake finish kernels");
        if (rc == JPT_OK && (e = hipMemcpy(out, result, b_img, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    }
    (void)hipFree(buf);
    return rc;
}

int jpt_debug_lens_sample(const void* camera160, float aperture_radius, float focus_distance, const float* origins3, const float* dirs3,
                          const float* xi2, uint32_t n, float* origins3_out, float* dirs3_out, float* basis9_out)
{
    if (!camera160 || (n && (!origins3 || !dirs3 || !xi2 || !origins3_out || !dirs3_out))) {
        g_debug_error = "null argument";
        return JPT_E_INVALID;
    }
    RefCamera cam;
    std::memcpy(&cam, camera160, sizeof cam);
    LensDev lens;
    lens.radius = aperture_radius;
    lens.focus = focus_distance;
    const bool finite = lens_basis(cam, lens);
    if (basis9_out) {
        const float b[9] = {lens.f.x, lens.f.y, lens.f.z, lens.r.x, lens.r.y, lens.r.z, lens.u.x, lens.u.y, lens.u.z};
        std::memcpy(basis9_out, b, sizeof b);
    }
    if (!finite) {
        g_debug_error = "the camera basis derived from camera160 is not finite";
        return JPT_E_STATE;
    }
    for (uint32_t i = 0; i < n; i++) {
        Ray ray;
        ray.o = f3{origins3[3 * (size_t)i], origins3[3 * (size_t)i + 1], origins3[3 * (size_t)i + 2]};
        ray.d = f3{dirs3[3 * (size_t)i], dirs3[3 * (size_t)i + 1], dirs3[3 * (size_t)i + 2]};
        ray.rD = rcp3(ray.d);
        lens_apply(lens, xi2[2 * (size_t)i], xi2[2 * (size_t)i + 1], ray);
        origins3_out[3 * (size_t)i] = ray.o.x;
        origins3_out[3 * (size_t)i + 1] = ray.o.y;
        origins3_out[3 * (size_t)i + 2] = ray.o.z;
        dirs3_out[3 * (size_t)i] = ray.d.x;
        dirs3_out[3 * (size_t)i + 1] = ray.d.y;
        dirs3_out[3 * (size_t)i + 2] = ray.d.z;
    }
    return JPT_OK;
}

int jpt_debug_env_tables(int device_id, const float* rgb, int32_t width, int32_t height, float* cond_out, float* marg_out, float* total_out)
{
    return env_sampling_debug(device_id, rgb, width, height, nullptr, 0, nullptr, 0, nullptr, nullptr, cond_out, marg_out, total_out);
}

int jpt_debug_env_sample(int device_id, const float* rgb, int32_t width, int32_t height, const float* rotation9, const float* xi2, uint32_t n,
                         float* dirs_out, float* pdf_out)
{
    return env_sampling_debug(device_id, rgb, width, height, rotation9, 1, xi2, n, dirs_out, pdf_out, nullptr, nullptr, nullptr);
}

int jpt_debug_env_pdf(int device_id, const float* rgb, int32_t width, int32_t height, const float* rotation9, const float* dirs3, uint32_t n,
                      float* pdf_out)
{
    return env_sampling_debug(device_id, rgb, width, height, rotation9, 2, dirs3, n, nullptr, pdf_out, nullptr, nullptr, nullptr);
}

int jpt_debug_tlas_order(int device_id, const float* lo3, const float* hi3, uint32_t n, uint64_t* keys_out, uint32_t* sorted_instances_out)
{
    if (n == 0) return JPT_OK;
    if (!lo3 || !hi3 || !sorted_instances_out) {
        g_debug_error = "jpt_debug_tlas_order: null argument";
        return JPT_E_INVALID;
    }
    if (n > kTlasRebuildMaxInstances) {
        g_debug_error = "jpt_debug_tlas_order: more than 32767 instances";
        return JPT_E_LIMIT;
    }
    if (device_id < 0) {
        tlas_order_host(lo3, hi3, 3, n, keys_out, sorted_instances_out);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the keys (n), the sort's two buffers (2 n), the boxes (6 n floats), the order (n words)
    const size_t b_keys = (size_t)n * 8, b_box = (size_t)n * 12;
    char* d_all = nullptr;
    if ((e = hipMalloc((void**)&d_all, 3 * b_keys + 2 * b_box + (size_t)n * 4)) != hipSuccess) return hip_fail(e, "hipMalloc");
    uint64_t* d_keys = reinterpret_cast<uint64_t*>(d_all);
    float* d_lo = reinterpret_cast<float*>(d_all + 3 * b_keys);
    float* d_hi = reinterpret_cast<float*>(d_all + 3 * b_keys + b_box);
    uint32_t* d_sorted = reinterpret_cast<uint32_t*>(d_all + 3 * b_keys + 2 * b_box);
    int rc = JPT_OK;
    if ((e = hipMemcpy(d_lo, lo3, b_box, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_hi, hi3, b_box, hipMemcpyHostToDevice)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_tlas_order(nullptr, d_lo, d_hi, 3, n, d_keys, d_keys + n, d_sorted);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "tlas_order_kernel");
    }
    if (rc == JPT_OK && keys_out && (e = hipMemcpy(keys_out, d_keys, b_keys, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK && (e = hipMemcpy(sorted_instances_out, d_sorted, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_mesh_order(int device_id, const float* vertices3, uint32_t n_vertices, const uint32_t* indices, uint32_t n_tris, uint32_t* codes_out,
                         uint32_t* sorted_tris_out)
{
    if (n_tris == 0) return JPT_OK;
    if (!vertices3 || !indices || !sorted_tris_out) {
        g_debug_error = "jpt_debug_mesh_order: null argument";
        return JPT_E_INVALID;
    }
    if (n_tris > kMeshRebuildMaxTris) {
        g_debug_error = "jpt_debug_mesh_order: more than 2^25 triangles";
        return JPT_E_LIMIT;
    }
    for (size_t k = 0; k < (size_t)n_tris * 3; k++)
        if (indices[k] >= n_vertices) {
            g_debug_error = "jpt_debug_mesh_order: a triangle names a vertex beyond n_vertices";
            return JPT_E_INVALID;
        }
    if (device_id < 0) {
        mesh_order_host(vertices3, indices, n_tris, codes_out, sorted_tris_out);
        return JPT_OK;
    }
    auto hip_fail = [](hipError_t e, const char* what) {
        g_debug_error = std::string(what) + ": " + hipGetErrorString(e);
        return JPT_E_DEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the vertices, the indices, the sort's working set
    const size_t b_verts = (size_t)n_vertices * 12, b_idx = (size_t)n_tris * 12, b_work = mesh_sort_words(n_tris) * 4;
    char* d_all = nullptr;
    if ((e = hipMalloc((void**)&d_all, b_verts + b_idx + b_work)) != hipSuccess) return hip_fail(e, "hipMalloc");
    MeshOrderArgs a;
    a.verts = reinterpret_cast<const float*>(d_all);
    a.vidx = reinterpret_cast<const uint32_t*>(d_all + b_verts);
    a.n_tris = n_tris;
    a.work = reinterpret_cast<uint32_t*>(d_all + b_verts + b_idx);
    int rc = JPT_OK;
    if ((e = hipMemcpy(d_all, vertices3, b_verts, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_all + b_verts, indices, b_idx, hipMemcpyHostToDevice)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_mesh_order_codes(nullptr, a);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "mesh_codes_kernel");
    }
    if (rc == JPT_OK && codes_out && (e = hipMemcpy(codes_out, mesh_order_codes(a), (size_t)n_tris * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail(e, "hipMemcpy");
    if (rc == JPT_OK) {
        launch_mesh_order_sort(nullptr, a);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "mesh_sort_scatter_kernel");
    }
    if (rc == JPT_OK && (e = hipMemcpy(sorted_tris_out, mesh_order_sorted(a), (size_t)n_tris * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d_all);
    return rc;
}

int jpt_debug_tlas_template(uint32_t n, int32_t* child_out, uint32_t capacity, uint32_t* n_records, uint32_t* n_levels, uint32_t* stack_need)
{
    if (n < 2 || n > kTlasRebuildMaxInstances) {
        g_debug_error = "jpt_debug_tlas_template: 2 .. 32767 instances";
        return JPT_E_INVALID;
    }
    TlasTemplate t;
    make_tlas_template(n, t);
    if (n_records) *n_records = t.n_records;
    if (n_levels) *n_levels = t.n_levels;
    if (stack_need) {
        std::vector<uint32_t> identity(n);
        for (uint32_t i = 0; i < n; i++) identity[i] = i;
        std::vector<WideNode4> records;
        tlas_template_records(t, identity.data(), records);
        *stack_need = stack_need4_under(records, 0);
    }
    if (child_out) {
        if (capacity < t.n_records) {
            g_debug_error = "jpt_debug_tlas_template: record buffer too small";
            return JPT_E_INVALID;
        }
        std::memcpy(child_out, t.child.data(), t.child.size() * sizeof(int32_t));
    }
    return JPT_OK;
}

}  // extern "C"
