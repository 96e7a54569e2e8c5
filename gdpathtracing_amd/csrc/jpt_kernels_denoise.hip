// jpt_kernels_denoise.hip -- jpt_denoise: the first-hit guide images and the edge-avoiding a-trous filter over the running mean.
// No reference counterpart (the reference lists a denoiser among its wanted features).  The arithmetic is pinned in
// jpt_denoise.h / DESIGN.md section 2; nothing here writes a buffer a render reads.
#include "../../include/jpt.h"
#include "jpt_atrous_pass.h"
#include "jpt_kernels.h"
#include "jpt_trace_core.h"

namespace jpt {

namespace {

// ---- guides -----------------------------------------------------------------------------------------------------------------
// One lane per pixel, one 8 x 8 tile per wave (ref_frame_kernel's tiling): the un-jittered ray through the pixel centre, the walk
// of the arrays the wavefront kernels walk stepped to its end with the whole stack in LDS (wf2_occlude's arrangement: one wave per
// block, no scratch), then the shading gather.  The closest hit is the walk's geometric answer -- the smallest accepted
// Moller-Trumbore t, no reach or tie logic.
constexpr int kGuideBlock = 64;
#include "jpt_guide_kernel.h"
#define JPT_CAMERA_MODEL 1
#include "jpt_guide_kernel.h"
#undef JPT_CAMERA_MODEL

// ---- filter -----------------------------------------------------------------------------------------------------------------
struct AtrousArgs {
    const float4* __restrict__ in;        // FIRST: the accumulation (sums); else i_k
    const float4* __restrict__ x;         // position_t
    const float4* __restrict__ n;         // normal
    const float4* __restrict__ albedo;    // read by the first pass (demodulation) and the last (remodulation)
    float4* __restrict__ out;             // i_k+1; LAST: the denoised image (r, g, b, 1)
    uint32_t* __restrict__ ldr;           // LAST: unorm8(ACES(denoised)) (may be null)
    int32_t width, height, step;
    float frame_count;                    // FIRST: what the sums are divided by
    AtrousTaps taps;
};

// what a pass reads and writes (atrous_pass' Filter): the first one demodulates the sums, the last one remodulates its result
template <bool FIRST, bool LAST>
struct AtrousFilter : AtrousArgs {
    static __device__ __forceinline__ float4 outside_x() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __device__ __forceinline__ float4 colour(size_t g, const float4&) const
    {
        const float4 v = in[g];
        if (!FIRST) return v;
        return atrous_demodulate(v, frame_count, albedo[g]);
    }
    __device__ __forceinline__ void write(size_t idx, const float4& r) const
    {
        if (LAST) atrous_write_last<false>(r, idx, albedo, out, nullptr, ldr);
        else out[idx] = r;
    }
};

// One pass (jpt_atrous_pass.h): tiled for HALO = 2 * step > 0, gathered for HALO = 0 (steps >= 4)
template <int HALO, bool FIRST, bool LAST>
__global__ __launch_bounds__(kAtrousBlock) void atrous_kernel(AtrousFilter<FIRST, LAST> f)
{
    atrous_pass<HALO>(f, f.width, f.height, f.step);
}

}  // namespace

void launch_guides(hipStream_t stream, const DeviceScene& ds, const RefCamera& cam, const CamModelDev& cm, int width, int height,
                   float4* position_t, float4* normal, float4* albedo)
{
    if (width <= 0 || height <= 0) return;
    const bool w4 = ds.use4;
    WideSceneDev sc;
    sc.blas_nodes = ds.blas_nodes;
    sc.tlas_nodes = ds.tlas_nodes;
    sc.nodesq = ds.nodesq;
    sc.tris = ds.wide_tris;
    sc.instances = w4 ? ds.wide_instances4 : ds.wide_instances;
    sc.tlas_root = w4 ? ds.tlas_root4 : ds.tlas_root;
    sc.n_instances = ds.n_instances;
    sc.reach_tri = ds.reach_tri;
    sc.reach_inst = ds.reach_inst;
    const SceneShading sh = ds.shading();
    const dim3 grid((unsigned)((width + 7) / 8), (unsigned)((height + 7) / 8)), block(kGuideBlock);
    if (cm.model != kCamPinhole) {   // (jpt_set_camera_model: the guides of the view the render took)
        if (w4) hipLaunchKernelGGL((guide_cam_kernel<true>), grid, block, 0, stream, sc, sh, cam, width, height, position_t, normal, albedo, cm);
        else hipLaunchKernelGGL((guide_cam_kernel<false>), grid, block, 0, stream, sc, sh, cam, width, height, position_t, normal, albedo, cm);
        return;
    }
    if (w4) hipLaunchKernelGGL((guide_kernel<true>), grid, block, 0, stream, sc, sh, cam, width, height, position_t, normal, albedo);
    else hipLaunchKernelGGL((guide_kernel<false>), grid, block, 0, stream, sc, sh, cam, width, height, position_t, normal, albedo);
}

void launch_atrous(hipStream_t stream, const AtrousParams& prm, int width, int height, const float4* sums, float frame_count,
                   const float4* position_t, const float4* normal, const float4* albedo, float4* ping, float4* pong, uint32_t* ldr)
{
    if (width <= 0 || height <= 0) return;
    AtrousArgs a = {};
    a.x = position_t;
    a.n = normal;
    a.albedo = albedo;
    a.ldr = ldr;
    a.width = width;
    a.height = height;
    a.frame_count = frame_count;
    float sc = prm.sigma_color;
    atrous_launch_passes(0, prm.passes, prm.passes, false, width, height, sums, ping, pong,
                         [&](auto halo, int k, const float4* src, float4* dst, bool last, dim3 grid, dim3 block) {
                             constexpr int HALO = decltype(halo)::value;
                             constexpr bool FIRST = HALO == 2;
                             a.in = src;
                             a.out = dst;
                             a.step = 1 << k;
                             a.taps = AtrousTaps{prm.normal_power_log2, prm.sigma_plane, sc * sc};
                             sc = sc * 0.5f;
                             if (last) hipLaunchKernelGGL((atrous_kernel<HALO, FIRST, true>), grid, block, 0, stream, AtrousFilter<FIRST, true>{a});
                             else hipLaunchKernelGGL((atrous_kernel<HALO, FIRST, false>), grid, block, 0, stream, AtrousFilter<FIRST, false>{a});
                         });
}

// the whole filter on the host (jpt_debug_atrous with JPT_DEVICE_HOST_ONLY): mean4 = (m.rgb, .) per pixel; out = (i_passes * amod, 1)
static void atrous_host(int32_t width, int32_t height, const AtrousParams& prm, const float4* mean4, const float4* position_t, const float4* normal,
                        const float4* albedo, float4* out)
{
    const size_t n = (size_t)width * height;
    std::vector<float4> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = atrous_demodulate(mean4[i], 1.0f, albedo[i]);
    float sc = prm.sigma_color;
    const float4* r = atrous_passes_host(prm.passes, width, height, position_t, normal, a.data(), b.data(), [&](int) {
        const AtrousTaps taps{prm.normal_power_log2, prm.sigma_plane, sc * sc};
        sc = sc * 0.5f;
        return taps;
    });
    for (size_t i = 0; i < n; i++) {
        const float4 am = atrous_amod(albedo[i]);
        out[i] = make_float4(r[i].x * am.x, r[i].y * am.y, r[i].z * am.z, 1.0f);
    }
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_atrous(int device, int32_t width, int32_t height, const jpt_denoise_params* params, const float* mean4,
                                const float* position_t, const float* normal, const float* albedo, float* out)
{
    if (!mean4 || !position_t || !normal || !albedo || !out || width <= 0 || height <= 0 || width > 65536 || height > 65536) return JPT_E_INVALID;
    const AtrousParams prm = denoise_params_of(params);
    std::string why;
    if (check_denoise_params(prm, why) != JPT_OK) return JPT_E_INVALID;
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    if (device == JPT_DEVICE_HOST_ONLY) {
        atrous_host(width, height, prm, reinterpret_cast<const float4*>(mean4), reinterpret_cast<const float4*>(position_t),
                    reinterpret_cast<const float4*>(normal), reinterpret_cast<const float4*>(albedo), reinterpret_cast<float4*>(out));
        return JPT_OK;
    }
    if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
    float4* buf = nullptr;   // mean, position_t, normal, albedo, ping, pong
    if (hipMalloc((void**)&buf, 6 * bytes) != hipSuccess) return JPT_E_DEVICE;
    bool ok = hipMemcpy(buf, mean4, bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(buf + n, position_t, bytes, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(buf + 2 * n, normal, bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(buf + 3 * n, albedo, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_atrous(nullptr, prm, width, height, buf, 1.0f, buf + n, buf + 2 * n, buf + 3 * n, buf + 4 * n, buf + 5 * n, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, buf + 4 * n, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(buf);
    return ok ? JPT_OK : JPT_E_DEVICE;
}
