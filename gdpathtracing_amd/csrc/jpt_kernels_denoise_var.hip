// jpt_kernels_denoise_var.hip -- jpt_denoise with jpt_set_denoise_variance on: the a-trous passes of jpt_kernels_denoise.hip with the
// colour weight measured against the variance of the mean, which travels through the passes in the .w of the colour.  No reference
// counterpart.  The arithmetic is pinned in jpt_denoise_var.h / DESIGN.md section 2; nothing here writes a buffer a render reads.
#include "../../include/jpt.h"
#include "jpt_atrous_pass.h"
#include "jpt_kernels.h"
#include "jpt_trace_core.h"

namespace jpt {

namespace {

// One pass (jpt_atrous_pass.h, whose AtrousVarFilter says what it reads and writes).  Tiled: the first pass demodulates and forms v_0
// while it stages, reading the plane once per staged pixel, and the prefilter reads the staged v.  Gathered: nine 4-byte loads of v.
template <int HALO, bool FIRST, bool LAST>
__global__ __launch_bounds__(kAtrousBlock) void atrous_var_kernel(AtrousVarFilter<FIRST, LAST> f)
{
    static_assert(HALO > 0 || !FIRST, "the first pass is a tiled one: the gather form reads v from the .w of its input");
    atrous_pass<HALO>(f, f.width, f.height, f.step);
}

}  // namespace

void launch_atrous_variance(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, int first_pass, const float4* src,
                            const float4* m2, uint32_t frame_count, const float4* position_t, const float4* normal, const float4* albedo, float4* ping,
                            float4* pong, uint32_t* ldr, float* var_out)
{
    if (width <= 0 || height <= 0) return;
    AtrousVarArgs a = atrous_var_args(prm, vprm, width, height, m2, frame_count, position_t, normal, albedo, ldr, var_out);
    atrous_launch_passes(first_pass, prm.passes, prm.passes, false, width, height, src, ping, pong,
                         [&](auto halo, int k, const float4* in, float4* out, bool last, dim3 grid, dim3 block) {
                             constexpr int HALO = decltype(halo)::value;
                             constexpr bool FIRST = HALO == 2;
                             a.in = in;
                             a.out = out;
                             a.step = 1 << k;
                             if (last) hipLaunchKernelGGL((atrous_var_kernel<HALO, FIRST, true>), grid, block, 0, stream, AtrousVarFilter<FIRST, true>{a});
                             else hipLaunchKernelGGL((atrous_var_kernel<HALO, FIRST, false>), grid, block, 0, stream, AtrousVarFilter<FIRST, false>{a});
                         });
}

// the whole filter on the host (jpt_debug_atrous_variance with JPT_DEVICE_HOST_ONLY): out = (i_passes * amod, 1), var_out = v_passes
static void atrous_var_host(int32_t width, int32_t height, const AtrousParams& prm, const AtrousVarParams& vprm, const float4* sum4, const float4* m2,
                            uint32_t frame_count, const float4* position_t, const float4* normal, const float4* albedo, float4* out, float* var_out)
{
    const size_t n = (size_t)width * height;
    const float nf = (float)frame_count, q = nf * (nf - 1.0f);
    std::vector<float4> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = atrous_var_first(sum4[i], m2[i], nf, q, albedo[i]);
    const AtrousVarTaps taps{prm.normal_power_log2, prm.sigma_plane, vprm.sigma_variance * vprm.sigma_variance, vprm.variance_floor};
    const float4* r = atrous_passes_host(prm.passes, width, height, position_t, normal, a.data(), b.data(), [&](int) { return taps; });
    for (size_t i = 0; i < n; i++) {
        const float4 am = atrous_amod(albedo[i]);
        out[i] = make_float4(r[i].x * am.x, r[i].y * am.y, r[i].z * am.z, 1.0f);
        var_out[i] = r[i].w;
    }
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_atrous_variance(int device, int32_t width, int32_t height, const jpt_denoise_params* params,
                                         const jpt_denoise_variance_params* vparams, const float* sum4, const float* m2_4, uint32_t frame_count,
                                         const float* position_t, const float* normal, const float* albedo, float* out4, float* var_out)
{
    if (!sum4 || !m2_4 || !position_t || !normal || !albedo || !out4 || !var_out || width <= 0 || height <= 0 || width > 65536 || height > 65536 ||
        frame_count < 2u)
        return JPT_E_INVALID;
    const AtrousParams prm = denoise_params_of(params);
    int32_t reserved = 0;
    const AtrousVarParams vprm = denoise_variance_params_of(vparams, reserved);
    std::string why;
    if (check_denoise_params(prm, why) != JPT_OK || check_denoise_variance_params(vprm, reserved, why) != JPT_OK) return JPT_E_INVALID;
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    const float4* in[5] = {reinterpret_cast<const float4*>(sum4), reinterpret_cast<const float4*>(m2_4), reinterpret_cast<const float4*>(position_t),
                           reinterpret_cast<const float4*>(normal), reinterpret_cast<const float4*>(albedo)};
    if (device == JPT_DEVICE_HOST_ONLY) {
        atrous_var_host(width, height, prm, vprm, in[0], in[1], frame_count, in[2], in[3], in[4], reinterpret_cast<float4*>(out4), var_out);
        return JPT_OK;
    }
    if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
    float4* buf = nullptr;   // sum, m2, position_t, normal, albedo, ping, pong, and n floats of v
    if (hipMalloc((void**)&buf, 7 * bytes + n * sizeof(float)) != hipSuccess) return JPT_E_DEVICE;
    float* var = reinterpret_cast<float*>(buf + 7 * n);
    bool ok = true;
    for (int k = 0; k < 5 && ok; k++) ok = hipMemcpy(buf + (size_t)k * n, in[k], bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_atrous_variance(nullptr, prm, vprm, width, height, 0, buf, buf + n, frame_count, buf + 2 * n, buf + 3 * n, buf + 4 * n, buf + 5 * n, buf + 6 * n,
                               nullptr, var);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out4, buf + 5 * n, bytes, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(var_out, var, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(buf);
    return ok ? JPT_OK : JPT_E_DEVICE;
}
