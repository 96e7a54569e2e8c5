// jpt_kernels_denoise.hip -- jpt_denoise: the first-hit guide images and the edge-avoiding a-trous filter over the running mean.
// No reference counterpart (the reference lists a denoiser among its wanted features).  The arithmetic is pinned in
// jpt_denoise.h / DESIGN.md section 2; nothing here writes a buffer a render reads.
#include "../../include/jpt.h"
#include "jpt_denoise.h"
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
    const float4* __restrict__ position_t;
    const float4* __restrict__ normal;
    const float4* __restrict__ albedo;    // read by the first pass (demodulation) and the last (remodulation)
    float4* __restrict__ out;             // i_k+1; LAST: the denoised image (r, g, b, 1)
    uint32_t* __restrict__ ldr;           // LAST: unorm8(ACES(denoised)) (may be null)
    int32_t width, height, step;
    float frame_count;                    // FIRST: what the sums are divided by
    int32_t npow;
    float sigma_plane, sc2;
};

constexpr int kTileW = 32, kTileH = 8, kAtrousBlock = kTileW * kTileH;

template <bool FIRST>
__device__ __forceinline__ float4 atrous_colour(const AtrousArgs& a, size_t idx)
{
    const float4 v = a.in[idx];
    if (!FIRST) return v;
    return atrous_demodulate(v, a.frame_count, a.albedo[idx]);
}

template <bool LAST>
__device__ __forceinline__ void atrous_write(const AtrousArgs& a, size_t idx, float4 r)
{
    if (!LAST) {
        a.out[idx] = r;
        return;
    }
    const float4 am = atrous_amod(a.albedo[idx]);
    const f3 den = mk3(r.x * am.x, r.y * am.y, r.z * am.z);
    a.out[idx] = make_float4(den.x, den.y, den.z, 1.0f);
    if (a.ldr) {
        const f3 col = aces_film(den);
        a.ldr[idx] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xFF000000u;
    }
}

// One pass, one lane per pixel, 32 x 8 pixels per block.  HALO = 2 * step > 0 (steps 1 and 2): the block stages its tile and a
// HALO-pixel border of colour, position_t and normal in LDS with 16-byte accesses (the first pass demodulates while it stages:
// once per staged pixel, not once per tap) and reads its 25 taps from there.  HALO = 0 (steps >= 4): the taps of a wave's row are
// themselves contiguous rows of 32 pixels, so 16-byte gathers straight from memory coalesce; a tile's border would be larger
// than the tile.
template <int HALO, bool FIRST, bool LAST>
__global__ __launch_bounds__(kAtrousBlock) void atrous_kernel(AtrousArgs a)
{
    const int lx = (int)threadIdx.x & (kTileW - 1), ly = (int)threadIdx.x / kTileW;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < a.width && y < a.height;
    const size_t idx = (size_t)y * (size_t)a.width + (size_t)x;
    if (HALO > 0) {
        constexpr int TW = kTileW + 2 * HALO, TH = kTileH + 2 * HALO, s = HALO / 2;
        __shared__ float4 tc[TW * TH], tx[TW * TH], tn[TW * TH];
        for (int i = (int)threadIdx.x; i < TW * TH; i += kAtrousBlock) {
            const int gx = x0 - HALO + i % TW, gy = y0 - HALO + i / TW;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), px = c, nn = c;
            if (gx >= 0 && gy >= 0 && gx < a.width && gy < a.height) {
                const size_t g = (size_t)gy * (size_t)a.width + (size_t)gx;
                c = atrous_colour<FIRST>(a, g);
                px = a.position_t[g];
                nn = a.normal[g];
            }
            tc[i] = c;
            tx[i] = px;
            tn[i] = nn;
        }
        __syncthreads();
        if (!inside) return;
        const int ci = (ly + HALO) * TW + (lx + HALO);
        const AtrousPixel p{tc[ci], tx[ci], tn[ci]};
        AtrousSum sum;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx, qy = y + s * dy;
                if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                const int qi = ci + s * dy * TW + s * dx;
                const AtrousPixel q{tc[qi], tx[qi], tn[qi]};
                sum.tap(p, q, dx, dy, a.npow, a.sigma_plane, a.sc2);
            }
        }
        atrous_write<LAST>(a, idx, sum.result(p));
    } else {
        if (!inside) return;
        const int s = a.step;
        const AtrousPixel p{atrous_colour<FIRST>(a, idx), a.position_t[idx], a.normal[idx]};
        AtrousSum sum;
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + s * dy;
            if (qy < 0 || qy >= a.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx;
                if (qx < 0 || qx >= a.width) continue;
                const size_t g = (size_t)qy * (size_t)a.width + (size_t)qx;
                const AtrousPixel q{atrous_colour<FIRST>(a, g), a.position_t[g], a.normal[g]};
                sum.tap(p, q, dx, dy, a.npow, a.sigma_plane, a.sc2);
            }
        }
        atrous_write<LAST>(a, idx, sum.result(p));
    }
}

template <int HALO, bool FIRST>
void launch_pass(hipStream_t stream, const AtrousArgs& a, bool last)
{
    const dim3 grid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH)), block(kAtrousBlock);
    if (last) hipLaunchKernelGGL((atrous_kernel<HALO, FIRST, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((atrous_kernel<HALO, FIRST, false>), grid, block, 0, stream, a);
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
    AtrousArgs a;
    a.position_t = position_t;
    a.normal = normal;
    a.albedo = albedo;
    a.ldr = ldr;
    a.width = width;
    a.height = height;
    a.frame_count = frame_count;
    a.npow = prm.normal_power_log2;
    a.sigma_plane = prm.sigma_plane;
    float sc = prm.sigma_color;
    // the last pass writes `ping` (atrous_result)
    float4* dst = (prm.passes & 1) ? ping : pong;
    float4* other = (prm.passes & 1) ? pong : ping;
    const float4* src = sums;
    for (int k = 0; k < prm.passes; k++, sc = sc * 0.5f) {
        a.in = src;
        a.out = dst;
        a.step = 1 << k;
        a.sc2 = sc * sc;
        const bool last = k + 1 == prm.passes;
        if (k == 0) launch_pass<2, true>(stream, a, last);
        else if (k == 1) launch_pass<4, false>(stream, a, last);
        else launch_pass<0, false>(stream, a, last);
        src = dst;
        float4* t = dst;
        dst = other;
        other = t;
    }
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_atrous(int device, int32_t width, int32_t height, const jpt_denoise_params* params, const float* mean4,
                                const float* position_t, const float* normal, const float* albedo, float* out)
{
    if (!mean4 || !position_t || !normal || !albedo || !out || width <= 0 || height <= 0 || width > 65536 || height > 65536) return JPT_E_INVALID;
    AtrousParams prm;
    if (params) {
        prm.passes = params->passes;
        prm.normal_power_log2 = params->normal_power_log2;
        prm.sigma_plane = params->sigma_plane;
        prm.sigma_color = params->sigma_color;
    }
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
