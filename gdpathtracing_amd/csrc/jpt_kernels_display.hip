// jpt_kernels_display.hip -- jpt_display: exposure, a pyramid bloom, the tone map and the transfer over the running mean (or over
// jpt_denoise's image).  No reference counterpart beyond the fixed unorm8(ACES(mean)) of progressive_rendering.glsl.  The arithmetic
// is pinned in jpt_display.h / DESIGN.md section 2; nothing here writes a buffer a render or jpt_denoise reads.
#include "../../include/jpt.h"
#include "jpt_display.h"

namespace jpt {

namespace {

constexpr int kTileW = 32, kTileH = 8, kDisplayBlock = kTileW * kTileH;

__device__ const float d_srgb_t[256] = {0.0f, JPT_DISPLAY_SRGB_T255};

struct Level {
    float4* p;
    int32_t w, h;
};

// D_1 from the source: one lane per pixel of D_1, 32 x 8 of them per block.  The block stages the 66 x 18 source pixels its taps
// touch (indices clamped to the image) in LDS with 16-byte accesses, as bright-pass values: base and bright pass run once per
// staged pixel, not once per tap, and B is never stored in memory.
__device__ __forceinline__ void display_down0_body(const float4* __restrict__ src, int32_t width, int32_t height, float fc, float exposure,
                                                   float threshold, Level out)
{
    constexpr int SW = 2 * kTileW + 2, SH = 2 * kTileH + 2;
    __shared__ float4 tile[SW * SH];
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    for (int i = (int)threadIdx.x; i < SW * SH; i += kDisplayBlock) {
        const int gx = display_clampi(2 * x0 - 1 + i % SW, width - 1), gy = display_clampi(2 * y0 - 1 + i / SW, height - 1);
        tile[i] = display_bright(display_base(src[(size_t)gy * (size_t)width + (size_t)gx], fc, exposure), threshold);
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & (kTileW - 1), ly = (int)threadIdx.x / kTileW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= out.w || y >= out.h) return;
    // the tap at column 2x - 1 + i is staged at 2lx + i when it lies inside the image; a clamped one is staged where its unclamped
    // column would be (the staging loop clamps every index the same way)
    DisplaySum s;
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int i = 0; i < 4; i++) s.tap(tile[(2 * ly + j) * SW + 2 * lx + i], display_w4(j) * display_w4(i));
    }
    out.p[(size_t)y * (size_t)out.w + (size_t)x] = make_float4(s.r, s.g, s.b, 0.0f);
}
__global__ __launch_bounds__(kDisplayBlock) void display_down0_kernel(const float4* __restrict__ src, int32_t width, int32_t height, float fc,
                                                                      float exposure, float threshold, Level out)
{
    display_down0_body(src, width, height, fc, exposure, threshold, out);
}
// the auto-exposure form (jpt_set_auto_exposure): the exposure is the parameter times the metered one, read from jpt_meter's state
// record -- every lane loads the same address.  An instantiation of its own: the kernel above is what it is without metering.
__global__ __launch_bounds__(kDisplayBlock) void display_down0_ae_kernel(const float4* __restrict__ src, int32_t width, int32_t height, float fc,
                                                                         float exposure, const float* __restrict__ metered, float threshold,
                                                                         Level out)
{
    display_down0_body(src, width, height, fc, exposure * metered[0], threshold, out);
}

// D_k+1 from D_k, k >= 1: one lane per pixel of D_k+1, 16 gathers of 16 bytes (a quarter of the image and less: they hit in L2)
__global__ __launch_bounds__(kDisplayBlock) void display_down_kernel(Level in, Level out)
{
    const int x = (int)blockIdx.x * kTileW + ((int)threadIdx.x & (kTileW - 1)), y = (int)blockIdx.y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= out.w || y >= out.h) return;
    DisplaySum s;
#pragma unroll 2   // (two rows' gathers in flight: all sixteen at once take more than 64 VGPRs)
    for (int j = 0; j < 4; j++) {
        const size_t row = (size_t)display_clampi(2 * y - 1 + j, in.h - 1) * (size_t)in.w;
#pragma unroll
        for (int i = 0; i < 4; i++) s.tap(in.p[row + (size_t)display_clampi(2 * x - 1 + i, in.w - 1)], display_w4(j) * display_w4(i));
    }
    out.p[(size_t)y * (size_t)out.w + (size_t)x] = make_float4(s.r, s.g, s.b, 0.0f);
}

// U_k = D_k + T(U_k+1), in place: a lane reads the coarser level and its own pixel, and writes its own pixel
__global__ __launch_bounds__(kDisplayBlock) void display_up_kernel(Level coarse, Level fine)
{
    const int x = (int)blockIdx.x * kTileW + ((int)threadIdx.x & (kTileW - 1)), y = (int)blockIdx.y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= fine.w || y >= fine.h) return;
    const DisplaySum t = display_tent_sum(coarse.p, coarse.w, coarse.h, x, y);
    const size_t idx = (size_t)y * (size_t)fine.w + (size_t)x;
    const float4 d = fine.p[idx];
    fine.p[idx] = make_float4(d.x + t.r, d.y + t.g, d.z + t.b, 0.0f);
}

// T(U_1), the composite, the tone map and the transfer: one lane per pixel.  The sRGB table is searched in LDS.
template <bool HAVE_BLOOM>
__device__ __forceinline__ void display_resolve_body(const float4* __restrict__ src, int32_t width, int32_t height, float fc, const DisplayConsts& k,
                                                     Level u1, float4* __restrict__ out_f32, uint32_t* __restrict__ out_rgba8)
{
    __shared__ float table[256];
    if (k.transfer == JPT_TRANSFER_SRGB) {
        table[threadIdx.x] = d_srgb_t[threadIdx.x];
        __syncthreads();
    }
    const int x = (int)blockIdx.x * kTileW + ((int)threadIdx.x & (kTileW - 1)), y = (int)blockIdx.y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= width || y >= height) return;
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    const float4 c = display_base(src[idx], fc, k.exposure);
    DisplaySum bloom;
    if (HAVE_BLOOM) bloom = display_tent_sum(u1.p, u1.w, u1.h, x, y);
    float4 v;
    const uint32_t q = display_resolve<HAVE_BLOOM>(k, c, bloom, table, v);
    out_f32[idx] = v;
    out_rgba8[idx] = q;
}
template <bool HAVE_BLOOM>
__global__ __launch_bounds__(kDisplayBlock) void display_resolve_kernel(const float4* __restrict__ src, int32_t width, int32_t height, float fc,
                                                                        DisplayConsts k, Level u1, float4* __restrict__ out_f32,
                                                                        uint32_t* __restrict__ out_rgba8)
{
    display_resolve_body<HAVE_BLOOM>(src, width, height, fc, k, u1, out_f32, out_rgba8);
}
template <bool HAVE_BLOOM>   // the auto-exposure form, as display_down0_ae_kernel
__global__ __launch_bounds__(kDisplayBlock) void display_resolve_ae_kernel(const float4* __restrict__ src, int32_t width, int32_t height, float fc,
                                                                           DisplayConsts k, const float* __restrict__ metered, Level u1,
                                                                           float4* __restrict__ out_f32, uint32_t* __restrict__ out_rgba8)
{
    k.exposure = k.exposure * metered[0];
    display_resolve_body<HAVE_BLOOM>(src, width, height, fc, k, u1, out_f32, out_rgba8);
}

dim3 grid_of(int w, int h) { return dim3((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH)); }

}  // namespace

void launch_display(hipStream_t stream, const DisplayParams& prm, int width, int height, const float4* src, float fc, float4* pyramid,
                    float4* out_f32, uint32_t* out_rgba8, const float* metered)
{
    if (width <= 0 || height <= 0) return;
    const DisplayConsts k = display_consts(prm);
    const dim3 block(kDisplayBlock);
    const int N = k.levels;
    Level lv[kDisplayMaxLevels + 1] = {};
    if (N > 0) {
        size_t off[kDisplayMaxLevels + 1] = {};
        display_pyramid_elems(width, height, N, off);
        int w = width, h = height;
        for (int l = 1; l <= N; l++) {
            w = display_level_size(w);
            h = display_level_size(h);
            lv[l] = Level{pyramid + off[l], w, h};
        }
        if (metered)
            hipLaunchKernelGGL(display_down0_ae_kernel, grid_of(lv[1].w, lv[1].h), block, 0, stream, src, width, height, fc, k.exposure, metered,
                               k.threshold, lv[1]);
        else
            hipLaunchKernelGGL(display_down0_kernel, grid_of(lv[1].w, lv[1].h), block, 0, stream, src, width, height, fc, k.exposure, k.threshold, lv[1]);
        for (int l = 1; l < N; l++) hipLaunchKernelGGL(display_down_kernel, grid_of(lv[l + 1].w, lv[l + 1].h), block, 0, stream, lv[l], lv[l + 1]);
        for (int l = N - 1; l >= 1; l--) hipLaunchKernelGGL(display_up_kernel, grid_of(lv[l].w, lv[l].h), block, 0, stream, lv[l + 1], lv[l]);
    }
    const dim3 grid = grid_of(width, height);
    if (metered) {
        if (N > 0) hipLaunchKernelGGL((display_resolve_ae_kernel<true>), grid, block, 0, stream, src, width, height, fc, k, metered, lv[1], out_f32, out_rgba8);
        else hipLaunchKernelGGL((display_resolve_ae_kernel<false>), grid, block, 0, stream, src, width, height, fc, k, metered, lv[1], out_f32, out_rgba8);
    } else {
        if (N > 0) hipLaunchKernelGGL((display_resolve_kernel<true>), grid, block, 0, stream, src, width, height, fc, k, lv[1], out_f32, out_rgba8);
        else hipLaunchKernelGGL((display_resolve_kernel<false>), grid, block, 0, stream, src, width, height, fc, k, lv[1], out_f32, out_rgba8);
    }
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_display(int device, int32_t width, int32_t height, const jpt_display_params* params, const float* mean4, float* out_f32,
                                 uint8_t* out_rgba8)
{
    if (!mean4 || (!out_f32 && !out_rgba8) || width <= 0 || height <= 0 || width > 65536 || height > 65536) return JPT_E_INVALID;
    DisplayParams prm;
    if (params) {
        prm.source = params->source;
        prm.tonemap = params->tonemap;
        prm.transfer = params->transfer;
        prm.bloom_levels = params->bloom_levels;
        prm.exposure = params->exposure;
        prm.white = params->white;
        prm.bloom_threshold = params->bloom_threshold;
        prm.bloom_strength = params->bloom_strength;
    }
    std::string why;
    if (check_display_params(prm, why) != JPT_OK) return JPT_E_INVALID;
    const size_t n = (size_t)width * height;
    if (device == JPT_DEVICE_HOST_ONLY) {
        display_host(width, height, prm, reinterpret_cast<const float4*>(mean4), 1.0f, reinterpret_cast<float4*>(out_f32),
                     reinterpret_cast<uint32_t*>(out_rgba8));
        return JPT_OK;
    }
    if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
    const size_t npyr = display_pyramid_elems(width, height, prm.bloom_levels, nullptr);
    float4* buf = nullptr;   // the image, the tone-mapped image, the pyramid, the rgba8 image
    if (hipMalloc((void**)&buf, (2 * n + npyr) * sizeof(float4) + n * sizeof(uint32_t)) != hipSuccess) return JPT_E_DEVICE;
    float4* pyr = buf + 2 * n;
    uint32_t* ldr = reinterpret_cast<uint32_t*>(pyr + npyr);
    bool ok = hipMemcpy(buf, mean4, n * sizeof(float4), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_display(nullptr, prm, width, height, buf, 1.0f, pyr, buf + n, ldr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        if (ok && out_f32) ok = hipMemcpy(out_f32, buf + n, n * sizeof(float4), hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && out_rgba8) ok = hipMemcpy(out_rgba8, ldr, n * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(buf);
    return ok ? JPT_OK : JPT_E_DEVICE;
}

extern "C" int jpt_debug_display_srgb_table(float* out255)
{
    if (!out255) return JPT_E_INVALID;
    for (int k = 1; k <= 255; k++) out255[k - 1] = kDisplaySrgbT[k];
    return JPT_OK;
}
