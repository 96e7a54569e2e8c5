// jpt_kernels_denoise_var.hip -- jpt_denoise with jpt_set_denoise_variance on: the a-trous passes of jpt_kernels_denoise.hip with the
// colour weight measured against the variance of the mean, which travels through the passes in the .w of the colour.  No reference
// counterpart.  The arithmetic is pinned in jpt_denoise_var.h / DESIGN.md section 2; nothing here writes a buffer a render reads.
#include "../../include/jpt.h"
#include "jpt_denoise_var.h"
#include "jpt_kernels.h"
#include "jpt_trace_core.h"

namespace jpt {

namespace {

struct AtrousVarArgs {
    const float4* __restrict__ in;        // FIRST: the accumulation (sums); else (i_k, v_k)
    const float4* __restrict__ m2;        // FIRST: the plane of jpt_set_variance
    const float4* __restrict__ position_t;
    const float4* __restrict__ normal;
    const float4* __restrict__ albedo;    // read by the first pass (demodulation) and the last (remodulation)
    float4* __restrict__ out;             // (i_k+1, v_k+1); LAST: the denoised image (r, g, b, 1)
    uint32_t* __restrict__ ldr;           // LAST: unorm8(ACES(denoised)) (may be null)
    float* __restrict__ var_out;          // LAST: v of the last pass
    int32_t width, height, step;
    float nf, q;                          // FIRST: (float)frame_count and nf * (nf - 1)
    int32_t npow;
    float sigma_plane, sv2, floor;
};

constexpr int kTileW = 32, kTileH = 8, kAtrousBlock = kTileW * kTileH;

template <bool FIRST>
__device__ __forceinline__ float4 atrous_var_colour(const AtrousVarArgs& a, size_t idx)
{
    const float4 v = a.in[idx];
    if (!FIRST) return v;
    return atrous_var_first(v, a.m2[idx], a.nf, a.q, a.albedo[idx]);
}

template <bool LAST>
__device__ __forceinline__ void atrous_var_write(const AtrousVarArgs& a, size_t idx, float4 r)
{
    if (!LAST) {
        a.out[idx] = r;
        return;
    }
    const float4 am = atrous_amod(a.albedo[idx]);
    const f3 den = mk3(r.x * am.x, r.y * am.y, r.z * am.z);
    a.out[idx] = make_float4(den.x, den.y, den.z, 1.0f);
    a.var_out[idx] = r.w;
    if (a.ldr) {
        const f3 col = aces_film(den);
        a.ldr[idx] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xFF000000u;
    }
}

// One pass, atrous_kernel's shape: one lane per pixel, 32 x 8 pixels per block.  HALO = 2 * step > 0 (steps 1 and 2): the block stages
// its tile and a HALO-pixel border of (colour, v), position_t and normal in LDS (the first pass demodulates and forms v_0 while it
// stages, reading the plane once per staged pixel) and reads the 3 x 3 prefilter and its 25 taps from there -- the prefilter's
// spacing is 1 and HALO >= 2 covers it.  HALO = 0 (steps >= 4): 16-byte gathers straight from memory, and nine 4-byte loads of v.
template <int HALO, bool FIRST, bool LAST>
__global__ __launch_bounds__(kAtrousBlock) void atrous_var_kernel(AtrousVarArgs a)
{
    static_assert(HALO > 0 || !FIRST, "the first pass is a tiled one: the gather form reads v from the .w of its input");
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
                c = atrous_var_colour<FIRST>(a, g);
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
        AtrousVarPrefilter pre;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                pre.tap(tc[ci + dy * TW + dx].w, dx, dy);
            }
        }
        const float den = pre.den(a.sv2, a.floor);
        AtrousVarSum sum;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx, qy = y + s * dy;
                if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                const int qi = ci + s * dy * TW + s * dx;
                const AtrousPixel q{tc[qi], tx[qi], tn[qi]};
                sum.tap(p, q, dx, dy, a.npow, a.sigma_plane, den);
            }
        }
        atrous_var_write<LAST>(a, idx, sum.result(p));
    } else {
        if (!inside) return;
        const int s = a.step;
        const AtrousPixel p{atrous_var_colour<FIRST>(a, idx), a.position_t[idx], a.normal[idx]};
        AtrousVarPrefilter pre;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                pre.tap(a.in[(size_t)qy * (size_t)a.width + (size_t)qx].w, dx, dy);
            }
        }
        const float den = pre.den(a.sv2, a.floor);
        AtrousVarSum sum;
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + s * dy;
            if (qy < 0 || qy >= a.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + s * dx;
                if (qx < 0 || qx >= a.width) continue;
                const size_t g = (size_t)qy * (size_t)a.width + (size_t)qx;
                const AtrousPixel q{atrous_var_colour<FIRST>(a, g), a.position_t[g], a.normal[g]};
                sum.tap(p, q, dx, dy, a.npow, a.sigma_plane, den);
            }
        }
        atrous_var_write<LAST>(a, idx, sum.result(p));
    }
}

template <int HALO, bool FIRST>
void launch_var_pass(hipStream_t stream, const AtrousVarArgs& a, bool last)
{
    const dim3 grid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH)), block(kAtrousBlock);
    if (last) hipLaunchKernelGGL((atrous_var_kernel<HALO, FIRST, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((atrous_var_kernel<HALO, FIRST, false>), grid, block, 0, stream, a);
}

}  // namespace

// passes first_pass .. passes - 1 of the filter; `src`: what pass first_pass reads (pass 0: the sums, with `m2` and `frame_count`)
static void launch_var_passes(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, int first_pass, const float4* src,
                              const float4* m2, uint32_t frame_count, const float4* position_t, const float4* normal, const float4* albedo, float4* ping,
                              float4* pong, uint32_t* ldr, float* var_out)
{
    if (width <= 0 || height <= 0) return;
    AtrousVarArgs a;
    a.m2 = m2;
    a.position_t = position_t;
    a.normal = normal;
    a.albedo = albedo;
    a.ldr = ldr;
    a.var_out = var_out;
    a.width = width;
    a.height = height;
    a.nf = (float)frame_count;
    a.q = a.nf * (a.nf - 1.0f);
    a.npow = prm.normal_power_log2;
    a.sigma_plane = prm.sigma_plane;
    a.sv2 = vprm.sigma_variance * vprm.sigma_variance;
    a.floor = vprm.variance_floor;
    // the last pass writes `ping` (launch_atrous' arrangement)
    float4* dst = ((prm.passes - first_pass) & 1) ? ping : pong;
    float4* other = ((prm.passes - first_pass) & 1) ? pong : ping;
    for (int k = first_pass; k < prm.passes; k++) {
        a.in = src;
        a.out = dst;
        a.step = 1 << k;
        const bool last = k + 1 == prm.passes;
        if (k == 0) launch_var_pass<2, true>(stream, a, last);
        else if (k == 1) launch_var_pass<4, false>(stream, a, last);
        else launch_var_pass<0, false>(stream, a, last);
        src = dst;
        float4* t = dst;
        dst = other;
        other = t;
    }
}

void launch_atrous_variance(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, const float4* sums,
                            const float4* m2, uint32_t frame_count, const float4* position_t, const float4* normal, const float4* albedo, float4* ping,
                            float4* pong, uint32_t* ldr, float* var_out)
{
    launch_var_passes(stream, prm, vprm, width, height, 0, sums, m2, frame_count, position_t, normal, albedo, ping, pong, ldr, var_out);
}

void launch_atrous_variance_from(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, int first_pass,
                                 const float4* src, const float4* position_t, const float4* normal, const float4* albedo, float4* ping, float4* pong,
                                 uint32_t* ldr, float* var_out)
{
    launch_var_passes(stream, prm, vprm, width, height, first_pass, src, nullptr, 2u, position_t, normal, albedo, ping, pong, ldr, var_out);
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
    AtrousParams prm;
    if (params) {
        prm.passes = params->passes;
        prm.normal_power_log2 = params->normal_power_log2;
        prm.sigma_plane = params->sigma_plane;
        prm.sigma_color = params->sigma_color;
    }
    AtrousVarParams vprm;
    int32_t reserved = 0;
    if (vparams) {
        vprm.enable = vparams->enable;
        vprm.sigma_variance = vparams->sigma_variance;
        vprm.variance_floor = vparams->variance_floor;
        reserved = vparams->reserved;
    }
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
        launch_atrous_variance(nullptr, prm, vprm, width, height, buf, buf + n, frame_count, buf + 2 * n, buf + 3 * n, buf + 4 * n, buf + 5 * n, buf + 6 * n,
                               nullptr, var);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out4, buf + 5 * n, bytes, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(var_out, var, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(buf);
    return ok ? JPT_OK : JPT_E_DEVICE;
}
