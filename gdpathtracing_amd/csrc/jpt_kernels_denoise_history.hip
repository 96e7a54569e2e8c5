// jpt_kernels_denoise_history.hip -- jpt_denoise with jpt_set_denoise_history on: the history stage (history_kernel) and the first
// variance-guided a-trous pass over the (m, v_0) image the stage leaves (atrous_var_pre_kernel); the later passes are those of
// jpt_kernels_denoise_var.hip (launch_atrous_variance from pass 1).  No reference counterpart.  The arithmetic is pinned in
// jpt_denoise_history.h and jpt_denoise_var.h / DESIGN.md section 2; nothing here writes a buffer a render reads.
#include "../../include/jpt.h"
#include "jpt_denoise_history.h"
#include "jpt_atrous_pass.h"
#include "jpt_kernels.h"
#include "jpt_trace_core.h"

namespace jpt {

namespace {

constexpr int kTileW = kAtrousTileW, kTileH = kAtrousTileH, kBlock = kAtrousBlock, kHalo = 2;
constexpr int kTW = AtrousTiles<kHalo>::TW;

struct HistoryArgs {
    const float4* __restrict__ sum;          // the accumulation (sums)
    const float4* __restrict__ albedo;
    const float4* __restrict__ x;            // position_t
    const float4* __restrict__ n;            // normal
    const float4* __restrict__ pa;           // the previous set (null: none): (m, N), (n, S), position_t
    const float4* __restrict__ pb;
    const float4* __restrict__ px;
    float4* __restrict__ na;                 // the new set
    float4* __restrict__ nb;
    float4* __restrict__ nx;
    float4* __restrict__ iv;                 // (m, v_0) for the filter
    int32_t width, height, npow, same_view;
    float nf;
    HistoryParams hp;
    HistoryView view;
    // what the stage's tiles hold beside the guides x and n (atrous_stage's Source): the demodulated mean
    static __device__ __forceinline__ float4 outside_x() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __device__ __forceinline__ float4 colour(size_t g, const float4&) const { return atrous_demodulate(sum[g], nf, albedo[g]); }
};

// One lane per pixel, 32 x 8 pixels per block.  Every lane gathers and integrates its history from memory (up to four taps of three
// 16-byte loads, neighbouring lanes on neighbouring texels).  Only a pixel whose history is shorter than min_history needs the 5 x 5
// estimate: the block votes, and only a block with such a pixel stages its tile and a 2-pixel halo of (c, X, n) in LDS (atrous_stage,
// jpt_atrous_pass.h) and runs the taps.
__global__ __launch_bounds__(kBlock) void history_kernel(HistoryArgs a)
{
    const int lx = (int)threadIdx.x & (kTileW - 1), ly = (int)threadIdx.x / kTileW;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < a.width && y < a.height;
    const size_t idx = (size_t)y * (size_t)a.width + (size_t)x;
    HistoryPixel o = {};
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), X = c, n = c;
    bool need = false;
    if (inside) {
        X = a.x[idx];
        n = a.n[idx];
        c = atrous_demodulate(a.sum[idx], a.nf, a.albedo[idx]);
        auto prev = [&](int qx, int qy) {
            const size_t g = (size_t)qy * (size_t)a.width + (size_t)qx;
            return HistoryTexel{a.pa[g], a.pb[g], a.px[g]};
        };
        const bool live = history_pixel(x, y, a.width, a.height, c, X, n, a.pa != nullptr, a.same_view != 0, a.view, a.hp, a.npow, a.nf, prev, o);
        need = live && o.spatial;
    }
    if (__syncthreads_or(need ? 1 : 0)) {   // (every lane of the block arrives: nothing above returns)
        const AtrousTiles<kHalo> t = atrous_stage<kHalo>(a, x0, y0, a.width, a.height);
        if (need) {
            const int ci = (ly + kHalo) * kTW + (lx + kHalo);
            const AtrousPixel p{c, X, n};
            HistorySpatial sp;
            uint32_t taken = 0u;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                    const int qi = ci + dy * kTW + dx;
                    const AtrousPixel q{t.c[qi], t.x[qi], t.n[qi]};
                    if (!history_spatial_accept(p, q, dx, dy, a.npow, a.hp.sigma_plane)) continue;
                    taken |= 1u << ((dy + 2) * 5 + (dx + 2));
                    sp.mean_tap(q.c);
                }
            }
            sp.mean_done();
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++)
                    if (taken & (1u << ((dy + 2) * 5 + (dx + 2)))) sp.dist_tap(t.c[ci + dy * kTW + dx]);
            }
            o.m.w = sp.result(o.al);
        }
    }
    if (!inside) return;
    a.iv[idx] = o.m;
    a.na[idx] = make_float4(o.m.x, o.m.y, o.m.z, o.N);
    a.nb[idx] = make_float4(n.x, n.y, n.z, o.S);
    a.nx[idx] = X;
}

// Pass 0 of the variance-guided filter over a pre-formed (i, v) image: the tiled pass of jpt_atrous_pass.h with the input as it is
// (atrous_var_kernel<2, true, ...> of jpt_kernels_denoise_var.hip forms (i_0, v_0) from the sums and the plane of second moments).
template <bool LAST>
__global__ __launch_bounds__(kBlock) void atrous_var_pre_kernel(AtrousVarFilter<false, LAST> f)
{
    atrous_pass<kHalo>(f, f.width, f.height, f.step);
}

}  // namespace

void launch_denoise_history(hipStream_t stream, const HistoryParams& hp, int normal_power_log2, int width, int height, const float4* sums, uint32_t frame_count,
                            const float4* position_t, const float4* normal, const float4* albedo, const HistoryView& prev_view, bool same_view,
                            const float4* prev_a, const float4* prev_b, const float4* prev_x, float4* new_a, float4* new_b, float4* new_x, float4* iv)
{
    if (width <= 0 || height <= 0) return;
    HistoryArgs a;
    a.sum = sums;
    a.albedo = albedo;
    a.x = position_t;
    a.n = normal;
    a.pa = prev_a;
    a.pb = prev_b;
    a.px = prev_x;
    a.na = new_a;
    a.nb = new_b;
    a.nx = new_x;
    a.iv = iv;
    a.width = width;
    a.height = height;
    a.npow = normal_power_log2;
    a.same_view = same_view ? 1 : 0;
    a.nf = (float)frame_count;
    a.hp = hp;
    a.view = prev_view;
    const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH)), block(kBlock);
    hipLaunchKernelGGL(history_kernel, grid, block, 0, stream, a);
}

void launch_atrous_history(hipStream_t stream, const AtrousParams& prm, const AtrousVarParams& vprm, int width, int height, const float4* iv,
                           const float4* position_t, const float4* normal, const float4* albedo, float4* ping, float4* pong, uint32_t* ldr, float* var_out)
{
    if (width <= 0 || height <= 0) return;
    AtrousVarArgs a = atrous_var_args(prm, vprm, width, height, nullptr, 2u, position_t, normal, albedo, ldr, var_out);
    const float4* i1 = atrous_launch_passes(0, 1, prm.passes, false, width, height, iv, ping, pong,
                                            [&](auto halo, int, const float4* in, float4* out, bool last, dim3 grid, dim3 block) {
                                                if constexpr (decltype(halo)::value == kHalo) {
                                                    a.in = in;
                                                    a.out = out;
                                                    a.step = 1;
                                                    if (last) hipLaunchKernelGGL(atrous_var_pre_kernel<true>, grid, block, 0, stream, AtrousVarFilter<false, true>{a});
                                                    else hipLaunchKernelGGL(atrous_var_pre_kernel<false>, grid, block, 0, stream, AtrousVarFilter<false, false>{a});
                                                }
                                            });
    launch_atrous_variance(stream, prm, vprm, width, height, 1, i1, nullptr, 2u, position_t, normal, albedo, ping, pong, ldr, var_out);
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_denoise_history(int device, int32_t width, int32_t height, const jpt_denoise_params* params,
                                         const jpt_denoise_history_params* hparams, const float* sum4, uint32_t frame_count, const float* position_t,
                                         const float* normal, const float* albedo, const float* prev_vp16, int32_t same_view, const float* prev_integrated4,
                                         const float* prev_normal_s4, const float* prev_position_t, float* iv_out4, float* integrated_out4, float* normal_s_out4)
{
    if (!sum4 || !position_t || !normal || !albedo || !iv_out4 || !integrated_out4 || !normal_s_out4 || width <= 0 || height <= 0 || width > 65536 ||
        height > 65536 || frame_count < 1u || (same_view != 0 && same_view != 1))
        return JPT_E_INVALID;
    const bool have_prev = prev_integrated4 != nullptr;
    if ((prev_normal_s4 != nullptr) != have_prev || (prev_position_t != nullptr) != have_prev) return JPT_E_INVALID;   // a set is three planes
    if (have_prev && !same_view && !prev_vp16) return JPT_E_INVALID;
    const AtrousParams prm = denoise_params_of(params);
    HistoryParams hp;
    int32_t reserved[4] = {0, 0, 0, 0};
    if (hparams) {
        hp.enable = hparams->enable;
        hp.max_history = hparams->max_history;
        hp.min_history = hparams->min_history;
        hp.sigma_plane = hparams->sigma_plane;
        for (int k = 0; k < 4; k++) reserved[k] = hparams->reserved[k];
    }
    std::string why;
    if (check_denoise_params(prm, why) != JPT_OK || check_denoise_history_params(hp, reserved, why) != JPT_OK) return JPT_E_INVALID;
    HistoryView view = {};
    if (prev_vp16)
        for (int k = 0; k < 16; k++) view.vp[k] = prev_vp16[k];
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    const float4* in[7] = {reinterpret_cast<const float4*>(sum4),     reinterpret_cast<const float4*>(position_t),       reinterpret_cast<const float4*>(normal),
                           reinterpret_cast<const float4*>(albedo),   reinterpret_cast<const float4*>(prev_integrated4), reinterpret_cast<const float4*>(prev_normal_s4),
                           reinterpret_cast<const float4*>(prev_position_t)};
    float4* out[3] = {reinterpret_cast<float4*>(iv_out4), reinterpret_cast<float4*>(integrated_out4), reinterpret_cast<float4*>(normal_s_out4)};
    if (device == JPT_DEVICE_HOST_ONLY) {
        history_host(width, height, hp, prm.normal_power_log2, in[0], frame_count, in[1], in[2], in[3], view, same_view != 0, in[4], in[5], in[6], out[0], out[1],
                     out[2]);
        return JPT_OK;
    }
    if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
    float4* buf = nullptr;   // the seven inputs, then iv, the new set's three planes
    if (hipMalloc((void**)&buf, 11 * bytes) != hipSuccess) return JPT_E_DEVICE;
    bool ok = true;
    for (int k = 0; k < (have_prev ? 7 : 4) && ok; k++) ok = hipMemcpy(buf + (size_t)k * n, in[k], bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_denoise_history(nullptr, hp, prm.normal_power_log2, width, height, buf, frame_count, buf + n, buf + 2 * n, buf + 3 * n, view, same_view != 0,
                               have_prev ? buf + 4 * n : nullptr, have_prev ? buf + 5 * n : nullptr, have_prev ? buf + 6 * n : nullptr, buf + 8 * n, buf + 9 * n,
                               buf + 10 * n, buf + 7 * n);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        for (int k = 0; k < 3 && ok; k++) ok = hipMemcpy(out[k], buf + (size_t)(7 + k) * n, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(buf);
    return ok ? JPT_OK : JPT_E_DEVICE;
}
