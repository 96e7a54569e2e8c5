// jpt_kernels_variance.hip -- jpt_set_variance's moment kernel, launched by launch_wf2_render in front of wf2_accumulate, and
// jpt_noise_estimate's two kernels; the host loops of jpt_debug_variance_moments and jpt_debug_noise_estimate.  The arithmetic:
// jpt_variance.h / DESIGN.md section 2.  No reference counterpart.
//
// variance_moments reads what wf2_accumulate is about to read -- every frame's finished value per (slot, frame), rad or fin8 -- and the
// accumulation as it stood before the render, replays the sum and adds each frame's squared deviation to the plane.  No path kernel
// knows about it, and it writes nothing but the plane.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jpt.h"
#include "jpt_bake_dir.h"
#include "jpt_kernels.h"
#include "jpt_variance.h"

namespace jpt {
namespace {

constexpr int kVarBlock = 256;   // four waves, each one 8 x 8 tile

typedef float var_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t var_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 var_ld4(const float4* p)
{
    const var_v4f v = __builtin_nontemporal_load(reinterpret_cast<const var_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 var_ldu4(const uint4* p)
{
    const var_v4u v = __builtin_nontemporal_load(reinterpret_cast<const var_v4u*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void var_st4(float4* p, const float4 v)
{
    var_v4f w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<var_v4f*>(p));
}
__device__ __forceinline__ f3 var_word(uint32_t q)   // the rgba8 load of progressive_rendering.glsl:33, as wf2_accumulate makes it
{
    return mk3(from_unorm8(q & 255u), from_unorm8((q >> 8) & 255u), from_unorm8((q >> 16) & 255u));
}

// One thread per pixel of the context's share, tile by tile exactly as wf2_accumulate walks it: a wave is one 8 x 8 tile, a pixel's
// frames are one run of rad / fin8, and a tile row's store into the plane is 128 contiguous bytes.  `slot` is the pixel's place in the
// render's window, which with the switch on is the whole share (no sky cull: prepare_render).  The old sum is read here, in front of
// wf2_accumulate on the same stream, so it is the accumulation before this render; the plain accum load is the only read of it.
__global__ __launch_bounds__(kVarBlock) void variance_moments(VarianceArgs a, FrameParams fp)
{
    const uint32_t slot = blockIdx.x * (uint32_t)kVarBlock + threadIdx.x;
    const uint32_t tile = slot >> 6, lane = slot & 63u;
    const uint32_t ty = tile / (uint32_t)a.full_tiles_x, tx = tile - ty * (uint32_t)a.full_tiles_x;
    if ((int)ty >= a.full_tiles_y) return;   // (the whole wave)
    const int px = (int)(tx * 8u + (lane & 7u)), ly = (int)(ty * 8u + (lane >> 3));
    if (px >= fp.width || ly >= fp.local_rows) return;
    const size_t idx = (size_t)ly * (size_t)fp.width + (size_t)px;
    // fp.frame_count = ProgressiveRendering frame_count of the FIRST frame of this render, as in wf2_accumulate
    bool have_prev = fp.frame_count > 1;
    f3 sum = mk3(0.0f, 0.0f, 0.0f), m2 = mk3(0.0f, 0.0f, 0.0f);
    if (have_prev) {
        const float4 s = var_ld4(&a.accum[idx]), m = var_ld4(&a.plane[idx]);
        sum = mk3(s.x, s.y, s.z);
        m2 = mk3(m.x, m.y, m.z);
    }
    uint32_t k = fp.frame_count;
    // rgba8 samples, one frame group, a multiple of four frames: a pixel's frames are consecutive 16-byte pieces of fin8 (wf2_accumulate's
    // packed-frames case, here for any such count: the next piece is in flight while this one's four frames are added)
    const bool packed_frames = fp.accum_mode == 0 && a.groups == 1 && (fp.n_frames & 3) == 0;
    if (packed_frames) {
        const uint4* mine = reinterpret_cast<const uint4*>(a.fin8 + (size_t)slot * (size_t)fp.n_frames);
        const int pieces = fp.n_frames >> 2;
        uint4 next = var_ldu4(&mine[0]);
        for (int c = 0; c < pieces; c++) {
            const uint4 q = next;
            if (c + 1 < pieces) next = var_ldu4(&mine[c + 1]);
            variance_add(sum, m2, have_prev, k, var_word(q.x));
            variance_add(sum, m2, true, k + 1u, var_word(q.y));
            variance_add(sum, m2, true, k + 2u, var_word(q.z));
            variance_add(sum, m2, true, k + 3u, var_word(q.w));
            have_prev = true;
            k += 4u;
        }
    } else {
        // the frames of group g are a block of their own in rad / fin8: [slot][frame of the group] behind the earlier groups' blocks
        const int g_base = fp.n_frames / a.groups, g_extra = fp.n_frames % a.groups;
        int g = 0, g_f0 = 0, g_nf = g_base + (g_extra > 0 ? 1 : 0);
        for (int f = 0; f < fp.n_frames; f++) {
            if (f >= g_f0 + g_nf) {
                g++;
                g_f0 += g_nf;
                g_nf = g_base + (g < g_extra ? 1 : 0);
            }
            const size_t at = (size_t)g_f0 * a.slots_per_frame + (size_t)slot * (size_t)g_nf + (size_t)(f - g_f0);
            f3 cur;
            if (fp.accum_mode == 0) {
                cur = var_word(__builtin_nontemporal_load(&a.fin8[at]));
            } else {
                const float4 r = var_ld4(&a.rad[at]);
                cur = mk3(r.x, r.y, r.z);
            }
            variance_add(sum, m2, have_prev, k, cur);
            have_prev = true;
            k++;
        }
    }
    var_st4(&a.plane[idx], make_float4(m2.x, m2.y, m2.z, 0.0f));
}

// ---- jpt_noise_estimate ---------------------------------------------------------------------------------------------------------

constexpr int kNoiseBlock = 256, kNoiseMaxBlocks = 2048;   // (meter_histogram_kernel's, for its reasons)
static_assert(kNoiseBlock == kMeterBins, "one lane per bin clears and flushes the block's bins");

// One pixel per lane into the block's bins, as meter_count does it with every weight 1: a wave whose counted lanes all name the same
// bin (a flat region; LDS atomics on one address run one lane after the other) adds their number with one atomic from one lane.
__device__ __forceinline__ void noise_count(uint32_t* bins, int bin)
{
    const bool counted = bin >= 0;
    const unsigned long long act = __ballot(counted);
    if (act == 0) return;
    const int leader = __ffsll(act) - 1;
    const int lead_bin = __builtin_amdgcn_readlane(bin, leader);
    if (__ballot(counted && bin == lead_bin) == act) {
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&bins[lead_bin], (uint32_t)__popcll(act));
    } else if (counted) {
        atomicAdd(&bins[bin], 1u);
    }
}

// The estimate: a wave per 8 x 8 tile of the image, two 16-byte loads per pixel (a third, of the bake normal, in a bake render),
// nothing written per pixel.  The tile's maximum is a butterfly over the wave, stored by lane 0; the bins and the count of pixels
// above the threshold are the block's in LDS (1 040 B), flushed with one vector atomic per non-empty word to one of the kMeterSets
// sets of global words, which the block's index picks (meter_histogram_kernel's arrangement).
__global__ __launch_bounds__(kNoiseBlock) void noise_estimate_kernel(const float4* __restrict__ sum, const float4* __restrict__ m2, const float4* __restrict__ normal,
                                                                     int32_t width, int32_t height, int32_t tiles_x, uint32_t n_tiles, float nf, float q, float floor,
                                                                     float threshold, uint32_t* __restrict__ sets, float* __restrict__ tiles)
{
    __shared__ uint32_t local[kNoiseSetWords];
    local[threadIdx.x] = 0;
    if (threadIdx.x < (uint32_t)(kNoiseSetWords - kNoiseBlock)) local[kNoiseBlock + threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_block = (uint32_t)(kNoiseBlock / 64);
    for (uint32_t tile = blockIdx.x * per_block + wave; tile < n_tiles; tile += gridDim.x * per_block) {   // (wave-uniform)
        const uint32_t ty = tile / (uint32_t)tiles_x, tx = tile - ty * (uint32_t)tiles_x;
        const int x = (int)(tx * 8u + (lane & 7u)), y = (int)(ty * 8u + (lane >> 3));
        int bin = -1;
        float mine = 0.0f;
        bool above = false;
        if (x < width && y < height) {
            const size_t idx = (size_t)y * (size_t)width + (size_t)x;
            const float4 s = sum[idx], m = m2[idx];
            const bool valid = normal == nullptr || bake_texel_valid(normal[idx]);
            float e;
            if (noise_pixel(s, m, nf, q, floor, valid, e)) {
                bin = noise_bin(e);
                mine = noise_tile_value(e);
                above = e > threshold;
            }
        }
        noise_count(local, bin);
        const unsigned long long ab = __ballot(above);
        if (ab != 0 && lane == 0) atomicAdd(&local[kMeterBins], (uint32_t)__popcll(ab));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float other = __shfl_xor(mine, d);
            mine = other > mine ? other : mine;
        }
        if (lane == 0) tiles[tile] = mine;
    }
    __syncthreads();
    uint32_t* set = sets + (blockIdx.x % (uint32_t)kMeterSets) * (uint32_t)kNoiseSetWords;
    const uint32_t h = local[threadIdx.x];
    if (h) atomicAdd(&set[threadIdx.x], h);
    if (threadIdx.x == 0 && local[kMeterBins]) atomicAdd(&set[kMeterBins], local[kMeterBins]);
}

// The resolve: one wave, four bins per lane, in a launch of its own behind the estimate (stream order is the synchronisation).  The
// sums are uint64 and exact and the maxima are of non-negative floats, so how they are split over the lanes does not show.  Every lane
// sums its four bins over the working sets, publishes them for jpt_read_noise and clears the sets for the next estimate; the tile map
// is walked with a stride of the wave.  Lane 0 stores the record.  All stores are plain vector stores.
__device__ __forceinline__ uint64_t noise_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}
__global__ __launch_bounds__(64) void noise_resolve_kernel(uint32_t* __restrict__ sets, uint32_t* __restrict__ published, const float* __restrict__ tiles,
                                                           uint32_t n_tiles, float threshold, int32_t percentile_permille, int32_t allowed_permille,
                                                           uint32_t frame_count, NoiseResult* __restrict__ result)
{
    const int lane = (int)threadIdx.x;
    uint4 h4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int s = 0; s < kMeterSets; s++) {
        uint4* set = reinterpret_cast<uint4*>(sets + s * kNoiseSetWords);
        const uint4 v = set[lane];
        set[lane] = make_uint4(0u, 0u, 0u, 0u);
        h4 = make_uint4(h4.x + v.x, h4.y + v.y, h4.z + v.z, h4.w + v.w);
    }
    uint64_t above = 0;
    if (lane < kMeterSets) {
        above = sets[lane * kNoiseSetWords + kMeterBins];
        sets[lane * kNoiseSetWords + kMeterBins] = 0u;
    }
    above = noise_wave_sum(above);
    reinterpret_cast<uint4*>(published)[lane] = h4;
    const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
    const uint64_t mine = (uint64_t)h[0] + h[1] + h[2] + h[3];
    uint64_t incl = mine;   // the count up to and including this lane's bins
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t below = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += below;
    }
    const uint64_t counted = (uint64_t)__shfl((unsigned long long)incl, 63);
    const uint64_t target = noise_target(counted, percentile_permille);
    uint64_t cum = incl - mine;
    int first_bin = kMeterBins;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cum += h[k];
        if (first_bin == kMeterBins && counted != 0 && cum >= target) first_bin = 4 * lane + k;
    }
    float max_error = 0.0f;
    uint64_t tiles_above = 0;
    // the tile map, 16 bytes per load and four loads in flight per lane (a 1920 x 1080 image has 32 400 tiles: one 4-byte load per
    // trip was 506 trips of a load's latency, 128 us; this is 32), then the last n_tiles % 4 tiles
    const uint32_t n4 = n_tiles >> 2;
    const float4* tiles4 = reinterpret_cast<const float4*>(tiles);
    for (uint32_t base = (uint32_t)lane; base < n4; base += 256u) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = base + 64u * (uint32_t)k < n4 ? tiles4[base + 64u * (uint32_t)k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (base + 64u * (uint32_t)k >= n4) break;   // (the zeros above are no tiles: a negative threshold would count them)
            const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                max_error = e[j] > max_error ? e[j] : max_error;
                tiles_above += e[j] > threshold ? 1u : 0u;
            }
        }
    }
    if ((uint32_t)lane < (n_tiles & 3u)) {
        const float v = tiles[4u * n4 + (uint32_t)lane];
        max_error = v > max_error ? v : max_error;
        tiles_above += v > threshold ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int other_bin = __shfl_xor(first_bin, d);
        first_bin = other_bin < first_bin ? other_bin : first_bin;
        const float other = __shfl_xor(max_error, d);
        max_error = other > max_error ? other : max_error;
    }
    tiles_above = noise_wave_sum(tiles_above);
    if (lane != 0) return;
    *result = noise_finish(counted, above, first_bin, max_error, (uint32_t)tiles_above, frame_count, allowed_permille);
}

}  // namespace

void launch_variance_moments(hipStream_t stream, const VarianceArgs& a, const FrameParams& fp)
{
    if (fp.n_frames <= 0 || a.full_tiles_x <= 0 || a.full_tiles_y <= 0) return;
    const uint32_t blocks = ((uint32_t)a.full_tiles_x * (uint32_t)a.full_tiles_y * 64u + (uint32_t)kVarBlock - 1u) / (uint32_t)kVarBlock;
    hipLaunchKernelGGL(variance_moments, dim3(blocks), dim3(kVarBlock), 0, stream, a, fp);
}

void launch_noise_estimate(hipStream_t stream, const NoiseParams& prm, int width, int height, const float4* sum, const float4* m2, uint32_t frame_count,
                           const float4* normal, uint32_t* bins, float* tiles, NoiseResult* result)
{
    if (width <= 0 || height <= 0) return;
    const int32_t tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const uint32_t n_tiles = (uint32_t)tiles_x * (uint32_t)tiles_y;
    const uint32_t per_block = (uint32_t)(kNoiseBlock / 64);
    const uint32_t want = (n_tiles + per_block - 1) / per_block;
    const float nf = (float)frame_count, q = nf * (nf - 1.0f);
    hipLaunchKernelGGL(noise_estimate_kernel, dim3(want < (uint32_t)kNoiseMaxBlocks ? want : (uint32_t)kNoiseMaxBlocks), dim3(kNoiseBlock), 0, stream, sum, m2,
                       normal, width, height, tiles_x, n_tiles, nf, q, prm.floor, prm.threshold, bins + kMeterBins, tiles);
    hipLaunchKernelGGL(noise_resolve_kernel, dim3(1), dim3(64), 0, stream, bins + kMeterBins, bins, tiles, n_tiles, prm.threshold, prm.percentile_permille,
                       prm.allowed_permille, frame_count, result);
}

// the moment on the host, over the caller's arrays: variance_add in a plain loop
void variance_moments_host(const float* radiance3, int32_t n_frames, uint32_t frame_count, int32_t accum_mode, float* sum4, float* m2_4, int32_t width,
                           int32_t height)
{
    const size_t n = (size_t)width * (size_t)height;
    for (size_t i = 0; i < n; i++) {
        bool have_prev = frame_count > 1;
        f3 sum = have_prev ? mk3(sum4[4 * i], sum4[4 * i + 1], sum4[4 * i + 2]) : mk3(0.0f, 0.0f, 0.0f);
        f3 m2 = have_prev ? mk3(m2_4[4 * i], m2_4[4 * i + 1], m2_4[4 * i + 2]) : mk3(0.0f, 0.0f, 0.0f);
        for (int32_t f = 0; f < n_frames; f++) {
            const float* r = radiance3 + ((size_t)f * n + i) * 3;
            f3 cur = mk3(r[0], r[1], r[2]);
            if (accum_mode == JPT_ACCUM_REF_LDR8) cur = bake_dir_ldr8(cur);   // (the rgba8 store and load)
            variance_add(sum, m2, have_prev, frame_count + (uint32_t)f, cur);
            have_prev = true;
        }
        sum4[4 * i] = sum.x; sum4[4 * i + 1] = sum.y; sum4[4 * i + 2] = sum.z; sum4[4 * i + 3] = 1.0f;   // (wf2_accumulate's alpha)
        m2_4[4 * i] = m2.x; m2_4[4 * i + 1] = m2.y; m2_4[4 * i + 2] = m2.z; m2_4[4 * i + 3] = 0.0f;
    }
}

}  // namespace jpt

using namespace jpt;

extern "C" {

int jpt_debug_variance_moments(const float* radiance3, int32_t n_frames, uint32_t frame_count, int32_t accum_mode, float* sum_inout, float* m2_inout,
                               int32_t width, int32_t height)
{
    const char* why = nullptr;
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536) why = "jpt_debug_variance_moments: width and height must be in [1, 65536]";
    else if (!sum_inout || !m2_inout || (n_frames > 0 && !radiance3)) why = "jpt_debug_variance_moments: null argument";
    else if (n_frames < 0) why = "jpt_debug_variance_moments: n_frames < 0";
    else if (frame_count == 0) why = "jpt_debug_variance_moments: frame_count starts at 1 (the first frame after a reset)";
    else if (accum_mode != JPT_ACCUM_REF_LDR8 && accum_mode != JPT_ACCUM_HDR_F32) why = "jpt_debug_variance_moments: unknown accum_mode";
    if (why) {
        set_debug_error(why);
        return JPT_E_INVALID;
    }
    if (n_frames == 0) return JPT_OK;   // (a render of no frames launches nothing: the sum and the plane stay)
    variance_moments_host(radiance3, n_frames, frame_count, accum_mode, sum_inout, m2_inout, width, height);
    return JPT_OK;
}

int jpt_debug_noise_estimate(int device, int32_t width, int32_t height, const jpt_noise_params* params, const float* sum4, const float* m2_4,
                             uint32_t frame_count, const uint8_t* valid_or_null, uint32_t* hist256_out, float* tiles_out, jpt_noise_result* result_out)
{
    if (!sum4 || !m2_4 || !result_out || width <= 0 || height <= 0 || width > 65536 || height > 65536) {
        set_debug_error("jpt_debug_noise_estimate: null argument, or width or height outside [1, 65536]");
        return JPT_E_INVALID;
    }
    NoiseParams prm;
    if (params) {
        prm.threshold = params->threshold;
        prm.floor = params->floor;
        prm.percentile_permille = params->percentile_permille;
        prm.allowed_permille = params->allowed_permille;
    }
    std::string why;
    if (check_noise_params(prm, why) != JPT_OK) {
        set_debug_error(why);
        return JPT_E_INVALID;
    }
    if (frame_count == 0) {
        set_debug_error("jpt_debug_noise_estimate: frame_count starts at 1");
        return JPT_E_INVALID;
    }
    if ((uint64_t)width * (uint64_t)height > (1ull << 30)) {
        set_debug_error("jpt_debug_noise_estimate: more than 2^30 pixels");
        return JPT_E_LIMIT;
    }
    const size_t n = (size_t)width * height;
    const size_t n_tiles = (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
    // (the caller's arrays need not be 16-byte aligned: copied; the validity mask becomes a bake normal image)
    std::vector<float4> img((valid_or_null ? 3 : 2) * n);
    for (size_t i = 0; i < n; i++) {
        img[i] = make_float4(sum4[4 * i], sum4[4 * i + 1], sum4[4 * i + 2], sum4[4 * i + 3]);
        img[n + i] = make_float4(m2_4[4 * i], m2_4[4 * i + 1], m2_4[4 * i + 2], m2_4[4 * i + 3]);
        if (valid_or_null) img[2 * n + i] = make_float4(0.0f, 0.0f, valid_or_null[i] ? 1.0f : 0.0f, 0.0f);
    }
    uint32_t hist[kMeterBins];
    std::vector<float> tiles(n_tiles);
    NoiseResult res;
    if (device == JPT_DEVICE_HOST_ONLY) {
        noise_host(width, height, prm, img.data(), img.data() + n, frame_count, valid_or_null ? img.data() + 2 * n : nullptr, hist, tiles.data(), &res);
    } else {
        if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
        char* buf = nullptr;   // the images, the tile map, the bins, the record
        const size_t img_bytes = img.size() * sizeof(float4), tile_bytes = (n_tiles * sizeof(float) + 15u) & ~(size_t)15u;
        if (hipMalloc((void**)&buf, img_bytes + tile_bytes + kNoiseBinWords * sizeof(uint32_t) + sizeof res) != hipSuccess) return JPT_E_DEVICE;
        const float4* d_img = reinterpret_cast<const float4*>(buf);
        float* d_tiles = reinterpret_cast<float*>(buf + img_bytes);
        uint32_t* d_bins = reinterpret_cast<uint32_t*>(buf + img_bytes + tile_bytes);
        NoiseResult* d_res = reinterpret_cast<NoiseResult*>(d_bins + kNoiseBinWords);
        bool ok = hipMemcpy(buf, img.data(), img_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(d_tiles, 0, tile_bytes + kNoiseBinWords * sizeof(uint32_t) + sizeof res) == hipSuccess;
        if (ok) {
            launch_noise_estimate(nullptr, prm, width, height, d_img, d_img + n, frame_count, valid_or_null ? d_img + 2 * n : nullptr, d_bins, d_tiles, d_res);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(hist, d_bins, sizeof hist, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(tiles.data(), d_tiles, n_tiles * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(&res, d_res, sizeof res, hipMemcpyDeviceToHost) == hipSuccess;
        }
        (void)hipFree(buf);
        if (!ok) return JPT_E_DEVICE;
    }
    if (hist256_out)
        for (int b = 0; b < kMeterBins; b++) hist256_out[b] = hist[b];
    if (tiles_out)
        for (size_t t = 0; t < n_tiles; t++) tiles_out[t] = tiles[t];
    static_assert(sizeof(jpt_noise_result) == sizeof(NoiseResult), "the record is jpt_noise_result");
    std::memcpy(result_out, &res, sizeof res);
    return JPT_OK;
}

}  // extern "C"
