// jpt_variance.h -- the arithmetic of jpt_set_variance and jpt_noise_estimate ("noise"): the second central
// moment of a pixel's frames kept beside the accumulation, and its reduction to one 32-byte answer.  No reference counterpart.
//
// The moment.  M2.c = sum over the frames f of (cur_f.c - mean.c)^2, c = r, g, b, kept frame by frame with an update that does not
// cancel.  With k the ProgressiveRendering frame_count of the frame (1: the first after a reset), cur the frame's value exactly as
// wf2_accumulate adds it and sum the accumulation's own sum, replayed with wf2_accumulate's own line:
//     sum = have_prev ? cur + sum : cur
//     k == 1:  m2 = +0                                  (whatever the plane held)
//     k >= 2:  kf = (float)k;  d = kf * cur - sum;  w = 1.0f / (kf * (kf - 1.0f));  m2 = m2 + (d * d) * w
// In real arithmetic this is Welford's update, (x - mean_old)(x - mean_new) = (k x - sum_k)^2 / (k (k - 1)); it uses the accumulation's
// sum, so no second mean is stored, and every term is >= 0, so m2 is never negative.  The textbook sum of squares minus the square of
// the sum cancels (tests/test_variance_host.py records by how much).  A pixel whose frames are all equal need not give exactly 0: k * x
// and x + x + ... round differently, so the result is of order x^2 * 2^-48.  It is not special-cased.
//
// The estimate.  Per pixel, with nf = (float)frame_count and q = nf * (nf - 1.0f):
//     mean.c = sum.c / nf;   v.c = m2.c / q
//     lm = 0.2126f * mean.x + 0.7152f * mean.y + 0.0722f * mean.z          (meter_bin's expression, left to right)
//     lv = 0.2126f * v.x + 0.7152f * v.y + 0.0722f * v.z
//     e  = sqrt(lv) / (lm + floor)                                          (the relative standard error of the mean)
// A pixel is counted when its six inputs are finite, lm >= 0 and (bake renders) its texel is valid.  A counted pixel's bin is
// meter_bin's, clampi((int)(bits(e) >> 20) - 856, 255); it is "above" when e > threshold; a tile's value is the largest e > 0 of its
// counted pixels, or 0 (a NaN e, which only a negative m2 handed in from outside can make, is in bin 255 and is never a maximum).
// The sums are integers and the maxima are of non-negative floats, so nothing depends on the order the pixels arrive in.
//
// Each + - * / sqrt is one binary32 operation in the order written (-ffp-contract=off): the device kernels
// (jpt_kernels_variance.hip) and the host forms of jpt_debug_variance_moments / jpt_debug_noise_estimate run these functions, and
// tests/np_variance.py restates them bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "jpt_device_math.h"
#include "jpt_meter.h"

namespace jpt {

constexpr uint32_t kNoiseEmpty = 1u, kNoiseConverged = 2u;   // JPT_NOISE_EMPTY, JPT_NOISE_CONVERGED
// the device's bins: the published histogram (what jpt_read_noise reads), then kMeterSets working sets of kNoiseSetWords words, of
// which a block adds to one: a set is 256 bins, the count of "above" pixels and three words of padding (16-byte rows)
constexpr int kNoiseSetWords = kMeterBins + 4;
constexpr int kNoiseBinWords = kMeterBins + kMeterSets * kNoiseSetWords;

struct NoiseParams {   // jpt_noise_params
    float threshold = 0.05f;
    float floor = 0.01f;
    int32_t percentile_permille = 950;
    int32_t allowed_permille = 0;
};

// the device's record, and what jpt_read_noise hands out: jpt_noise_result, 32 bytes
struct NoiseResult {
    float error, max_error;
    uint32_t flags, tiles_above;
    uint64_t counted, above;
};
static_assert(sizeof(NoiseResult) == 32, "jpt_noise_result is 32 bytes");

// the checks of jpt_set_noise_params, also run by jpt_debug_noise_estimate
inline int check_noise_params(const NoiseParams& p, std::string& why)
{
    if (p.threshold != p.threshold) why = "jpt_noise_params: threshold must not be NaN";
    else if (!std::isfinite(p.floor) || !(p.floor > 0.0f)) why = "jpt_noise_params: floor must be finite and > 0";
    else if (p.percentile_permille < 1 || p.percentile_permille > 1000) why = "jpt_noise_params: percentile_permille must be in [1, 1000]";
    else if (p.allowed_permille < 0 || p.allowed_permille > 1000) why = "jpt_noise_params: allowed_permille must be in [0, 1000]";
    else return 0;    // JPT_OK
    return -1;        // JPT_E_INVALID
}

// ---- the moment -----------------------------------------------------------------------------------------------------------------

// one frame more: `sum` is wf2_accumulate's, replayed; k is the frame's ProgressiveRendering frame_count
__host__ __device__ __forceinline__ void variance_add(f3& sum, f3& m2, bool have_prev, uint32_t k, const f3 cur)
{
    sum = have_prev ? cur + sum : cur;   // progressive_rendering.glsl:34-36, as wf2_accumulate has it
    if (k < 2u) {
        m2 = mk3(0.0f, 0.0f, 0.0f);
        return;
    }
    const float kf = (float)k;
    const f3 d = mk3(kf * cur.x - sum.x, kf * cur.y - sum.y, kf * cur.z - sum.z);
    const float w = 1.0f / (kf * (kf - 1.0f));
    m2 = m2 + (d * d) * w;
}

// ---- the estimate ---------------------------------------------------------------------------------------------------------------

// per pixel: e, and whether the pixel is counted (`valid`: its texel is one, or the render is no bake render)
__host__ __device__ __forceinline__ bool noise_pixel(const float4& sum, const float4& m2, float nf, float q, float floor, bool valid, float& e)
{
    const float mx = sum.x / nf, my = sum.y / nf, mz = sum.z / nf;
    const float vx = m2.x / q, vy = m2.y / q, vz = m2.z / q;
    const float lm = 0.2126f * mx + 0.7152f * my + 0.0722f * mz;
    const float lv = 0.2126f * vx + 0.7152f * vy + 0.0722f * vz;
    e = __builtin_sqrtf(lv) / (lm + floor);
    return valid && display_finite(sum.x) && display_finite(sum.y) && display_finite(sum.z) && display_finite(m2.x) && display_finite(m2.y) &&
           display_finite(m2.z) && lm >= 0.0f;
}
__host__ __device__ __forceinline__ int noise_bin(float e) { return display_clampi((int)(meter_float_bits(e) >> 20) - 856, kMeterBins - 1); }
// what a counted pixel offers to its tile's maximum
__host__ __device__ __forceinline__ float noise_tile_value(float e) { return e > 0.0f ? e : 0.0f; }
// the upper edge of bin b
__host__ __device__ __forceinline__ float noise_bin_edge(int b) { return meter_bits_float((uint32_t)(b + 1 + 856) << 20); }

// resolve: from the sums to the record.  first_bin: the first bin at which the cumulative count reaches the percentile's target
// (256: none, counted == 0)
__host__ __device__ __forceinline__ uint64_t noise_target(uint64_t counted, int32_t percentile_permille)
{
    return (counted * (uint64_t)percentile_permille + 999u) / 1000u;
}
__host__ __device__ __forceinline__ NoiseResult noise_finish(uint64_t counted, uint64_t above, int first_bin, float max_error, uint32_t tiles_above,
                                                             uint32_t frame_count, int32_t allowed_permille)
{
    NoiseResult r;
    r.counted = counted;
    r.above = above;
    r.tiles_above = tiles_above;
    if (frame_count < 2u || counted == 0) {
        r.flags = kNoiseEmpty;
        r.error = 0.0f;
        r.max_error = 0.0f;
        return r;
    }
    r.error = noise_bin_edge(first_bin);
    r.max_error = max_error;
    r.flags = above * 1000u <= counted * (uint64_t)allowed_permille ? kNoiseConverged : 0u;
    return r;
}

// the whole pass on the host (jpt_debug_noise_estimate with JPT_DEVICE_HOST_ONLY); normal: the bake normal image, or null
inline void noise_host(int32_t width, int32_t height, const NoiseParams& prm, const float4* sum, const float4* m2, uint32_t frame_count, const float4* normal,
                       uint32_t* hist, float* tiles, NoiseResult* result)
{
    const float nf = (float)frame_count, q = nf * (nf - 1.0f);
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    for (int b = 0; b < kMeterBins; b++) hist[b] = 0;
    for (int t = 0; t < tiles_x * tiles_y; t++) tiles[t] = 0.0f;
    uint64_t counted = 0, above = 0;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const bool valid = !normal || normal[i].x * normal[i].x + normal[i].y * normal[i].y + normal[i].z * normal[i].z > 0.0f;   // bake_texel_valid
            float e;
            if (!noise_pixel(sum[i], m2[i], nf, q, prm.floor, valid, e)) continue;
            hist[noise_bin(e)]++;
            counted++;
            if (e > prm.threshold) above++;
            float& t = tiles[(size_t)(y / 8) * tiles_x + x / 8];
            const float v = noise_tile_value(e);
            t = v > t ? v : t;
        }
    const uint64_t target = noise_target(counted, prm.percentile_permille);
    uint64_t cum = 0;
    int first_bin = kMeterBins;
    for (int b = 0; b < kMeterBins; b++) {
        cum += hist[b];
        if (first_bin == kMeterBins && counted && cum >= target) first_bin = b;
    }
    float max_error = 0.0f;
    uint32_t tiles_above = 0;
    for (int t = 0; t < tiles_x * tiles_y; t++) {
        max_error = tiles[t] > max_error ? tiles[t] : max_error;
        if (tiles[t] > prm.threshold) tiles_above++;
    }
    *result = noise_finish(counted, above, first_bin, max_error, tiles_above, frame_count, prm.allowed_permille);
}

// What the moment kernel of one render reads and writes (jpt_kernels_variance.hip): the per-(slot, frame) values wf2_accumulate
// reads, in its layout, the accumulation as it stood before the render, and the plane.  Every pointer is device memory.
struct FrameParams;
struct VarianceArgs {
    const float4* rad = nullptr;       // JPT_ACCUM_HDR_F32: the finished radiance per (slot, frame)
    const uint32_t* fin8 = nullptr;    // JPT_ACCUM_REF_LDR8: the same as rgba8 words
    const float4* accum = nullptr;     // the accumulation before this render's wf2_accumulate (read when fp.frame_count > 1)
    float4* plane = nullptr;           // width x local_rows float4: (M2.r, M2.g, M2.b, 0)
    int32_t full_tiles_x = 0, full_tiles_y = 0;   // the context's share of the image in 8 x 8 tiles: with the switch on a render's window is all of it
    uint32_t slots_per_frame = 0;      // full_tiles_x * full_tiles_y * 64
    int32_t groups = 1;                // the frame groups whose blocks of rad / fin8 are read
};
// on `stream`, in front of wf2_accumulate: one thread per pixel of the share; fp is the render's (frame_index / frame_count of its FIRST frame)
void launch_variance_moments(hipStream_t stream, const VarianceArgs& a, const FrameParams& fp);
// jpt_noise_estimate's launches on `stream`, over `bins` (kNoiseBinWords words; the working sets behind the first 256 must be zero, and
// are left zero), width * height <= 2^30: the estimate (one wave per 8 x 8 tile) fills the working sets and `tiles`
// (ceil(width / 8) * ceil(height / 8) floats), the resolve (one wave, a launch of its own) publishes bins[0 .. 255] and writes `result`.
void launch_noise_estimate(hipStream_t stream, const NoiseParams& prm, int width, int height, const float4* sum, const float4* m2, uint32_t frame_count,
                           const float4* normal, uint32_t* bins, float* tiles, NoiseResult* result);

}  // namespace jpt
