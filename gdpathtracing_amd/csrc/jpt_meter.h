// jpt_meter.h -- the arithmetic of jpt_meter ("metering"): a 256-bin log-luminance histogram of the running
// mean of the progressive accumulation (or of jpt_denoise's image) and its resolve into one exposure value, with percentile
// clipping and temporal adaptation.  No reference counterpart.  The pixel step is binary32 + - * /, compares and one shift of the
// value's bits, the resolve is uint64 arithmetic and four binary32 operations, each one operation in source order: the device
// kernels (jpt_kernels_meter.hip) and the host form of jpt_debug_meter run these functions, and tests/np_meter.py restates them
// bit for bit.  The bins are integer sums, so the histogram does not depend on the order the pixels arrive in.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "jpt_display.h"

namespace jpt {

constexpr int kMeterBins = 256;
// the device's bins: the published histogram (what jpt_read_meter reads), then kMeterSets working sets of which a block adds to one
// (atomics of many blocks on one address wait for each other: jpt_kernels_meter.hip); 17 KB
constexpr int kMeterSets = 16;
constexpr int kMeterBinWords = (1 + kMeterSets) * kMeterBins;
constexpr uint32_t kMeterEmpty = 1u, kMeterFirst = 2u;   // JPT_METER_EMPTY, JPT_METER_FIRST

struct MeterParams {   // jpt_meter_params
    int32_t source = 0;   // JPT_DISPLAY_SOURCE_ACCUM
    int32_t mode = 0;     // JPT_METER_AVERAGE
    int32_t low_permille = 100;
    int32_t high_permille = 900;
    float key = 0.18f;
    float min_exposure = 0.015625f;
    float max_exposure = 64.0f;
    float adapt = 1.0f;
};

// the device's state record, and what jpt_read_meter hands out: jpt_meter_result, 32 bytes
struct MeterState {
    float exposure, target, luminance;
    uint32_t flags;
    uint64_t weight, used;
};
static_assert(sizeof(MeterState) == 32, "jpt_meter_result is 32 bytes");

// the checks of jpt_set_meter_params, also run by jpt_debug_meter
inline int check_meter_params(const MeterParams& p, std::string& why)
{
    if (p.source < 0 || p.source > 1) why = "jpt_meter_params: source must be JPT_DISPLAY_SOURCE_ACCUM or JPT_DISPLAY_SOURCE_DENOISED";
    else if (p.mode < 0 || p.mode > 1) why = "jpt_meter_params: mode must be JPT_METER_AVERAGE or JPT_METER_CENTER_WEIGHTED";
    else if (p.low_permille < 0 || p.low_permille > 1000) why = "jpt_meter_params: low_permille must be in [0, 1000]";
    else if (p.high_permille <= p.low_permille || p.high_permille > 1000) why = "jpt_meter_params: high_permille must be in (low_permille, 1000]";
    else if (!std::isfinite(p.key) || !(p.key > 0.0f)) why = "jpt_meter_params: key must be finite and > 0";
    else if (!std::isfinite(p.min_exposure) || !(p.min_exposure > 0.0f)) why = "jpt_meter_params: min_exposure must be finite and > 0";
    else if (!std::isfinite(p.max_exposure) || !(p.max_exposure >= p.min_exposure)) why = "jpt_meter_params: max_exposure must be finite and >= min_exposure";
    else if (!(p.adapt >= 0.0f && p.adapt <= 1.0f)) why = "jpt_meter_params: adapt must be in [0, 1]";
    else return 0;    // JPT_OK
    return -1;        // JPT_E_INVALID
}

__host__ __device__ __forceinline__ uint32_t meter_float_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__host__ __device__ __forceinline__ float meter_bits_float(uint32_t b) { return __builtin_bit_cast(float, b); }

// per pixel, 1.-4.: the bin of the running mean's luminance, or -1 for a pixel that is not counted (a non-finite channel, or a
// luminance that is not over 0).  Eight bins per octave from 2^-20 (bin 0) to 2^12 (the end of bin 255): the exponent and the top
// three bits of the fraction, less 856 = (127 - 20) << 3; darker and brighter values land in the end bins.
__host__ __device__ __forceinline__ int meter_bin(const float4& sum, float fc)
{
    const float mx = sum.x / fc, my = sum.y / fc, mz = sum.z / fc;
    const float lum = 0.2126f * mx + 0.7152f * my + 0.0722f * mz;
    if (!display_finite(mx) || !display_finite(my) || !display_finite(mz) || !(lum > 0.0f)) return -1;
    return display_clampi((int)(meter_float_bits(lum) >> 20) - 856, kMeterBins - 1);
}

// per pixel, 5.: 1, or 4 in the middle half of both axes under JPT_METER_CENTER_WEIGHTED
__host__ __device__ __forceinline__ uint32_t meter_weight(int mode, int x, int y, int width, int height)
{
    const int64_t x4 = 4 * (int64_t)x, y4 = 4 * (int64_t)y, w = width, h = height;   // (64 bits: only width * height is bounded)
    return (mode == 1 && x4 >= w && x4 < 3 * w && y4 >= h && y4 < 3 * h) ? 4u : 1u;
}

// resolve, 4.: what of bin b's weight h, with `cum` the weight before it, lies between lo and hi
__host__ __device__ __forceinline__ uint64_t meter_clip(uint64_t cum, uint32_t h, uint64_t lo, uint64_t hi)
{
    const uint64_t end = cum + h;
    const int64_t c = (int64_t)(end < hi ? end : hi) - (int64_t)(cum > lo ? cum : lo);
    return c > 0 ? (uint64_t)c : 0;
}

// resolve, 5.-7.: from the sums to the state.  `first`: no state before this call (prev is not read).
__host__ __device__ __forceinline__ MeterState meter_finish(uint64_t total, uint64_t used, uint64_t S, float key, float min_exposure, float max_exposure,
                                                            float adapt, bool first, float prev)
{
    MeterState st;
    st.flags = first ? kMeterFirst : 0u;
    st.weight = total;
    st.used = used;
    if (used == 0) {
        st.flags |= kMeterEmpty;
        st.exposure = first ? display_clamp(1.0f, min_exposure, max_exposure) : prev;
        st.target = st.exposure;
        st.luminance = 0.0f;
        return st;
    }
    const uint64_t p = (S * 32768u) / used;
    const float l_avg = meter_bits_float(0x35800000u + (uint32_t)(p << 4));
    const float e_t = display_clamp(key / l_avg, min_exposure, max_exposure);
    if (first) {
        st.exposure = e_t;
    } else {
        const float d = e_t - prev;
        const float step = d * adapt;
        st.exposure = prev + step;
    }
    st.target = e_t;
    st.luminance = l_avg;
    return st;
}

// the whole pass on the host (jpt_debug_meter with device -1): src = sums (or an image, fc = 1)
inline void meter_host(int32_t width, int32_t height, const MeterParams& prm, const float4* src, float fc, bool first, float prev, uint32_t* hist,
                       MeterState* state)
{
    for (int b = 0; b < kMeterBins; b++) hist[b] = 0;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const int b = meter_bin(src[(size_t)y * width + x], fc);
            if (b >= 0) hist[b] += meter_weight(prm.mode, x, y, width, height);
        }
    uint64_t total = 0;
    for (int b = 0; b < kMeterBins; b++) total += hist[b];
    const uint64_t lo = total * (uint64_t)prm.low_permille / 1000u, hi = total * (uint64_t)prm.high_permille / 1000u;
    uint64_t cum = 0, used = 0, S = 0;
    for (int b = 0; b < kMeterBins; b++) {
        const uint64_t c = meter_clip(cum, hist[b], lo, hi);
        used += c;
        S += c * (uint64_t)(2 * b + 1);
        cum += hist[b];
    }
    *state = meter_finish(total, used, S, prm.key, prm.min_exposure, prm.max_exposure, prm.adapt, first, prev);
}

// jpt_meter's launches (jpt_kernels_meter.hip), on `stream`, over `bins` (kMeterBinWords words): the working sets are filled from
// `src` (width * height sums, or an image with fc = 1; width * height <= 2^30) and resolved into `state` by one wave in a launch
// of its own behind the histogram, which also publishes their sum as bins[0 .. 255] and clears them for the next call.  `first`:
// `state` holds nothing yet and the working sets are cleared here.  Nothing else is written.
void launch_meter(hipStream_t stream, const MeterParams& prm, int width, int height, const float4* src, float fc, bool first, uint32_t* bins,
                  MeterState* state);

}  // namespace jpt
