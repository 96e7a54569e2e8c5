// jpt_kernels_meter.hip -- jpt_meter: the log-luminance histogram of the running mean (or of jpt_denoise's image) and its resolve
// into one exposure value on the device.  No reference counterpart.  The arithmetic is pinned in jpt_meter.h / DESIGN.md section 2;
// nothing here writes a buffer a render, jpt_denoise or jpt_display writes.
#include "../../include/jpt.h"
#include "jpt_meter.h"

#include <cmath>

namespace jpt {

namespace {

// 2 048 blocks at most (eight per CU) with four 16-byte loads in flight per lane: a 1920 x 1080 image is one trip of the loop.
// Measured at that size (tools/meter_rate.py): 512 / 1 024 / 2 048 / 4 096 blocks over one set of global bins took 21 / 27 / 33 /
// 58 us per call -- a block's flush to a bin waits for every other block's flush to that bin, ~12 ns each --, over 16 sets 2 048
// blocks take 11.5 us; 8 or 32 sets, 1 024 or 4 096 blocks, and unrolls of 2 and 8 are all within 1 us of that.
constexpr int kMeterBlock = 256, kMeterUnroll = 4, kMeterMaxBlocks = 2048;
static_assert(kMeterBlock == kMeterBins, "one lane per bin clears and flushes the block's bins");

// One pixel per lane into the block's bins.  Called by whole waves (a lane without a counted pixel passes bin = -1).  A flat
// region sends every lane of a wave to one bin, and LDS atomics on one address run one lane after the other; so a wave whose
// counted lanes all name the same bin adds their weights with one atomic from one lane.  Any other wave adds per lane.
__device__ __forceinline__ void meter_count(uint32_t* bins, int bin, uint32_t weight)
{
    const bool counted = bin >= 0;
    const unsigned long long act = __ballot(counted);
    if (act == 0) return;
    const int leader = __ffsll(act) - 1;
    const int lead_bin = __builtin_amdgcn_readlane(bin, leader);
    if (__ballot(counted && bin == lead_bin) == act) {
        const uint32_t sum = (uint32_t)__popcll(act) + 3u * (uint32_t)__popcll(__ballot(counted && weight == 4u));
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&bins[lead_bin], sum);
    } else if (counted) {
        atomicAdd(&bins[bin], weight);
    }
}

// The histogram: 16 bytes read per pixel, nothing written per pixel.  One set of bins per block in LDS (1 KB): the four waves of a
// block share one LDS unit, so a set per wave would take four times the flush and save no atomic.  A grid-stride loop, four loads
// of 16 bytes in flight per lane, with a block-uniform bound so that whole waves reach meter_count; then one vector atomic per
// non-empty bin to one of the kMeterSets sets of global bins (the block's index picks it, so that blocks that run side by side add
// to different addresses), 256 contiguous bytes per wave instruction.
template <bool CENTER>
__global__ __launch_bounds__(kMeterBlock) void meter_histogram_kernel(const float4* __restrict__ src, uint32_t n, int32_t width, int32_t height,
                                                                      float fc, uint32_t* __restrict__ bins)
{
    __shared__ uint32_t local[kMeterBins];
    local[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * (uint32_t)kMeterBlock;
    for (uint32_t base = blockIdx.x * (uint32_t)kMeterBlock; base < n; base += kMeterUnroll * stride) {   // (n <= 2^30: no wrap)
        float4 v[kMeterUnroll];
        uint32_t idx[kMeterUnroll];
#pragma unroll
        for (int k = 0; k < kMeterUnroll; k++) {
            idx[k] = base + (uint32_t)k * stride + threadIdx.x;
            if (idx[k] < n) v[k] = src[idx[k]];
        }
#pragma unroll
        for (int k = 0; k < kMeterUnroll; k++) {
            int bin = -1;
            uint32_t weight = 1;
            if (idx[k] < n) {
                bin = meter_bin(v[k], fc);
                if (CENTER) {
                    const uint32_t y = idx[k] / (uint32_t)width;
                    weight = meter_weight(1, (int)(idx[k] - y * (uint32_t)width), (int)y, width, height);
                }
            }
            meter_count(local, bin, weight);
        }
    }
    __syncthreads();
    const uint32_t mine = local[threadIdx.x];
    if (mine) atomicAdd(&bins[(blockIdx.x % (uint32_t)kMeterSets) * (uint32_t)kMeterBins + threadIdx.x], mine);
}

// The resolve: one wave, four bins per lane, in a launch of its own behind the histogram (stream order is the synchronisation).
// The sums are uint64 and exact, so how they are split over the lanes does not show: the weight before a lane's bins is a scan
// over the wave, `used` and `S` are butterfly sums.  Lane 0 takes the binary32 steps and stores the record; every lane sums its
// four bins over the working sets, publishes them for jpt_read_meter and clears the sets for the next histogram (no memset in
// front of a call that is not a FIRST one).  All stores are plain vector stores.
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}
__global__ __launch_bounds__(64) void meter_resolve_kernel(uint32_t* __restrict__ bins, uint32_t* __restrict__ published, int32_t low_permille,
                                                           int32_t high_permille, float key, float min_exposure, float max_exposure, float adapt,
                                                           int32_t first, MeterState* __restrict__ state)
{
    const int lane = (int)threadIdx.x;
    uint4 h4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int s = 0; s < kMeterSets; s++) {
        uint4* set = reinterpret_cast<uint4*>(bins + s * kMeterBins);
        const uint4 v = set[lane];
        set[lane] = make_uint4(0u, 0u, 0u, 0u);
        h4 = make_uint4(h4.x + v.x, h4.y + v.y, h4.z + v.z, h4.w + v.w);
    }
    reinterpret_cast<uint4*>(published)[lane] = h4;
    const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
    const uint64_t mine = (uint64_t)h[0] + h[1] + h[2] + h[3];
    uint64_t incl = mine;   // the weight up to and including this lane's bins
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t below = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += below;
    }
    const uint64_t total = (uint64_t)__shfl((unsigned long long)incl, 63);
    const uint64_t lo = total * (uint64_t)low_permille / 1000u, hi = total * (uint64_t)high_permille / 1000u;
    uint64_t cum = incl - mine, used = 0, S = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t c = meter_clip(cum, h[k], lo, hi);
        used += c;
        S += c * (uint64_t)(2 * (4 * lane + k) + 1);
        cum += h[k];
    }
    used = wave_sum(used);
    S = wave_sum(S);
    if (lane != 0) return;
    const float prev = first ? 0.0f : state->exposure;
    *state = meter_finish(total, used, S, key, min_exposure, max_exposure, adapt, first != 0, prev);
}

}  // namespace

void launch_meter(hipStream_t stream, const MeterParams& prm, int width, int height, const float4* src, float fc, bool first, uint32_t* bins,
                  MeterState* state)
{
    if (width <= 0 || height <= 0) return;
    const uint32_t n = (uint32_t)width * (uint32_t)height;
    // the resolve leaves the working bins cleared; only a FIRST call (fresh buffers, or a reset) clears them itself
    if (first) (void)hipMemsetAsync(bins + kMeterBins, 0, kMeterSets * kMeterBins * sizeof(uint32_t), stream);
    const uint32_t per_block = (uint32_t)(kMeterBlock * kMeterUnroll);
    const uint32_t want = (n + per_block - 1) / per_block;
    const dim3 grid(want < (uint32_t)kMeterMaxBlocks ? want : (uint32_t)kMeterMaxBlocks), block(kMeterBlock);
    if (prm.mode == JPT_METER_CENTER_WEIGHTED)
        hipLaunchKernelGGL((meter_histogram_kernel<true>), grid, block, 0, stream, src, n, width, height, fc, bins + kMeterBins);
    else
        hipLaunchKernelGGL((meter_histogram_kernel<false>), grid, block, 0, stream, src, n, width, height, fc, bins + kMeterBins);
    hipLaunchKernelGGL(meter_resolve_kernel, dim3(1), dim3(64), 0, stream, bins + kMeterBins, bins, prm.low_permille, prm.high_permille, prm.key, prm.min_exposure,
                       prm.max_exposure, prm.adapt, first ? 1 : 0, state);
}

}  // namespace jpt

using namespace jpt;

extern "C" int jpt_debug_meter(int device, int32_t width, int32_t height, const jpt_meter_params* params, const float* mean4, float prev_exposure,
                               uint32_t* hist256_out, jpt_meter_result* result_out)
{
    if (!mean4 || !result_out || width <= 0 || height <= 0 || width > 65536 || height > 65536) return JPT_E_INVALID;
    MeterParams prm;
    if (params) {
        prm.source = params->source;
        prm.mode = params->mode;
        prm.low_permille = params->low_permille;
        prm.high_permille = params->high_permille;
        prm.key = params->key;
        prm.min_exposure = params->min_exposure;
        prm.max_exposure = params->max_exposure;
        prm.adapt = params->adapt;
    }
    std::string why;
    if (check_meter_params(prm, why) != JPT_OK) return JPT_E_INVALID;
    const bool first = std::isnan(prev_exposure);
    if (!first && std::isinf(prev_exposure)) return JPT_E_INVALID;
    if ((uint64_t)width * (uint64_t)height > (1ull << 30)) return JPT_E_LIMIT;
    const size_t n = (size_t)width * height;
    uint32_t hist[kMeterBins];
    MeterState st;
    if (device == JPT_DEVICE_HOST_ONLY) {
        meter_host(width, height, prm, reinterpret_cast<const float4*>(mean4), 1.0f, first, prev_exposure, hist, &st);
    } else {
        if (hipSetDevice(device) != hipSuccess) return JPT_E_DEVICE;
        char* buf = nullptr;   // the image, the bins, the state record
        if (hipMalloc((void**)&buf, n * sizeof(float4) + kMeterBinWords * sizeof(uint32_t) + sizeof st) != hipSuccess) return JPT_E_DEVICE;
        uint32_t* d_bins = reinterpret_cast<uint32_t*>(buf + n * sizeof(float4));
        MeterState* d_state = reinterpret_cast<MeterState*>(d_bins + kMeterBinWords);
        st = MeterState{};
        st.exposure = first ? 0.0f : prev_exposure;
        bool ok = hipMemcpy(buf, mean4, n * sizeof(float4), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(d_bins, 0, kMeterBinWords * sizeof(uint32_t)) == hipSuccess && hipMemcpy(d_state, &st, sizeof st, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            launch_meter(nullptr, prm, width, height, reinterpret_cast<const float4*>(buf), 1.0f, first, d_bins, d_state);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(hist, d_bins, sizeof hist, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(&st, d_state, sizeof st, hipMemcpyDeviceToHost) == hipSuccess;
        }
        (void)hipFree(buf);
        if (!ok) return JPT_E_DEVICE;
    }
    if (hist256_out)
        for (int b = 0; b < kMeterBins; b++) hist256_out[b] = hist[b];
    result_out->exposure = st.exposure;
    result_out->target = st.target;
    result_out->luminance = st.luminance;
    result_out->flags = st.flags;
    result_out->weight = st.weight;
    result_out->used = st.used;
    return JPT_OK;
}
