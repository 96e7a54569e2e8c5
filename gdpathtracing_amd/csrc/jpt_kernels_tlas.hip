// jpt_kernels_tlas.hip -- a new topology for the instance level, made on the device (jpt_scene_rebuild_tlas): the instances sorted
// along a Morton curve through the centres of their world boxes (the arithmetic: jpt_tlas_rebuild.h), then the child words of a fixed
// four-way tree over the sorted positions (the host's template, a function of the instance count) written into a TLAS tail.  The boxes
// and the quantised records are the refit's (jpt_kernels_post.hip).  No reference counterpart: the reference rebuilds on the host.
#include "jpt_kernels.h"
#include "jpt_tlas_rebuild.h"

namespace jpt {

namespace {

constexpr int kOrderThreads = 1024, kOrderWaves = kOrderThreads / 64;
constexpr int kKeyDigits = 6;   // 8-bit digits over the key's 45 bits

__device__ inline int32_t wave_min(int32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ inline int32_t wave_max(int32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

}  // namespace

// One block does all of it, its steps ordered by __syncthreads (as tlas4_refit_kernel): at most 32 767 keys are less work than a
// grid-wide handshake costs, and no block ever waits for another.
//   1. the bounds of the finite centres per axis: per-thread, per-wave, then sixteen LDS integer atomics per bound on ordered keys
//   2. the keys
//   3. an LSD radix sort, six passes of 8 bits.  Per pass the digits' histogram (LDS atomics) and its exclusive scan give every
//      digit's first position; then the keys go through in tiles of 1024, in order: inside a wave a key's rank among the equal
//      digits before it comes from eight ballots, across the tile's sixteen waves from a per-digit walk over the waves' counts.
//      Stable, so the six passes sort; the keys are unique, so the result is THE sorted order.
// kLds: both key buffers in LDS (n <= kTlasLdsKeys); otherwise in `scratch` (2 n keys of device memory: written and read by this
// block only, across __syncthreads).
template <bool kLds>
__global__ __launch_bounds__(kOrderThreads) void tlas_order_kernel(const float* __restrict__ lo, const float* __restrict__ hi, uint32_t stride,
                                                                   uint32_t n, uint64_t* __restrict__ keys_out, uint64_t* __restrict__ scratch,
                                                                   uint32_t* __restrict__ sorted_out)
{
    __shared__ int32_t s_bound[6];
    __shared__ uint32_t s_first[256];                // a digit's histogram, then the next position of the digit
    __shared__ uint32_t s_wave_total[4];
    __shared__ uint16_t s_count[kOrderWaves][256];   // per wave of the tile: keys with the digit (zero between tiles)
    __shared__ uint16_t s_offset[kOrderWaves][256];  // ... and where the wave's first of them goes
    __shared__ uint64_t s_keys[kLds ? 2 * kTlasLdsKeys : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    if (tid < 3) s_bound[tid] = kTlasKeyBoundsMin;
    else if (tid < 6) s_bound[tid] = kTlasKeyBoundsMax;
    for (uint32_t j = tid; j < (uint32_t)kOrderWaves * 256u; j += kOrderThreads) (&s_count[0][0])[j] = 0;
    __syncthreads();
    {
        int32_t kmin[3] = {kTlasKeyBoundsMin, kTlasKeyBoundsMin, kTlasKeyBoundsMin}, kmax[3] = {kTlasKeyBoundsMax, kTlasKeyBoundsMax, kTlasKeyBoundsMax};
        for (uint32_t i = tid; i < n; i += kOrderThreads)
            for (int k = 0; k < 3; k++) {
                const float c = tlas_centre(lo[(size_t)i * stride + k], hi[(size_t)i * stride + k]);
                const int32_t key = ordered_key(c);
                const bool fin = tlas_finite(c);
                kmin[k] = fin ? min(kmin[k], key) : kmin[k];
                kmax[k] = fin ? max(kmax[k], key) : kmax[k];
            }
        for (int k = 0; k < 3; k++) {
            const int32_t a = wave_min(kmin[k]), b = wave_max(kmax[k]);
            if (lane == 0) {
                atomicMin(&s_bound[k], a);
                atomicMax(&s_bound[3 + k], b);
            }
        }
    }
    __syncthreads();
    uint64_t* from = kLds ? s_keys : scratch;
    uint64_t* to = from + (kLds ? kTlasLdsKeys : n);
    {
        float bmin[3], inv[3];
        for (int k = 0; k < 3; k++) {
            bmin[k] = from_ordered_key(s_bound[k]);
            inv[k] = tlas_inv_extent(bmin[k], from_ordered_key(s_bound[3 + k]));
        }
        for (uint32_t i = tid; i < n; i += kOrderThreads) {
            const float l[3] = {lo[(size_t)i * stride], lo[(size_t)i * stride + 1], lo[(size_t)i * stride + 2]};
            const float h[3] = {hi[(size_t)i * stride], hi[(size_t)i * stride + 1], hi[(size_t)i * stride + 2]};
            const uint64_t key = tlas_key(l, h, bmin, inv, i);
            from[i] = key;
            if (keys_out) keys_out[i] = key;
        }
    }
    __syncthreads();
    for (int pass = 0; pass < kKeyDigits; pass++) {
        const int shift = 8 * pass;
        if (tid < 256) s_first[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kOrderThreads) atomicAdd(&s_first[(uint32_t)(from[i] >> shift) & 255u], 1u);
        __syncthreads();
        // exclusive scan of the 256 counts by the first four waves
        uint32_t own = 0, incl = 0;
        if (tid < 256) {
            own = incl = s_first[tid];
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if ((int)lane >= d) incl += up;
            }
            if (lane == 63) s_wave_total[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t base = 0;
            for (uint32_t w = 0; w < wave; w++) base += s_wave_total[w];
            s_first[tid] = base + incl - own;
        }
        __syncthreads();
        for (uint32_t tile = 0; tile < n; tile += kOrderThreads) {
            const uint32_t i = tile + tid;
            const bool valid = i < n;
            const uint64_t key = valid ? from[i] : 0ull;
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            // the lanes of this wave that hold the same digit
            unsigned long long same = __ballot(valid);
            for (int b = 0; b < 8; b++) {
                const bool bit = (digit >> b) & 1u;
                const unsigned long long with = __ballot(valid && bit);
                same &= bit ? with : ~with;
            }
            const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            if (valid && rank == 0) s_count[wave][digit] = (uint16_t)__popcll(same);
            __syncthreads();
            if (tid < 256) {
                uint32_t run = s_first[tid];
                for (int w = 0; w < kOrderWaves; w++) {
                    const uint32_t cnt = s_count[w][tid];
                    s_offset[w][tid] = (uint16_t)run;   // (n <= 32 767)
                    s_count[w][tid] = 0;
                    run += cnt;
                }
                s_first[tid] = run;
            }
            __syncthreads();
            if (valid) to[(uint32_t)s_offset[wave][digit] + rank] = key;
            // (the next tile's counts are written after its ballots and read after its first barrier: nobody is still here then)
        }
        __syncthreads();
        uint64_t* t = from;
        from = to;
        to = t;
    }
    // an even number of passes: the sorted keys are where the keys were made
    for (uint32_t i = tid; i < n; i += kOrderThreads) sorted_out[i] = (uint32_t)(from[i] & 0x7fffull);
}

// One thread per record of the template: its child words into the tail at `base`, internal references shifted by the base, a leaf
// slot over sorted position p naming instance sorted[p].  Empty slots get the empty box (the refit leaves them alone); the boxes of
// the others are the refit's to write.
__global__ __launch_bounds__(256) void tlas_template_kernel(const int32_t* __restrict__ tmpl, uint32_t n_records, const uint32_t* __restrict__ sorted,
                                                            WideNode4* __restrict__ nodes4, uint32_t base)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    WideNode4& o = nodes4[base + r];
    for (int k = 0; k < 4; k++) {
        const int32_t c = tmpl[(size_t)r * 4 + k];
        o._pad[k] = 0u;   // (the tail beyond the last upload's records has never been written)
        if (c == kEmptyChild) {
            o.lo_x[k] = o.lo_y[k] = o.lo_z[k] = 3.402823466e38f;
            o.hi_x[k] = o.hi_y[k] = o.hi_z[k] = -3.402823466e38f;
            o.child[k] = kEmptyChild;
        } else {
            o.child[k] = c >= 0 ? c + (int32_t)base : ~(int32_t)sorted[(uint32_t)~c];
        }
    }
}

// the records of one TLAS tail into another, internal references rebased: a refit into a copy of the instance level that still
// holds an older topology starts from the current copy's
__global__ __launch_bounds__(256) void tlas_tail_copy_kernel(WideNode4* __restrict__ nodes4, uint32_t from_base, uint32_t to_base, uint32_t n_records)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    WideNode4 rec = nodes4[from_base + r];
    for (int k = 0; k < 4; k++)
        if (rec.child[k] >= 0) rec.child[k] = rec.child[k] - (int32_t)from_base + (int32_t)to_base;
    nodes4[to_base + r] = rec;
}

void launch_tlas_order(hipStream_t stream, const float* lo, const float* hi, uint32_t stride, uint32_t n, uint64_t* keys_out, uint64_t* scratch,
                       uint32_t* sorted_out)
{
    if (n == 0) return;
    if (n <= kTlasLdsKeys)
        hipLaunchKernelGGL(tlas_order_kernel<true>, dim3(1), dim3(kOrderThreads), 0, stream, lo, hi, stride, n, keys_out, scratch, sorted_out);
    else
        hipLaunchKernelGGL(tlas_order_kernel<false>, dim3(1), dim3(kOrderThreads), 0, stream, lo, hi, stride, n, keys_out, scratch, sorted_out);
}

void launch_tlas_template(hipStream_t stream, const int32_t* tmpl, uint32_t n_records, const uint32_t* sorted, WideNode4* nodes4, uint32_t base)
{
    if (n_records == 0) return;
    hipLaunchKernelGGL(tlas_template_kernel, dim3((n_records + 255) / 256), dim3(256), 0, stream, tmpl, n_records, sorted, nodes4, base);
}

void launch_tlas_tail_copy(hipStream_t stream, WideNode4* nodes4, uint32_t from_base, uint32_t to_base, uint32_t n_records)
{
    if (n_records == 0 || from_base == to_base) return;
    hipLaunchKernelGGL(tlas_tail_copy_kernel, dim3((n_records + 255) / 256), dim3(256), 0, stream, nodes4, from_base, to_base, n_records);
}

}  // namespace jpt
