// jpt_kernels_reflection.hip -- jpt_reflection_prefilter: every reflection probe's strip of the accumulation image turned into a
// GGX-prefiltered mip chain (the arithmetic and the two images' layouts: jpt_reflection.h, where reflection_prefilter_host restates the
// transform for the host).
//
// refl_chain_kernel builds one level of the source chain per launch, one thread per output texel: level 0 reads the accumulation (one
// 16-byte load) and divides by the frame count, level m + 1 reads its 2 x 2 block of level m (four 16-byte loads).
//
// refl_prefilter_kernel: a 256-thread block takes 256 consecutive output texels of one (probe, level).  The grid is probe-major -- all
// the blocks of a probe's levels are consecutive block ids -- so the blocks in flight at one time gather from a few probes' source
// chains (2.1 MB each at S = 128), not from all of them.  The level's table is staged once per block in LDS (4 KB of entries and 256
// level bytes); the sample index is wave-uniform, so the table reads are broadcasts.  Per sample a lane rotates the entry into its
// texel's frame, finds the face and the texel of the entry's source level and gathers 16 bytes.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "jpt_kernels.h"

namespace jpt {

namespace {

constexpr int kReflBlock = 256;

__global__ __launch_bounds__(kReflBlock) void refl_chain_kernel(ReflDev rd, uint32_t m, const float4* __restrict__ accum, float frame_count,
                                                                float4* __restrict__ chain)
{
    const uint32_t shift = rd.shift, ls = shift - m, s = 1u << ls;   // this level's size
    // (a level has at most as many texels as the image has pixels, 2^26: 32-bit indices, and the / 6 is probe_div's)
    const uint32_t total = (rd.n * 6u) << (2u * ls);
    const uint32_t at = blockIdx.x * (uint32_t)kReflBlock + threadIdx.x;
    if (at >= total) return;
    const uint32_t pf = at >> (2u * ls), p = probe_div(pf, kCubeInv6), f = pf - p * 6u;
    const uint32_t j = (at >> ls) & (s - 1u), i = at & (s - 1u);
    const uint32_t r = (f << (2u * ls)) | (j << ls) | i;   // the texel within the probe's level
    float4* probe_chain = chain + (uint64_t)p * (uint64_t)((8u << (2u * shift)) - 2u);
    const uint32_t ss = 1u << (2u * shift);
    float4 v;
    if (m == 0u) {
        const uint32_t trow = p / rd.per_row, tcol = p - trow * rd.per_row;
        const size_t width = (size_t)rd.per_row * 6u * s;
        const float4 a = accum[((size_t)trow * s + j) * width + ((size_t)tcol * 6u + f) * s + i];
        v = make_float4(a.x / frame_count, a.y / frame_count, a.z / frame_count, 0.0f);
    } else {
        const uint32_t s0 = s << 1;
        const float4* src = probe_chain + 8u * (ss - s0 * s0) + ((size_t)f * s0 + 2u * j) * s0 + 2u * i;
        const float4 a = src[0], b = src[1], c = src[s0], d = src[s0 + 1u];
        v = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.0f);
    }
    probe_chain[8u * (ss - s * s) + r] = v;
}

// blocks of 256 texels that level l of one probe takes
__host__ __device__ __forceinline__ uint32_t level_blocks(uint32_t shift, uint32_t l)
{
    return ((6u << (2u * (shift - l))) + (uint32_t)kReflBlock - 1u) / (uint32_t)kReflBlock;
}

__global__ __launch_bounds__(kReflBlock) void refl_prefilter_kernel(ReflDev rd, uint32_t blocks_per_probe, const float4* __restrict__ chain,
                                                                    const float4* __restrict__ table, const uint8_t* __restrict__ levels,
                                                                    float4* __restrict__ out)
{
    __shared__ float4 s_tab[kReflSamplesMax];
    __shared__ uint8_t s_lvl[kReflSamplesMax];
    const uint32_t shift = rd.shift;
    // (block-uniform, on the scalar unit: the probe, then the level this block belongs to and its first texel)
    const uint32_t p = blockIdx.x / blocks_per_probe;
    uint32_t blk = blockIdx.x - p * blocks_per_probe, l = 0;
    for (;;) {
        const uint32_t nb = level_blocks(shift, l);
        if (blk < nb) break;
        blk -= nb;
        l++;
    }
    const uint32_t count = l == 0u ? 0u : rd.count[l];
    if (threadIdx.x < count) {
        s_tab[threadIdx.x] = table[(size_t)l * rd.samples + threadIdx.x];
        s_lvl[threadIdx.x] = levels[(size_t)l * rd.samples + threadIdx.x];
    }
    __syncthreads();
    const uint32_t ls = shift - l, s = 1u << ls, per_probe = 6u << (2u * ls);
    const uint32_t r = blk * (uint32_t)kReflBlock + threadIdx.x;
    if (r >= per_probe) return;
    const float4* probe_chain = chain + (uint64_t)p * (uint64_t)((8u << (2u * shift)) - 2u);
    const uint32_t ss = 1u << (2u * shift);
    float4* dst = out + (uint64_t)rd.n * (8u * (ss - s * s)) + (uint64_t)p * per_probe + r;
    if (l == 0u) {
        const float4 c = probe_chain[r];
        *dst = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    const uint32_t f = r >> (2u * ls), j = (r >> ls) & (s - 1u), i = r & (s - 1u);
    *dst = refl_texel(probe_chain, shift, f, i, j, s, s_tab, s_lvl, count);
}

}  // namespace

void launch_reflection_chain(hipStream_t stream, const ReflDev& rd, const float4* accum, float frame_count, float4* chain)
{
    for (uint32_t m = 0; m <= rd.shift; m++) {
        const uint64_t total = (uint64_t)rd.n * (6ull << (2u * (rd.shift - m)));
        const unsigned blocks = (unsigned)((total + (uint64_t)kReflBlock - 1) / (uint64_t)kReflBlock);
        hipLaunchKernelGGL(refl_chain_kernel, dim3(blocks), dim3(kReflBlock), 0, stream, rd, m, accum, frame_count, chain);
    }
}

void launch_reflection_prefilter(hipStream_t stream, const ReflDev& rd, const float4* chain, const float4* table, const uint8_t* levels, float4* out)
{
    uint32_t per_probe = 0;
    for (uint32_t l = 0; l < rd.n_levels; l++) per_probe += level_blocks(rd.shift, l);
    hipLaunchKernelGGL(refl_prefilter_kernel, dim3(rd.n * per_probe), dim3(kReflBlock), 0, stream, rd, per_probe, chain, table, levels, out);
}

}  // namespace jpt
