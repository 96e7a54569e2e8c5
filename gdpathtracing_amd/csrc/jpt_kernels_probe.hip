// jpt_kernels_probe.hip -- jpt_probe_project: every probe's tile of the accumulation image reduced to nine L2 SH coefficients per
// colour channel (the sum and its order: jpt_probe.h, where probe_project_host restates it for the host).
//
// One wave per probe, four probes per 256-thread block.  The quadrature table (cells * 9 floats, at most 36 KB) is staged once per
// block in LDS; a lane reads its cells' sums with one 16-byte load each -- consecutive lanes take consecutive pixels of a tile row --
// and the table's nine entries of the cell from LDS (a stride of 9 words between lanes: no bank conflict).  The 27 accumulators are
// then summed across the wave by six butterfly steps: lane ^ 1, ^ 2 and ^ 8 are DPP modifiers of the add itself (quad_perm, row_ror:8),
// lane ^ 4, ^ 16 and ^ 32 a ds_bpermute and an add.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "jpt_kernels.h"

namespace jpt {

namespace {

constexpr int kProjBlock = 256;
constexpr int kProjProbes = kProjBlock / 64;   // probes (waves) per block

template <int CTRL>
__device__ __forceinline__ float dpp_read(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// v + v[lane ^ S] in every lane of a full wave
template <int S>
__device__ __forceinline__ float butterfly_add(float v)
{
    if constexpr (S == 1) return v + dpp_read<0xB1>(v);         // quad_perm:[1,0,3,2]
    else if constexpr (S == 2) return v + dpp_read<0x4E>(v);    // quad_perm:[2,3,0,1]
    else if constexpr (S == 8) return v + dpp_read<0x128>(v);   // row_ror:8 (a row is 16 lanes)
    else return v + __shfl_xor(v, S);
}

__global__ __launch_bounds__(kProjBlock) void probe_project_kernel(ProbeDev pd, const float4* __restrict__ accum, float frame_count,
                                                                   const float* __restrict__ table, float4* __restrict__ out)
{
    __shared__ float s_table[kProbeMaxCells * 9];
    const uint32_t tile_w = pd.tile_w(), tile_h = pd.tile_h(), cells = tile_w * tile_h;
    for (uint32_t k = threadIdx.x; k < cells * 9u; k += (uint32_t)kProjBlock) s_table[k] = table[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * (uint32_t)kProjProbes + (threadIdx.x >> 6);   // (wave-uniform)
    if (p >= pd.n) return;
    const uint32_t trow = p / pd.per_row, tcol = p - trow * pd.per_row;
    const size_t width = (size_t)pd.per_row * tile_w;
    const float4* tile = accum + (size_t)trow * tile_h * width + (size_t)tcol * tile_w;
    float acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0f;
    for (uint32_t c = lane; c < cells; c += 64u) {
        const uint32_t j = probe_div(c, pd.inv_w), i = c - j * tile_w;
        const float4 px = tile[(size_t)j * width + i];
        const float m[3] = {px.x / frame_count, px.y / frame_count, px.z / frame_count};
        const float* t = &s_table[c * 9u];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const float tk = t[k];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float term = m[ch] * tk;
                acc[3 * k + ch] = acc[3 * k + ch] + term;
            }
        }
    }
    // (every lane of the wave is here: the loop's trip counts differ, its exit does not leave lanes behind)
#pragma unroll
    for (int k = 0; k < 27; k++) {
        float v = acc[k];
        v = butterfly_add<32>(v);
        v = butterfly_add<16>(v);
        v = butterfly_add<8>(v);
        v = butterfly_add<4>(v);
        v = butterfly_add<2>(v);
        v = butterfly_add<1>(v);
        acc[k] = v;
    }
    // lanes 0..8 store one float4 each: 144 contiguous bytes per probe (every lane holds every sum; the coefficient is picked without
    // indexing the register array by a lane-dependent value)
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (lane == (uint32_t)k) {
            r = acc[3 * k];
            g = acc[3 * k + 1];
            b = acc[3 * k + 2];
        }
    if (lane < 9u) out[(size_t)p * 9 + lane] = make_float4(r, g, b, 0.0f);
}

}  // namespace

void launch_probe_project(hipStream_t stream, const ProbeDev& pd, const float4* accum, float frame_count, const float* table, float4* out)
{
    const unsigned blocks = (pd.n + (uint32_t)kProjProbes - 1u) / (uint32_t)kProjProbes;
    hipLaunchKernelGGL(probe_project_kernel, dim3(blocks), dim3(kProjBlock), 0, stream, pd, accum, frame_count, table, out);
}

}  // namespace jpt
