// jpt_kernels_bake_dir.hip -- the moment kernel of directional lightmaps (jpt_set_bake_directional; the arithmetic: jpt_bake_dir.h),
// launched by launch_wf2_render directly behind wf2_accumulate, and the host loop of jpt_debug_bake_moments.
//
// bake_moments reads what wf2_accumulate has just read -- every frame's finished value per (slot, frame), rad or fin8 -- before the
// render's workspace is given back, recomputes the direction in which each frame's path left its texel and adds value * direction to
// the three planes.  No path kernel knows about it.
#include <string>
#include <vector>

#include "../../include/jpt.h"
#include "jpt_bake_dir.h"
#include "jpt_kernels.h"

namespace jpt {
namespace {

constexpr int kDirBlock = 256;   // four waves, each one 8 x 8 tile

typedef float dir_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t dir_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 dir_ld4(const float4* p)
{
    const dir_v4f v = __builtin_nontemporal_load(reinterpret_cast<const dir_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 dir_ldu4(const uint4* p)
{
    const dir_v4u v = __builtin_nontemporal_load(reinterpret_cast<const dir_v4u*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void dir_st4(float4* p, const float4 v)
{
    dir_v4f w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<dir_v4f*>(p));
}
__device__ __forceinline__ f3 dir_word(uint32_t q)   // the rgba8 load of progressive_rendering.glsl:33, as wf2_accumulate makes it
{
    return mk3(from_unorm8(q & 255u), from_unorm8((q >> 8) & 255u), from_unorm8((q >> 16) & 255u));
}

// One thread per texel of the context's share, tile by tile exactly as wf2_accumulate walks it: a wave is one 8 x 8 tile, a texel's
// frames are one run of rad / fin8, and a tile row's store into a plane is 128 contiguous bytes.  `slot` is the texel's place in the
// render's window, which for a bake render is the whole share (no sky cull: PrimaryRays::sky_cull()).
__global__ __launch_bounds__(kDirBlock) void bake_moments(BakeDirArgs a, FrameParams fp)
{
    const uint32_t slot = blockIdx.x * (uint32_t)kDirBlock + threadIdx.x;
    const uint32_t tile = slot >> 6, lane = slot & 63u;
    const uint32_t ty = tile / (uint32_t)a.full_tiles_x, tx = tile - ty * (uint32_t)a.full_tiles_x;
    if ((int)ty >= a.full_tiles_y) return;   // (the whole wave)
    const int px = (int)(tx * 8u + (lane & 7u)), ly = (int)(ty * 8u + (lane >> 3));
    if (px >= fp.width || ly >= fp.local_rows) return;
    const size_t idx = (size_t)ly * (size_t)fp.width + (size_t)px, plane = (size_t)fp.width * (size_t)fp.local_rows;
    const int py = local_to_global_row(ly, fp);
    const float4 n4 = a.normal[(size_t)py * (size_t)fp.width + (size_t)px];
    if (!bake_texel_valid(n4)) {   // +0 in all nine values, whatever the planes held
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        dir_st4(&a.planes[idx], zero);
        dir_st4(&a.planes[plane + idx], zero);
        dir_st4(&a.planes[2 * plane + idx], zero);
        return;
    }
    // fp.frame_count = ProgressiveRendering frame_count of the FIRST frame of this render, as in wf2_accumulate
    bool have_prev = fp.frame_count > 1;
    BakeMoments M;
    M.m[0] = M.m[1] = M.m[2] = mk3(0.0f, 0.0f, 0.0f);
    if (have_prev) {
        const float4 mx = dir_ld4(&a.planes[idx]), my = dir_ld4(&a.planes[plane + idx]), mz = dir_ld4(&a.planes[2 * plane + idx]);
        M.m[0] = mk3(mx.x, mx.y, mx.z);
        M.m[1] = mk3(my.x, my.y, my.z);
        M.m[2] = mk3(mz.x, mz.y, mz.z);
    }
    const BakeDirTexel t = bake_dir_texel(n4);
    // rgba8 samples, one frame group, a multiple of four frames: a texel's frames are consecutive 16-byte pieces of fin8 (wf2_accumulate's
    // packed-frames case, here for any such count: the next piece is in flight while the four directions of this one are made)
    const bool packed_frames = fp.accum_mode == 0 && a.groups == 1 && (fp.n_frames & 3) == 0;
    if (packed_frames) {
        const uint4* mine = reinterpret_cast<const uint4*>(a.fin8 + (size_t)slot * (size_t)fp.n_frames);
        const int pieces = fp.n_frames >> 2;
        uint4 next = dir_ldu4(&mine[0]);
        for (int c = 0; c < pieces; c++) {
            const uint4 q = next;
            if (c + 1 < pieces) next = dir_ldu4(&mine[c + 1]);
            const uint32_t f0 = fp.frame_index + 4u * (uint32_t)c;
            bake_moments_add(M, have_prev, dir_word(q.x), bake_dir_frame(t, px, py, f0));
            bake_moments_add(M, true, dir_word(q.y), bake_dir_frame(t, px, py, f0 + 1u));
            bake_moments_add(M, true, dir_word(q.z), bake_dir_frame(t, px, py, f0 + 2u));
            bake_moments_add(M, true, dir_word(q.w), bake_dir_frame(t, px, py, f0 + 3u));
            have_prev = true;
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
                cur = dir_word(__builtin_nontemporal_load(&a.fin8[at]));
            } else {
                const float4 r = dir_ld4(&a.rad[at]);
                cur = mk3(r.x, r.y, r.z);
            }
            bake_moments_add(M, have_prev, cur, bake_dir_frame(t, px, py, fp.frame_index + (uint32_t)f));
            have_prev = true;
        }
    }
    dir_st4(&a.planes[idx], make_float4(M.m[0].x, M.m[0].y, M.m[0].z, 0.0f));
    dir_st4(&a.planes[plane + idx], make_float4(M.m[1].x, M.m[1].y, M.m[1].z, 0.0f));
    dir_st4(&a.planes[2 * plane + idx], make_float4(M.m[2].x, M.m[2].y, M.m[2].z, 0.0f));
}

}  // namespace

void launch_bake_moments(hipStream_t stream, const BakeDirArgs& a, const FrameParams& fp)
{
    if (fp.n_frames <= 0 || a.full_tiles_x <= 0 || a.full_tiles_y <= 0) return;
    const uint32_t blocks = ((uint32_t)a.full_tiles_x * (uint32_t)a.full_tiles_y * 64u + (uint32_t)kDirBlock - 1u) / (uint32_t)kDirBlock;
    hipLaunchKernelGGL(bake_moments, dim3(blocks), dim3(kDirBlock), 0, stream, a, fp);
}

// the same sum on the host, over the caller's arrays: the functions of jpt_bake_dir.h in a plain loop
void bake_moments_host(const float4* normal4, int32_t width, int32_t height, const float* radiance3, int32_t n_frames, uint32_t first_frame_index,
                       uint32_t frame_count, int32_t accum_mode, float* moments)
{
    const size_t n = (size_t)width * (size_t)height;
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            BakeMoments M;
            if (!bake_texel_valid(normal4[i])) {
                for (int k = 0; k < 3; k++)
                    for (int c = 0; c < 4; c++) moments[(k * n + i) * 4 + c] = 0.0f;
                continue;
            }
            bool have_prev = frame_count > 1;
            for (int k = 0; k < 3; k++) M.m[k] = have_prev ? mk3(moments[(k * n + i) * 4], moments[(k * n + i) * 4 + 1], moments[(k * n + i) * 4 + 2]) : mk3(0.0f, 0.0f, 0.0f);
            const BakeDirTexel t = bake_dir_texel(normal4[i]);
            for (int32_t f = 0; f < n_frames; f++) {
                const float* r = radiance3 + ((size_t)f * n + i) * 3;
                f3 cur = mk3(r[0], r[1], r[2]);
                if (accum_mode == JPT_ACCUM_REF_LDR8) cur = bake_dir_ldr8(cur);
                bake_moments_add(M, have_prev, cur, bake_dir_frame(t, x, y, first_frame_index + (uint32_t)f));
                have_prev = true;
            }
            for (int k = 0; k < 3; k++) {
                float* o = moments + (k * n + i) * 4;
                o[0] = M.m[k].x;
                o[1] = M.m[k].y;
                o[2] = M.m[k].z;
                o[3] = 0.0f;
            }
        }
}

}  // namespace jpt

using namespace jpt;

extern "C" {

int jpt_debug_bake_moments(const float* position4, const float* normal4, int32_t width, int32_t height, const float* radiance3, int32_t n_frames,
                           uint32_t first_frame_index, uint32_t frame_count, int32_t accum_mode, float* moments_inout)
{
    std::string why;
    int rc = check_bake_size("jpt_debug_bake_moments", width, height, why);
    if (rc == JPT_OK && (!position4 || !normal4 || !moments_inout || (n_frames > 0 && !radiance3))) {
        why = "jpt_debug_bake_moments: null argument";
        rc = JPT_E_INVALID;
    }
    if (rc == JPT_OK && n_frames < 0) {
        why = "jpt_debug_bake_moments: n_frames < 0";
        rc = JPT_E_INVALID;
    }
    if (rc == JPT_OK && frame_count == 0) {
        why = "jpt_debug_bake_moments: frame_count starts at 1 (the first frame after a reset)";
        rc = JPT_E_INVALID;
    }
    if (rc == JPT_OK && accum_mode != JPT_ACCUM_REF_LDR8 && accum_mode != JPT_ACCUM_HDR_F32) {
        why = "jpt_debug_bake_moments: unknown accum_mode";
        rc = JPT_E_INVALID;
    }
    if (rc == JPT_OK) rc = check_bake_texels("jpt_debug_bake_moments", position4, normal4, (size_t)width * (size_t)height, why);
    if (rc != JPT_OK) {
        set_debug_error(why);
        return rc;
    }
    if (n_frames == 0) return JPT_OK;   // (a render of no frames launches nothing: the planes stay)
    // (normal4 need not be 16-byte aligned: copied)
    std::vector<float4> n((size_t)width * (size_t)height);
    for (size_t i = 0; i < n.size(); i++) n[i] = make_float4(normal4[4 * i], normal4[4 * i + 1], normal4[4 * i + 2], normal4[4 * i + 3]);
    bake_moments_host(n.data(), width, height, radiance3, n_frames, first_frame_index, frame_count, accum_mode, moments_inout);
    return JPT_OK;
}

}  // extern "C"
