// jpt_cube.h -- reflection probes, the capture (jpt_set_reflection_probes): one render holds a strip of six cube faces per probe, side
// by side, and jpt_reflection_prefilter (jpt_reflection.h) turns every strip into a GGX-prefiltered mip chain on the device.  Nothing
// downstream of ray generation knows: the rays go into the queues as they are, like the lens's, the camera models', the bake's and the
// light probes'.
//
// Layout.  With S = face_size, probe p owns the strip 6 S wide and S high whose top-left pixel is ((p % per_row) * 6 S, (p / per_row) * S);
// face f of the strip is the S x S square at x = f * S.  The image is per_row * 6 S wide and ceil(n / per_row) * S high.  A pixel of a
// strip with index >= n has no path: radiance 0, first-hit distance cam.far_, no ray counted -- exactly like a tile without a light probe.
//
// The map.  Texel (i, j) of a face covers a in [2 i / S - 1, 2 (i + 1) / S - 1) and b likewise in j; the direction is normalize3 of the
// OpenGL cube-map face table (the one Godot's cubemaps use):
//     face 0 = +X  ( 1, -b, -a)      face 1 = -X  (-1, -b,  a)
//     face 2 = +Y  ( a,  1,  b)      face 3 = -Y  ( a, -1, -b)
//     face 4 = +Z  ( a, -b,  1)      face 5 = -Z  (-a, -b, -1)
// so a texel's accumulated mean is its box-filtered radiance in face coordinates.
//
// The arithmetic of the ray is pinned (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations, restated in numpy by
// tests/np_reflection.py); host and device run these functions (the *_cube forms of the primary kernels, the audit kernel and
// jpt_debug_cube_rays).
//
// Out of scope: box projection / parallax correction, blending between probes, an octahedral layout, a jpt_multi_* form.
#pragma once

#include "jpt_probe.h"

namespace jpt {

constexpr int32_t kCubeFaceMin = 4, kCubeFaceMax = 256;   // face_size: a power of two
constexpr int32_t kCubeMaxProbes = 1 << 20;
constexpr uint64_t kCubeMaxPixels = 1ull << 26;            // the image
// the two constants a cube ray's (xi0, xi1) are hashed with: this feature's own (the bake's are 0x3c6ef372, 0xa54ff53a, the light
// probes' 0x510e527f, 0x9b05688c)
constexpr uint32_t kCubeHashX = 0x1f83d9abu, kCubeHashY = 0x5be0cd19u;
// floor(2^32 / 6) + 1: (x * kCubeInv6) >> 32 == x / 6 for every x < 2^26 (the error term x * 6 stays below 2^32), as probe_div's
constexpr uint32_t kCubeInv6 = 0x2aaaaaabu;

// The reflection probes of one render, passed by value to its bounce-0 launch: a null pointer is a camera render (nothing is read
// then).  shift: log2 of the face size, so the divisions of a pixel into (probe, face, i, j) are shifts and masks by a wave-uniform
// value plus one v_mul_hi_u32 for the / 6.  Five scalar registers -- two fewer than ProbeDev, whose note (jpt_probe.h) says why the
// count matters: the bounce-0 kernels live at the limit of theirs, and the face size's float form is made per refill from the shift.
struct CubeDev {
    const float* position = nullptr;   // n * 3, world space
    uint32_t n = 0, per_row = 0, shift = 0;
    __host__ __device__ uint32_t face_size() const { return 1u << shift; }
};

inline int32_t cube_log2(int32_t face_size)
{
    int32_t s = 0;
    while ((1 << s) < face_size) s++;
    return s;
}

inline CubeDev make_cube_dev(const float* position, int32_t n, int32_t face_size, int32_t per_row)
{
    CubeDev cd;
    cd.position = position;
    cd.n = (uint32_t)n;
    cd.per_row = (uint32_t)per_row;
    cd.shift = (uint32_t)cube_log2(face_size);
    return cd;
}

inline void cube_image_size(int32_t n, int32_t face_size, int32_t per_row, uint64_t& width, uint64_t& height)
{
    width = (uint64_t)per_row * 6u * (uint64_t)face_size;
    height = (((uint64_t)n + (uint64_t)per_row - 1) / (uint64_t)per_row) * (uint64_t)face_size;
}

#if defined(__HIPCC__)

// pixel (px, py) of the image -> its probe, its face and its texel of the face; false: the strip has no probe
__host__ __device__ __forceinline__ bool cube_cell(const CubeDev& cd, int px, int py, uint32_t& p, uint32_t& f, uint32_t& i, uint32_t& j)
{
    const uint32_t mask = cd.face_size() - 1u;
    const uint32_t fx = (uint32_t)px >> cd.shift, col = probe_div(fx, kCubeInv6), row = (uint32_t)py >> cd.shift;
    f = fx - col * 6u;
    i = (uint32_t)px & mask;
    j = (uint32_t)py & mask;
    p = row * cd.per_row + col;
    return p < cd.n;
}

// the face table: the direction of (a, b) on face f, before normalize3
__host__ __device__ __forceinline__ f3 cube_face_direction(uint32_t f, float a, float b)
{
    const float na = -a, nb = -b;
    if (f < 2u) return f == 0u ? mk3(1.0f, nb, na) : mk3(-1.0f, nb, a);
    if (f < 4u) return f == 2u ? mk3(a, 1.0f, b) : mk3(a, -1.0f, nb);
    return f == 4u ? mk3(a, nb, 1.0f) : mk3(na, nb, -1.0f);
}

// The first ray of pixel (px, py)'s path of frame `frame`, texel (i, j) of face f of a cube of face size `size` at `o`:
//   the seeds and the jitter draw of primary_ray, taken and discarded, so (sx, sy) leave as they do under a camera and every later
//   vertex draws what it draws today; (xi0, xi1) from one pcg2d round of a COPY (sx ^ kCubeHashX, sy ^ kCubeHashY); the face table,
//   normalised; no origin offset.
// its two halves, as probe_draw / probe_direction: the draws ...
__host__ __device__ __forceinline__ void cube_draw(int px, int py, uint32_t frame, uint32_t& sx, uint32_t& sy, float& xi0, float& xi1)
{
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    uint32_t hx = sx ^ kCubeHashX, hy = sy ^ kCubeHashY;
    pcg2d(hx, hy, xi0, xi1);
}
// ... and the map
__host__ __device__ __forceinline__ f3 cube_direction(uint32_t f, uint32_t i, uint32_t j, uint32_t size, float xi0, float xi1)
{
    const float s = (float)size;
    const float a = 2.0f * (((float)i + xi0) / s) - 1.0f;
    const float b = 2.0f * (((float)j + xi1) / s) - 1.0f;
    return normalize3(cube_face_direction(f, a, b));
}
__host__ __device__ __forceinline__ Ray cube_ray(const f3 o, uint32_t f, uint32_t i, uint32_t j, uint32_t size, int px, int py, uint32_t frame, uint32_t& sx,
                                                 uint32_t& sy)
{
    float xi0, xi1;
    cube_draw(px, py, frame, sx, sy, xi0, xi1);
    Ray ray;
    ray.o = o;
    ray.d = cube_direction(f, i, j, size, xi0, xi1);
    ray.rD = rcp3(ray.d);
    return ray;
}

__host__ __device__ __forceinline__ f3 cube_position(const CubeDev& cd, uint32_t p)
{
    const uint32_t at = 3u * p;   // (a 32-bit offset from the scalar base: p < 2^20)
    return mk3(cd.position[at], cd.position[at + 1u], cd.position[at + 2u]);
}

#endif  // __HIPCC__

}  // namespace jpt
