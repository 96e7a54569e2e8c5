// jpt_probe.h -- light probes (jpt_set_probes, jpt_probe_project): one render holds a small sphere tile per probe, side by side, and a
// post call reduces every tile to nine L2 spherical-harmonic coefficients per colour channel on the device.  Nothing downstream of ray
// generation knows: the rays go into the queues as they are, like the lens's, the camera models' and the bake's.
//
// Layout.  Probe p owns the tile_w x tile_h tile whose top-left pixel is ((p % per_row) * tile_w, (p / per_row) * tile_h); the image is
// per_row * tile_w wide and ceil(n / per_row) * tile_h high.  A pixel of a tile with index >= n has no path: radiance 0, first-hit
// distance cam.far_, no ray counted -- exactly like an invalid bake texel.
//
// The map.  Cell (i, j) of a tile covers u in [i, i + 1) / tile_w, v in [j, j + 1) / tile_h of the cylindrical equal-area map
//     phi = (u - 0.5) * 2 pi,  z = 1 - 2 v,  r = sqrt(1 - z^2),  d = (r sin phi, z, r cos phi)          (world axes)
// so every cell subtends 4 pi / (tile_w * tile_h): the polar axis is world +Y, row 0 is the up pole and the centre column is +Z -- the
// orientation of JPT_CAMERA_EQUIRECT with an identity basis.
//
// The basis.  Real spherical harmonics of bands 0..2 in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), written
// in the frame of the map, (X, Y, Z) = (d.z, d.x, d.y) -- a cyclic permutation of the world axes, so Z is the polar axis and phi the
// azimuth from X towards Y:
//     Y0 = 0.2820948
//     Y1 = 0.4886025 Y = 0.4886025 d.x        Y2 = 0.4886025 Z = 0.4886025 d.y        Y3 = 0.4886025 X = 0.4886025 d.z
//     Y4 = 1.0925484 X Y = 1.0925484 d.z d.x  Y5 = 1.0925484 Y Z = 1.0925484 d.x d.y  Y6 = 0.3153916 (3 Z^2 - 1) = 0.3153916 (3 d.y^2 - 1)
//     Y7 = 1.0925484 X Z = 1.0925484 d.z d.y  Y8 = 0.5462742 (X^2 - Y^2) = 0.5462742 (d.z^2 - d.x^2)
// In this frame every function is (a function of z) x (one Fourier mode of phi), which is what makes the cell means separable and the
// Gram matrix of the cell means diagonal on a uniform grid.
//
// The quadrature is a table of tile_w * tile_h * 9 floats made on the host in double (probe_basis_table, jpt_primary.cpp): the mean of
// Y_k over the cell (closed forms), times the cell's solid angle, divided by G_kk = sum over cells of w * mean^2, times the band's
// cosine-lobe factor (pi, 2 pi / 3, pi / 4) with JPT_PROBE_IRRADIANCE; rounded to float.  A column whose G_kk vanishes is zero: two rows
// of cells cannot tell Y6 from a constant (tile_h = 2) and four columns cannot see cos 2 phi (tile_w = 4, Y8).
//
// The arithmetic of the ray and of the sum is pinned (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations, restated in
// numpy by tests/np_probe.py); host and device run these functions (the *_probe forms of the primary kernels, the audit kernel, the
// projection kernel of jpt_kernels_probe.hip and the jpt_debug_probe_* entry points).
#pragma once

#include "jpt_shade.h"

namespace jpt {

constexpr int32_t kProbeTileWMin = 4, kProbeTileWMax = 64, kProbeTileHMin = 2, kProbeTileHMax = 32;
constexpr int32_t kProbeMaxCells = 1024;           // tile_w * tile_h: the table is at most 36 KB, staged in LDS
constexpr int32_t kProbeMaxProbes = 1 << 20;
constexpr uint64_t kProbeMaxPixels = 1ull << 26;   // the image
// The least Gram diagonal of a column the table keeps: below it the function's cell means vanish on the grid (exactly, or to rounding
// noise) and the column is zero -- the coefficient reads 0 instead of NaN.  Of the accepted tiles only tile_h = 2 (Y6) and tile_w = 4
// (Y8) have such a column; every other column of every accepted tile has a diagonal above 0.2 (1 in the continuous limit).
constexpr double kProbeGramMin = 1e-9;
// the two constants a probe ray's (xi0, xi1) are hashed with: this feature's own (the bake's are 0x3c6ef372, 0xa54ff53a)
constexpr uint32_t kProbeHashX = 0x510e527fu, kProbeHashY = 0x9b05688cu;

// The probes of one render, passed by value to its bounce-0 launch: a null pointer is a camera render (nothing is read then).
// tile: tile_w | tile_h << 8 (both fit a byte).  inv_w / inv_h: floor(2^32 / tile) + 1, so that (x * inv) >> 32 == x / tile for every x <
// 2^26 (tile <= 64: the error term x * tile stays below 2^32) -- the divisions of a pixel into (probe, i, j) are by wave-uniform values
// and cost a v_mul_hi_u32 each.  Seven scalar registers in all: the bounce-0 kernels live at the limit of theirs, and with the tile's
// sides as two integers and two floats beside these the walk's loop-invariant vector registers went to scratch (measured on the ISA).
struct ProbeDev {
    const float* position = nullptr;   // n * 3, world space
    uint32_t n = 0, per_row = 0, tile = 0;
    uint32_t inv_w = 0, inv_h = 0;
    __host__ __device__ uint32_t tile_w() const { return tile & 0xffu; }
    __host__ __device__ uint32_t tile_h() const { return tile >> 8; }
};

inline ProbeDev make_probe_dev(const float* position, int32_t n, int32_t tile_w, int32_t tile_h, int32_t per_row)
{
    ProbeDev pd;
    pd.position = position;
    pd.n = (uint32_t)n;
    pd.per_row = (uint32_t)per_row;
    pd.tile = (uint32_t)tile_w | ((uint32_t)tile_h << 8);
    pd.inv_w = (uint32_t)((1ull << 32) / (uint64_t)tile_w) + 1u;
    pd.inv_h = (uint32_t)((1ull << 32) / (uint64_t)tile_h) + 1u;
    return pd;
}

inline void probe_image_size(int32_t n, int32_t tile_w, int32_t tile_h, int32_t per_row, uint64_t& width, uint64_t& height)
{
    width = (uint64_t)per_row * (uint64_t)tile_w;
    height = (((uint64_t)n + (uint64_t)per_row - 1) / (uint64_t)per_row) * (uint64_t)tile_h;
}

#if defined(__HIPCC__)

__host__ __device__ __forceinline__ uint32_t probe_div(uint32_t x, uint32_t inv) { return (uint32_t)(((uint64_t)x * (uint64_t)inv) >> 32); }

// pixel (px, py) of the image -> its probe and its cell of the probe's tile; false: the tile has no probe
__host__ __device__ __forceinline__ bool probe_cell(const ProbeDev& pd, int px, int py, uint32_t& p, uint32_t& i, uint32_t& j)
{
    const uint32_t col = probe_div((uint32_t)px, pd.inv_w), row = probe_div((uint32_t)py, pd.inv_h);
    i = (uint32_t)px - col * pd.tile_w();
    j = (uint32_t)py - row * pd.tile_h();
    p = row * pd.per_row + col;
    return p < pd.n;
}

// The first ray of pixel (px, py)'s path of frame `frame`, cell (i, j) of a tile of tile_w x tile_h cells of the probe at `o`:
//   the seeds and the jitter draw of primary_ray, taken and discarded, so (sx, sy) leave as they do under a camera and every later
//   vertex draws what it draws today; (xi0, xi1) from one pcg2d round of a COPY (sx ^ kProbeHashX, sy ^ kProbeHashY); the map above,
//   not renormalised; no origin offset.
// its two halves, for the kernels that order them around their loads: the draws ...
__host__ __device__ __forceinline__ void probe_draw(int px, int py, uint32_t frame, uint32_t& sx, uint32_t& sy, float& xi0, float& xi1)
{
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    uint32_t hx = sx ^ kProbeHashX, hy = sy ^ kProbeHashY;
    pcg2d(hx, hy, xi0, xi1);
}
// ... and the map
__host__ __device__ __forceinline__ f3 probe_direction(uint32_t i, uint32_t j, uint32_t tile_w, uint32_t tile_h, float xi0, float xi1)
{
    const float u = ((float)i + xi0) / (float)tile_w;
    const float v = ((float)j + xi1) / (float)tile_h;
    const float phi = (u - 0.5f) * 6.2831853f;
    const float z = 1.0f - 2.0f * v;
    const float r = __builtin_sqrtf(1.0f - z * z);
    float sp, cp;
    sincos_(phi, sp, cp);
    return mk3(r * sp, z, r * cp);
}
__host__ __device__ __forceinline__ Ray probe_ray(const f3 o, uint32_t i, uint32_t j, uint32_t tile_w, uint32_t tile_h, int px, int py, uint32_t frame,
                                                  uint32_t& sx, uint32_t& sy)
{
    float xi0, xi1;
    probe_draw(px, py, frame, sx, sy, xi0, xi1);
    Ray ray;
    ray.o = o;
    ray.d = probe_direction(i, j, tile_w, tile_h, xi0, xi1);
    ray.rD = rcp3(ray.d);
    return ray;
}

__host__ __device__ __forceinline__ f3 probe_position(const ProbeDev& pd, uint32_t p)
{
    const uint32_t at = 3u * p;   // (a 32-bit offset from the scalar base: p < 2^20)
    return mk3(pd.position[at], pd.position[at + 1u], pd.position[at + 2u]);
}

#endif  // __HIPCC__

// ---- the projection (jpt_probe_project): the pinned sum, as the host runs it ----------------------------------------------------
//
// One wave per probe.  Lane l adds the cells l, l + 64, l + 128 ... in raster order (c = j * tile_w + i) into 27 accumulators that start
// at +0: mean = accum.rgb / (float)frame_count, each term mean * t and then an add (no contraction); six butterfly steps v = v +
// v[lane ^ s], s = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits (float addition is commutative).  out: (r, g, b, 0)
// per coefficient, 9 float4 per probe.  `accum` is the whole image, row-major, `width` = per_row * tile_w pixels wide.
inline void probe_project_host(const float* accum4, uint32_t frame_count, int32_t n, int32_t tile_w, int32_t tile_h, int32_t per_row, const float* table,
                               float* out)
{
    const size_t width = (size_t)per_row * (size_t)tile_w;
    const int32_t cells = tile_w * tile_h;
    const float fc = (float)frame_count;
    for (int32_t p = 0; p < n; p++) {
        const size_t x0 = (size_t)(p % per_row) * (size_t)tile_w, y0 = (size_t)(p / per_row) * (size_t)tile_h;
        float acc[64][27];
        for (int l = 0; l < 64; l++) {
            for (int k = 0; k < 27; k++) acc[l][k] = 0.0f;
            for (int32_t c = l; c < cells; c += 64) {
                const float* px = accum4 + 4 * ((y0 + (size_t)(c / tile_w)) * width + x0 + (size_t)(c % tile_w));
                const float m[3] = {px[0] / fc, px[1] / fc, px[2] / fc};
                for (int k = 0; k < 9; k++) {
                    const float t = table[(size_t)c * 9 + k];
                    for (int ch = 0; ch < 3; ch++) {
                        const float term = m[ch] * t;
                        acc[l][3 * k + ch] = acc[l][3 * k + ch] + term;
                    }
                }
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            float nxt[64][27];
            for (int l = 0; l < 64; l++)
                for (int k = 0; k < 27; k++) nxt[l][k] = acc[l][k] + acc[l ^ s][k];
            for (int l = 0; l < 64; l++)
                for (int k = 0; k < 27; k++) acc[l][k] = nxt[l][k];
        }
        for (int k = 0; k < 9; k++) {
            float* o = out + ((size_t)p * 9 + k) * 4;
            o[0] = acc[0][3 * k];
            o[1] = acc[0][3 * k + 1];
            o[2] = acc[0][3 * k + 2];
            o[3] = 0.0f;
        }
    }
}

}  // namespace jpt
