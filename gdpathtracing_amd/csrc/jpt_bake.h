// jpt_bake.h -- lightmap baking (jpt_set_bake_texels, jpt_bake_begin / jpt_bake_add_surface): the path of texel (x, y) starts on the
// surface point the texel covers and leaves in a cosine-distributed direction about the surface normal, with throughput 1.  The
// running mean of the accumulation is then E / pi, E the irradiance at the texel: the radiance a white Lambertian surface sends back,
// which is what a lightmap stores.  Nothing downstream of ray generation knows: the rays go into the queues as they are, like the
// lens's and the camera models'.
//
// Two device images of width * height float4 each say where the texels are: position4 = (world position, w) and normal4 = (world
// normal, w).  A texel is VALID when dot(n.xyz, n.xyz) > 0 (NaN fails); all zeros is the canonical invalid texel.  An invalid texel
// traces nothing: radiance 0, first-hit distance cam.far_.
//
// The arithmetic is pinned (DESIGN.md "Pinned semantics": a fixed sequence of binary32 operations, restated in numpy by
// tests/np_bake.py); host and device run these functions (the *_bake forms of the primary kernels, the audit kernel, the rasteriser
// of jpt_kernels_bake.hip and the jpt_debug_bake_* entry points).
#pragma once

#include "jpt_shade.h"

namespace jpt {

constexpr uint64_t kBakeMaxTexels = 1ull << 26;      // 2 GiB of images
constexpr uint32_t kBakeMaxTriangles = 1u << 24;     // per jpt_bake_add_surface (a winner is a triangle index; its float is exact)
constexpr uint32_t kBakeNoWinner = 0xffffffffu;

// The texel images of one render, passed by value to its bounce-0 launch: null pointers are a camera render (nothing is read then).
struct BakeDev {
    const float4* position = nullptr;
    const float4* normal = nullptr;
};

// One surface as the rasteriser reads it; every pointer addresses n_vertices / 3 * n_tris elements (device memory on the device)
struct BakeSurfaceDev {
    const float* vertices = nullptr;   // n_vertices * 3
    const float* normals = nullptr;    // n_vertices * 3
    const float* uv2 = nullptr;        // n_vertices * 2
    const int32_t* indices = nullptr;  // n_tris * 3, each in 0 .. n_vertices - 1 (checked by the host)
    uint32_t n_tris = 0;
    float transform[16] = {};          // the mat4 jpt_scene_add_instance makes of transform12 (transform12_to_mat16)
};

#if defined(__HIPCC__)

__host__ __device__ __forceinline__ bool bake_texel_valid(const float4 n) { return n.x * n.x + n.y * n.y + n.z * n.z > 0.0f; }

// The first ray of texel (px, py)'s path of frame `frame`, from the texel's position and normal (a valid texel's):
//   the seeds and the jitter draw of primary_ray, taken and discarded, so (sx, sy) leave as they do under a camera and every later
//   vertex draws what it draws today; (xi0, xi1) from one pcg2d round of a COPY (sx ^ 0x3c6ef372, sy ^ 0xa54ff53a); the shading
//   space of the normalised normal and the diffuse branch of sample_brdf (sample_hemisphere_psa), composed as sample_brdf's last
//   statement composes it and not renormalised; the origin offset of bounce_step.
__host__ __device__ __forceinline__ Ray bake_ray(const float4 p4, const float4 n4, int px, int py, uint32_t frame, uint32_t& sx, uint32_t& sy)
{
    prng_seed((uint32_t)px, (uint32_t)py, frame, sx, sy);
    float r0, r1;
    pcg2d(sx, sy, r0, r1);
    uint32_t hx = sx ^ 0x3c6ef372u, hy = sy ^ 0xa54ff53au;
    float xi0, xi1;
    pcg2d(hx, hy, xi0, xi1);
    const f3 nrm = normalize3(mk3(n4.x, n4.y, n4.z));
    // get_shading_space (brdfs.glsl:83-93), as sample_brdf builds it
    const float sign = nrm.z > 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + nrm.z);
    const float b = nrm.x * nrm.y * a;
    const f3 c0 = mk3(1.0f + sign * nrm.x * nrm.x * a, sign * b, -sign * nrm.x);
    const f3 c1 = mk3(b, sign + nrm.y * nrm.y * a, -nrm.y);
    const f3 c2 = nrm;
    float sp, cp;
    sincos_((2.0f * JPT_PI) * xi0, sp, cp);
    const float radius = __builtin_sqrtf(xi1);
    const float z = __builtin_sqrtf(1.0f - radius * radius);
    const f3 local = mk3(radius * cp, radius * sp, z);
    Ray ray;
    ray.o = mk3(p4.x, p4.y, p4.z) + nrm * 0.001f;
    ray.d = mk3(c0.x * local.x + c1.x * local.y + c2.x * local.z, c0.y * local.x + c1.y * local.y + c2.y * local.z,
                c0.z * local.x + c1.z * local.y + c2.z * local.z);
    ray.rD = rcp3(ray.d);
    return ray;
}

// ---- the UV2 rasteriser (jpt_bake_add_surface): coverage at texel centres, the lowest triangle index wins a texel ---------------

struct BakeTri2 {   // a triangle's UV2 corners in texels, and its signed doubled area
    float ax, ay, bx, by, cx, cy, area;
};

__host__ __device__ __forceinline__ float bake_edge(float ux, float uy, float vx, float vy, float px, float py)
{
    return (vx - ux) * (py - uy) - (vy - uy) * (px - ux);
}

__host__ __device__ __forceinline__ BakeTri2 bake_tri2(const BakeSurfaceDev& s, uint32_t t, int32_t width, int32_t height)
{
    const int32_t ia = s.indices[3 * (size_t)t], ib = s.indices[3 * (size_t)t + 1], ic = s.indices[3 * (size_t)t + 2];
    const float W = (float)width, H = (float)height;
    BakeTri2 q;
    q.ax = s.uv2[2 * (size_t)ia] * W;
    q.ay = s.uv2[2 * (size_t)ia + 1] * H;
    q.bx = s.uv2[2 * (size_t)ib] * W;
    q.by = s.uv2[2 * (size_t)ib + 1] * H;
    q.cx = s.uv2[2 * (size_t)ic] * W;
    q.cy = s.uv2[2 * (size_t)ic + 1] * H;
    q.area = (q.bx - q.ax) * (q.cy - q.ay) - (q.by - q.ay) * (q.cx - q.ax);
    return q;
}

// |area| > 0 (NaN fails): the triangle can cover a texel at all
__host__ __device__ __forceinline__ bool bake_tri_drawn(const BakeTri2& q) { return __builtin_fabsf(q.area) > 0.0f; }

// The edge functions of texel (x, y)'s centre, negated for the other winding; true when all three are >= 0: the texel is covered
__host__ __device__ __forceinline__ bool bake_cover(const BakeTri2& q, int32_t x, int32_t y, float& e_b, float& e_c)
{
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float ea = bake_edge(q.bx, q.by, q.cx, q.cy, px, py);
    float eb = bake_edge(q.cx, q.cy, q.ax, q.ay, px, py);
    float ec = bake_edge(q.ax, q.ay, q.bx, q.by, px, py);
    if (q.area < 0.0f) {
        ea = -ea;
        eb = -eb;
        ec = -ec;
    }
    e_b = eb;
    e_c = ec;
    return ea >= 0.0f && eb >= 0.0f && ec >= 0.0f;
}

// The texels a triangle may claim: its corners' bounding box, one texel wider on every side, clipped to the image; the whole image
// when a corner is not finite.  The box is part of the rule, not only a bound on the walk: with exact arithmetic no texel centre
// outside it is covered, but the rounded edge functions of a sliver can all come out >= 0 far along its line -- host, device and
// numpy all leave such a texel alone.  False: nothing to visit.
__host__ __device__ __forceinline__ bool bake_tri_box(const BakeTri2& q, int32_t width, int32_t height, int32_t& x0, int32_t& y0, int32_t& x1, int32_t& y1)
{
    const float W = (float)width, H = (float)height;
    const float all[6] = {q.ax, q.ay, q.bx, q.by, q.cx, q.cy};
    bool finite = true;
    for (int k = 0; k < 6; k++) finite = finite && (all[k] - all[k] == 0.0f);
    x0 = y0 = 0;
    x1 = width - 1;
    y1 = height - 1;
    if (!finite) return true;
    float lx = q.ax < q.bx ? q.ax : q.bx, hx = q.ax > q.bx ? q.ax : q.bx;
    float ly = q.ay < q.by ? q.ay : q.by, hy = q.ay > q.by ? q.ay : q.by;
    lx = lx < q.cx ? lx : q.cx;
    hx = hx > q.cx ? hx : q.cx;
    ly = ly < q.cy ? ly : q.cy;
    hy = hy > q.cy ? hy : q.cy;
    lx = lx - 1.0f;
    ly = ly - 1.0f;
    hx = hx + 1.0f;
    hy = hy + 1.0f;
    // (float -> int conversions of values inside [0, W) and [0, H) only: they truncate)
    if (lx > 0.0f) x0 = lx < W ? (int32_t)lx : width;
    if (ly > 0.0f) y0 = ly < H ? (int32_t)ly : height;
    if (hx < W) x1 = hx > 0.0f ? (int32_t)hx : -1;
    if (hy < H) y1 = hy > 0.0f ? (int32_t)hy : -1;
    return x0 <= x1 && y0 <= y1;
}

// column-major 4x4 times (p, 1) / (d, 0): xform_point / xform_dir of jpt_device_math.h, for host and device
__host__ __device__ __forceinline__ f3 bake_xform_point(const float* m, f3 p)
{
    return f3{m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
              m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]};
}
__host__ __device__ __forceinline__ f3 bake_xform_dir(const float* m, f3 d)
{
    return f3{m[0] * d.x + m[4] * d.y + m[8] * d.z, m[1] * d.x + m[5] * d.y + m[9] * d.z, m[2] * d.x + m[6] * d.y + m[10] * d.z};
}

// The texel (x, y) that triangle t won: barycentric weights from the edge functions (u = e_B / |area|, v = e_C / |area|, w0 = 1 - u
// - v: the weights and order of get_shading_data), the interpolated position and normal through the transform.  A non-finite
// component makes the texel invalid (all zeros).
__host__ __device__ __forceinline__ void bake_resolve(const BakeSurfaceDev& s, uint32_t t, int32_t width, int32_t height, int32_t x, int32_t y, float4& p4,
                                                      float4& n4)
{
    const BakeTri2 q = bake_tri2(s, t, width, height);
    float eb, ec;
    (void)bake_cover(q, x, y, eb, ec);
    const float aa = __builtin_fabsf(q.area);
    const float u = eb / aa, v = ec / aa;
    const float w0 = 1.0f - u - v;
    const int32_t ia = s.indices[3 * (size_t)t], ib = s.indices[3 * (size_t)t + 1], ic = s.indices[3 * (size_t)t + 2];
    const float *va = s.vertices + 3 * (size_t)ia, *vb = s.vertices + 3 * (size_t)ib, *vc = s.vertices + 3 * (size_t)ic;
    const float *na = s.normals + 3 * (size_t)ia, *nb = s.normals + 3 * (size_t)ib, *nc = s.normals + 3 * (size_t)ic;
    const f3 lp = (mk3(va[0], va[1], va[2]) * w0 + mk3(vb[0], vb[1], vb[2]) * u) + mk3(vc[0], vc[1], vc[2]) * v;
    const f3 ln = (mk3(na[0], na[1], na[2]) * w0 + mk3(nb[0], nb[1], nb[2]) * u) + mk3(nc[0], nc[1], nc[2]) * v;
    const f3 p = bake_xform_point(s.transform, lp);
    const f3 n = normalize3(bake_xform_dir(s.transform, ln));
    const float all[6] = {p.x, p.y, p.z, n.x, n.y, n.z};
    bool finite = true;
    for (int k = 0; k < 6; k++) finite = finite && (all[k] - all[k] == 0.0f);
    p4 = finite ? make_float4(p.x, p.y, p.z, (float)t) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    n4 = finite ? make_float4(n.x, n.y, n.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

#endif  // __HIPCC__

}  // namespace jpt
