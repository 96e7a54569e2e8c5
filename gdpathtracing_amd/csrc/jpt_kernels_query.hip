// jpt_kernels_query.hip -- jpt_query_rays / jpt_query_pixels: the walk of guide_kernel and wf2_occlude_lt opened to rays the caller
// supplies.  No reference counterpart.  The hit rule and the encodings are pinned in include/jpt.h / DESIGN.md section 2; nothing
// here writes a buffer a render or a read-back reads.
#include "../../include/jpt.h"
#include "jpt_kernels.h"
#include "jpt_trace_core.h"

namespace jpt {

namespace {

constexpr int kQueryBlock = 64;
constexpr float kQueryMiss = 1e9f;   // the pipeline's miss sentinel (Traversal::begin)

__device__ __forceinline__ bool finite_(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// One lane per ray, one wave per block, the whole stack in LDS (wf2_occlude's arrangement: no scratch).  The ray is two 16-byte
// loads (origin | tmax, direction | reserved).  CLOSEST (ANY = false): the walk starts with hit.t = tmax and is stepped to its end
// -- the smallest accepted Moller-Trumbore t, no reach or tie logic, a hit when it ends with hit.t < tmax --, then the shading
// gather guide_kernel makes, and the jpt_ray_hit as four 16-byte stores.  ANY: wf2_occlude_lt's walk, stopped at the first accepted
// triangle with t < tmax; only the byte is written.
template <bool W4, bool ANY>
__global__ __launch_bounds__(kQueryBlock) void query_kernel(WideSceneDev sc, SceneShading sh, const float4* __restrict__ rays, uint32_t n,
                                                            float4* __restrict__ hits, uint8_t* __restrict__ occluded)
{
    constexpr int kDepth = kStackLds + kStackSpill;
    __shared__ int32_t stack[kDepth * kQueryBlock];
    const size_t i = (size_t)blockIdx.x * kQueryBlock + threadIdx.x;   // (n may lie within a block of 2^32)
    if (i >= n) return;
    const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
    const f3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r1.x, r1.y, r1.z);
    const bool bad = !(finite_(o.x) && finite_(o.y) && finite_(o.z) && finite_(d.x) && finite_(d.y) && finite_(d.z)) ||
                     (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
    const float tmax = (r0.w > 0.0f && r0.w < kQueryMiss) ? r0.w : kQueryMiss;   // NaN, <= 0, >= 1e9 (inf): the miss sentinel
    const typename Traversal<false, W4>::Stack st{&stack[threadIdx.x], nullptr, kQueryBlock, kDepth, 0};
    DevCounters cnt = {};
    Traversal<false, W4> tr;
    bool hit = false;
    if (!bad) {
        tr.begin(sc, o, d);
        tr.hit.t = tmax;
        if (ANY) {
            while (tr.hit.t >= tmax && tr.step(sc, st, cnt)) {
            }
        } else {
            while (tr.step(sc, st, cnt)) {
            }
        }
        hit = tr.hit.t < tmax;
    }
    if (occluded) occluded[i] = hit ? 1 : 0;
    if (ANY) return;
    // the miss encoding: t = -1, instance = -1, everything else 0 (a bad ray: the same with its flag)
    float4 q0 = make_float4(-1.0f, 0.0f, 0.0f, __int_as_float(-1)), q1 = make_float4(0.0f, 0.0f, __uint_as_float(bad ? (uint32_t)JPT_HIT_BAD_RAY : 0u), 0.0f);
    float4 q2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q3 = q2;
    if (hit) {
        Hit h;
        h.t = tr.hit.t;
        h.u = tr.hit.u;
        h.v = tr.hit.v;
        h.tri = tr.hit.tri;
        h.inst = (tr.hit.inst >> kInstBits) & kInstMask;   // the instance whose local ray found the triangle kept (guide_kernel)
        const RefInstance& b = sh.instances[h.inst];
        h.lo = xform_point(b.inverse_transform, o);
        h.ld = xform_dir(b.inverse_transform, d);
        const ShadeTriRegs tq = load_shade_tri(sh, h.tri);
        const Shading s = get_shading_data<3>(sh, h, tr.hit.front, tq);
        // the material index and the uv as get_shading_data forms them
        const uint32_t slot = __float_as_uint(tq.q3.w);
        const unsigned long long word = (unsigned long long)h.inst * 44ull + 41ull + (unsigned long long)slot;
        uint32_t mat_id = word < (unsigned long long)sh.n_instances * 44ull ? reinterpret_cast<const uint32_t*>(sh.instances)[word] : 0u;
        if (mat_id >= sh.n_materials) mat_id = 0;
        const float w0 = 1.0f - h.u - h.v;
        const float uvx = tq.q2.y * w0 + tq.q2.w * h.u + tq.q3.y * h.v;
        const float uvy = tq.q2.z * w0 + tq.q3.x * h.u + tq.q3.z * h.v;
        const uint32_t flags = (uint32_t)JPT_HIT_VALID | (tr.hit.front ? (uint32_t)JPT_HIT_FRONT : 0u);
        q0 = make_float4(h.t, h.u, h.v, __uint_as_float(h.inst));
        q1 = make_float4(__uint_as_float(h.tri), __uint_as_float(mat_id), __uint_as_float(flags), s.position.x);
        q2 = make_float4(s.position.y, s.position.z, s.normal.x, s.normal.y);
        q3 = make_float4(s.normal.z, uvx, uvy, 0.0f);
    }
    float4* out = hits + 4 * i;
    out[0] = q0;
    out[1] = q1;
    out[2] = q2;
    out[3] = q3;
}

// jpt_query_pixels: the jpt_ray of each raster position, tmax = the miss sentinel -- cam.position and raster_direction, the
// un-jittered pinhole ray of the guide pass.  A non-finite coordinate gives a non-finite direction: query_kernel flags the ray.
__global__ __launch_bounds__(256) void query_pixel_rays(RefCamera cam, int width, int height, const float2* __restrict__ xy, uint32_t n,
                                                        float4* __restrict__ rays)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 p = xy[i];
    float ww;
    f3 d = raster_direction(cam, width, height, p.x, p.y, ww);
    if (!(finite_(p.x) && finite_(p.y))) d = mk3(__uint_as_float(0x7fc00000u), 0.0f, 0.0f);
    rays[2 * i] = make_float4(cam.position.x, cam.position.y, cam.position.z, kQueryMiss);
    rays[2 * i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

// ... and under a camera model other than the pinhole (jpt_set_camera_model): the model's ray of the exact position
// (camera_raster_ray), so picking hits what the picture shows
__global__ __launch_bounds__(256) void query_pixel_rays_cam(RefCamera cam, CamModelDev cm, int width, int height, const float2* __restrict__ xy,
                                                            uint32_t n, float4* __restrict__ rays)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 p = xy[i];
    Ray ray = camera_raster_ray(cam, cm, width, height, p.x, p.y);
    if (!(finite_(p.x) && finite_(p.y))) ray.d = mk3(__uint_as_float(0x7fc00000u), 0.0f, 0.0f);
    rays[2 * i] = make_float4(ray.o.x, ray.o.y, ray.o.z, kQueryMiss);
    rays[2 * i + 1] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f);
}

}  // namespace

void launch_query(hipStream_t stream, const DeviceScene& ds, bool any, const void* rays, uint32_t n, void* hits, void* occluded)
{
    if (n == 0) return;
    const bool w4 = ds.use4;
    WideSceneDev sc;   // the arrays the wavefront kernels walk, with the current copy of the instance level (launch_guides)
    sc.blas_nodes = ds.blas_nodes;
    sc.tlas_nodes = ds.tlas_nodes;
    sc.nodesq = ds.nodesq;
    sc.tris = ds.wide_tris;
    sc.instances = w4 ? ds.wide_instances4 : ds.wide_instances;
    sc.tlas_root = w4 ? ds.tlas_root4 : ds.tlas_root;
    sc.n_instances = ds.n_instances;
    sc.reach_tri = ds.reach_tri;
    sc.reach_inst = ds.reach_inst;
    const SceneShading sh = ds.shading();
    const dim3 grid(n / kQueryBlock + (n % kQueryBlock != 0 ? 1u : 0u)), block(kQueryBlock);
    with_consts<2, 2>([&](auto W, auto A) {
        hipLaunchKernelGGL((query_kernel<W, A>), grid, block, 0, stream, sc, sh, static_cast<const float4*>(rays), n,
                           static_cast<float4*>(hits), static_cast<uint8_t*>(occluded));
    }, w4 ? 1 : 0, any ? 1 : 0);
}

void launch_query_pixel_rays(hipStream_t stream, const RefCamera& cam, const CamModelDev& cm, int width, int height, const void* xy, uint32_t n,
                             void* rays)
{
    if (n == 0) return;
    const dim3 grid(n / 256u + (n % 256u != 0 ? 1u : 0u)), block(256);
    if (cm.model != kCamPinhole)
        hipLaunchKernelGGL(query_pixel_rays_cam, grid, block, 0, stream, cam, cm, width, height, static_cast<const float2*>(xy), n, static_cast<float4*>(rays));
    else
        hipLaunchKernelGGL(query_pixel_rays, grid, block, 0, stream, cam, width, height, static_cast<const float2*>(xy), n, static_cast<float4*>(rays));
}

}  // namespace jpt
