// jpt_query.cpp -- the ray queries over the device scene: jpt_query_rays, jpt_query_rays_device and jpt_query_pixels, over QueryState
// (jpt_ctx.h).  On the context's stream: behind the accumulation of every render queued so far and behind the device refits
// (queue_instance_refit makes the stream wait for each), and ahead of a later jpt_scene_update_mesh, whose drain event is recorded on this
// stream.  A later refit writes the copy of the instance level a query reads only after the event that retired it, recorded on this
// stream too.
#include "jpt_ctx.h"

#include <cstring>
#include <string>

namespace {

constexpr uint32_t kQueryChunk = 1u << 20;   // rays per trip through the staging buffers (host forms)

// the checks every form shares, in the order the header gives: arguments, then the device, then the state; `done`: n == 0
int query_checks(jpt_ctx* c, int32_t mode, const void* rays, uint32_t n, const void* hits, const void* occluded, const char* what, bool& done)
{
    done = false;
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_QUERY_CLOSEST && mode != JPT_QUERY_ANY) return fail(c, JPT_E_INVALID, std::string(what) + ": unknown mode");
    if (mode == JPT_QUERY_ANY && hits) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_ANY writes occluded_out only (hits_out must be NULL)");
    if (n == 0) {
        done = true;
        return JPT_OK;
    }
    if (!rays) return fail(c, JPT_E_INVALID, std::string(what) + ": null rays");
    if (mode == JPT_QUERY_CLOSEST && !hits) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_CLOSEST needs hits_out");
    if (mode == JPT_QUERY_ANY && !occluded) return fail(c, JPT_E_INVALID, std::string(what) + ": JPT_QUERY_ANY needs occluded_out");
    return JPT_OK;
}

int query_state(jpt_ctx* c, const char* what)
{
    if (c->device < 0) return fail(c, JPT_E_DEVICE, std::string("host-only context: ") + what + " runs on the device");
    if (!c->scene.device_ready) return fail(c, JPT_E_STATE, std::string(what) + ": no scene");
    HIP_TRY(c, hipSetDevice(c->device));
    return JPT_OK;
}

// One chunk of a host form: `m` rays (or, pixels: raster positions seen through that model) from `in` up, the walk, the results back into hits / occluded
// (either may be null).  Device layout of d_query: [rays 32 B][hits 64 B][bytes 1 B] per ray of a chunk, each part 16-byte aligned.
int query_chunk(jpt_ctx* c, bool any, const CamModelDev* pixels, const void* in, uint32_t m, jpt_ray_hit* hits, uint8_t* occluded)
{
    const size_t cap = c->query.d_query.n / 97;
    char* d_rays = c->query.d_query.p;
    char* d_hits = d_rays + cap * sizeof(jpt_ray);
    char* d_occ = d_hits + cap * sizeof(jpt_ray_hit);
    char* h = c->image.h_read_pinned.as<char>();
    hipStream_t s = c->stream;
    if (pixels) {   // 8 B per ray go up, into the hits' part; the rays are made from them in place on the device
        std::memcpy(h, in, (size_t)m * 2 * sizeof(float));
        HIP_TRY(c, hipMemcpyAsync(d_hits, h, (size_t)m * 2 * sizeof(float), hipMemcpyHostToDevice, s));
        launch_query_pixel_rays(s, c->camera, *pixels, c->width, c->height, d_hits, m, d_rays);
    } else {
        std::memcpy(h, in, (size_t)m * sizeof(jpt_ray));
        HIP_TRY(c, hipMemcpyAsync(d_rays, h, (size_t)m * sizeof(jpt_ray), hipMemcpyHostToDevice, s));
    }
    launch_query(s, c->ds, any, d_rays, m, any ? nullptr : d_hits, occluded ? d_occ : nullptr);
    HIP_TRY(c, hipGetLastError());
    char* h_occ = h + (size_t)m * sizeof(jpt_ray_hit);
    if (hits) HIP_TRY(c, hipMemcpyAsync(h, d_hits, (size_t)m * sizeof(jpt_ray_hit), hipMemcpyDeviceToHost, s));
    if (occluded) HIP_TRY(c, hipMemcpyAsync(h_occ, d_occ, m, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (hits) std::memcpy(hits, h, (size_t)m * sizeof(jpt_ray_hit));
    if (occluded) std::memcpy(occluded, h_occ, m);
    return JPT_OK;
}

int query_host(jpt_ctx* c, bool any, const CamModelDev* pixels, const void* in, uint32_t n, jpt_ray_hit* hits, uint8_t* occluded)
{
    const size_t cap = ((size_t)(n < kQueryChunk ? n : kQueryChunk) + 15) & ~(size_t)15;
    if (c->query.d_query.n < cap * 97) HIP_TRY(c, c->query.d_query.resize(cap * 97));
    HIP_TRY(c, c->image.h_read_pinned.reserve(cap * (sizeof(jpt_ray_hit) + 1)));
    const size_t in_stride = pixels ? 2 * sizeof(float) : sizeof(jpt_ray);
    for (size_t first = 0; first < n; first += kQueryChunk) {
        const uint32_t m = (uint32_t)(n - first < kQueryChunk ? n - first : kQueryChunk);
        const int rc = query_chunk(c, any, pixels, static_cast<const char*>(in) + first * in_stride, m, hits ? hits + first : nullptr,
                                   occluded ? occluded + first : nullptr);
        if (rc != JPT_OK) return rc;
    }
    return JPT_OK;
}

}  // namespace

extern "C" {

int jpt_query_rays(jpt_ctx* c, int32_t mode, const jpt_ray* rays, uint32_t n, jpt_ray_hit* hits_out, uint8_t* occluded_out)
{
    bool done;
    int rc = query_checks(c, mode, rays, n, hits_out, occluded_out, "jpt_query_rays", done);
    if (rc != JPT_OK || done) return rc;
    if ((rc = query_state(c, "jpt_query_rays")) != JPT_OK) return rc;
    return query_host(c, mode == JPT_QUERY_ANY, nullptr, rays, n, hits_out, occluded_out);
}

int jpt_query_rays_device(jpt_ctx* c, int32_t mode, const void* d_rays, uint32_t n, void* d_hits_out, void* d_occluded_out)
{
    bool done;
    int rc = query_checks(c, mode, d_rays, n, d_hits_out, d_occluded_out, "jpt_query_rays_device", done);
    if (rc != JPT_OK || done) return rc;
    const void* ptrs[3] = {d_rays, d_hits_out, d_occluded_out};
    for (const void* p : ptrs)
        if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) return fail(c, JPT_E_INVALID, "jpt_query_rays_device: the pointers must be 16-byte aligned");
    if ((rc = query_state(c, "jpt_query_rays_device")) != JPT_OK) return rc;
    for (const void* p : ptrs) {
        if (!p) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != c->device) {
            (void)hipGetLastError();
            return fail(c, JPT_E_INVALID, "jpt_query_rays_device: the pointers must be device memory of the context's device");
        }
    }
    launch_query(c->stream, c->ds, mode == JPT_QUERY_ANY, d_rays, n, d_hits_out, d_occluded_out);
    HIP_TRY(c, hipGetLastError());
    return JPT_OK;
}

int jpt_query_pixels(jpt_ctx* c, const float* xy, uint32_t n, jpt_ray_hit* hits_out)
{
    bool done;
    int rc = query_checks(c, JPT_QUERY_CLOSEST, xy, n, hits_out, nullptr, "jpt_query_pixels", done);
    if (rc != JPT_OK || done) return rc;
    if ((rc = query_state(c, "jpt_query_pixels")) != JPT_OK) return rc;
    if (!c->params_set || !c->camera_set) return fail(c, JPT_E_STATE, "jpt_query_pixels: jpt_set_params / jpt_set_camera not called");
    CamModelDev cm;   // (jpt_set_camera_model: picking follows the model)
    if ((rc = view_now(c, "jpt_query_pixels", "picking rays", cm)) != JPT_OK) return rc;
    return query_host(c, false, &cm, xy, n, hits_out, nullptr);
}

}  // extern "C"
