// jpt_image.cpp -- the image itself (ImageState, jpt_ctx.h): the partition and the framebuffers of its rows, the progressive count and
// what starts it over, the image assembled from every rank's piece, and the read-backs of all of them (include/jpt.h).
#include "jpt_ctx.h"

#include <algorithm>
#include <cstring>

int32_t jpt::rows_of_rank(int32_t height, int32_t rank, int32_t world)
{
    const int32_t n_strips = (height + kStripRows - 1) / kStripRows;
    int32_t rows = 0;
    for (int32_t s = rank; s < n_strips; s += world) {
        const int32_t y0 = s * kStripRows;
        rows += (y0 + kStripRows <= height) ? kStripRows : (height - y0);
    }
    return rows;
}

int32_t jpt::max_rows_of_any_rank(int32_t height, int32_t world)
{
    int32_t m = 0;
    for (int32_t r = 0; r < world; r++) m = std::max(m, rows_of_rank(height, r, world));
    return m;
}

// local strip-major rows -> full image rows, on the host
void jpt::scatter_rows(const char* local, char* out, int32_t width, int32_t height, int32_t rank, int32_t world, size_t px_bytes)
{
    const int32_t n_strips = (height + kStripRows - 1) / kStripRows;
    int32_t ly = 0;
    for (int32_t s = rank; s < n_strips; s += world) {
        for (int32_t r = 0; r < kStripRows; r++) {
            const int32_t y = s * kStripRows + r;
            if (y >= height) break;
            std::memcpy(out + (size_t)y * width * px_bytes, local + (size_t)ly * width * px_bytes, (size_t)width * px_bytes);
            ly++;
        }
    }
}

// (the table: jpt_ctx.h)
void jpt::restart_sum(jpt_ctx* c, SumRestart how, uint32_t count)
{
    ImageState& im = c->image;
    im.assembled = im.assembled_ldr = false;
    if (how == kSumRendered) return;
    c->frame_count = count;  // frame_count == 1 on the next frame overwrites the sum (progressive_rendering.glsl:34)
    im.accum_restarts++;
    if (how != kSumFramebuffers) c->stats.frames = count;
    // temporal mode: history images start from zero again, and jpt_read_accum_f32 has nothing to show until a pass has run
    if (how == kSumReset) c->reproj.restart();
    if (how == kSumFramebuffers) c->post.framebuffers_remade(false);
}

// The blocking read-backs' pinned staging buffer grows to the largest read-back ever made (133 MB after one jpt_read_accum_f32 of a
// 3840 x 2160 image) and would otherwise be held until jpt_destroy: given back whenever the framebuffers are re-made (another
// resolution or partition) and by jpt_set_memory_policy; the next read-back allocates what it needs.
void jpt::release_read_staging(jpt_ctx* c) { c->image.h_read_pinned.release(); }

// Blocking read-backs (jpt_read_ldr_rgba8 / accum_f32 / depth_f32): device -> the context's pinned read buffer -> the caller's
// memory.  A device-to-host copy straight into pageable memory runs at ~3 GB/s (8 MB of display image: 2.7 ms; 33 MB of float4
// sums: 11 ms); through pinned memory the copy runs at the link's rate and the host copy at memory speed.  (A buffer of its
// own: the split read-back's staging buffer may hold an image in flight.)
int jpt::staged_read(jpt_ctx* c, const void* src, size_t bytes)
{
    HIP_TRY(c, c->image.h_read_pinned.reserve(bytes));
    if (bytes) {
        HIP_TRY(c, hipMemcpyAsync(c->image.h_read_pinned.p, src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return JPT_OK;
}

int jpt::read_out(jpt_ctx* c, const void* src, size_t bytes, void* out)
{
    const int rc = staged_read(c, src, bytes);
    if (rc == JPT_OK && bytes) std::memcpy(out, c->image.h_read_pinned.p, bytes);
    return rc;
}

int jpt::read_rows_out(jpt_ctx* c, const void* src, size_t elem, int comps, bool whole, void* out)
{
    const ImageState& im = c->image;
    const size_t px_bytes = elem * (size_t)comps, full = (size_t)c->width * c->height * px_bytes;
    if (whole || c->world == 1) return read_out(c, src, whole ? full : (size_t)c->local_rows * c->width * px_bytes, out);
    const int rc = staged_read(c, src, (size_t)c->local_rows * c->width * px_bytes);
    if (rc != JPT_OK) return rc;
    std::memset(out, 0, full);
    scatter_rows(im.h_read_pinned.as<const char>(), static_cast<char*>(out), c->width, c->height, c->rank, c->world, px_bytes);
    return JPT_OK;
}

namespace {

int alloc_framebuffers(jpt_ctx* c)
{
    ImageState& im = c->image;
    // every rank allocates the same (maximum) size so a gather sees equal-sized pieces
    const int32_t piece_rows = max_rows_of_any_rank(c->height, c->world);
    const size_t npx = (size_t)piece_rows * c->width;
    if (npx != im.d_accum.n) release_read_staging(c);
    c->local_rows = rows_of_rank(c->height, c->rank, c->world);
    im.piece_rows = piece_rows;
    im.piece_px = npx;
    HIP_TRY(c, im.d_accum.resize(npx));
    HIP_TRY(c, im.d_ldr.resize(npx));
    HIP_TRY(c, im.d_depth.resize(npx));
    HIP_TRY(c, c->d_counters.resize(1));
    if (npx) {
        HIP_TRY(c, hipMemsetAsync(im.d_accum.p, 0, npx * sizeof(float4), c->stream));
        HIP_TRY(c, hipMemsetAsync(im.d_ldr.p, 0, npx * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(im.d_depth.p, 0, npx * sizeof(float), c->stream));
    }
    restart_sum(c, kSumFramebuffers);
    return JPT_OK;
}

// The pinned staging buffer of the display image's split read-backs holds one full image, whatever the read-back in flight copies:
// jpt_readback_ldr_end copies a whole image out of it unless the context is a partition when it is called
int ensure_ldr_pinned(jpt_ctx* c)
{
    HIP_TRY(c, c->image.ldr_read.buf.reserve((size_t)c->width * c->height * sizeof(uint32_t)));
    return JPT_OK;
}

int read_common(jpt_ctx* c, void* out)
{
    if (!c || !out) return fail(c, JPT_E_INVALID, "null output");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return JPT_OK;
}

}  // namespace

extern "C" {

int jpt_set_params(jpt_ctx* c, int32_t width, int32_t height, int32_t max_bounces, int32_t accum_mode, int32_t sampler_mode)
{
    if (!c) return JPT_E_INVALID;
    if (width < 0 || height < 0 || width > 65536 || height > 65536) return fail(c, JPT_E_INVALID, "bad resolution");
    if (max_bounces < 0 || max_bounces > kMaxBounces) return fail(c, JPT_E_INVALID, "max_bounces must be in [0,64]");
    if (accum_mode != JPT_ACCUM_REF_LDR8 && accum_mode != JPT_ACCUM_HDR_F32) return fail(c, JPT_E_INVALID, "unknown accum_mode");
    if (sampler_mode < JPT_SAMPLER_NEAREST_CLAMP || sampler_mode > JPT_SAMPLER_LINEAR_REPEAT) return fail(c, JPT_E_INVALID, "unknown sampler_mode");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no framebuffers");
    HIP_TRY(c, hipSetDevice(c->device));
    if (width != c->width || height != c->height) {
        // the post stages' images are of the old size: given back once the work that uses them has run
        if (c->post.sized_buffers()) HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->post.framebuffers_remade(true);
        c->primary.sh_valid = c->primary.refl_valid = false;   // (jpt_probe_project's coefficients and jpt_reflection_prefilter's chain likewise)
        // the temporal history is of the old size too (a new TemporalReprojection object): zeros at the next pass, and nothing to
        // read until then -- the pixel count alone does not tell (32 x 32 -> 16 x 64), and hist_written is sized by the old one
        c->reproj.restart();
    }
    c->width = width;
    c->height = height;
    c->max_bounces = max_bounces;
    c->accum_mode = accum_mode;
    c->sampler_mode = sampler_mode;
    c->ds.sampler_mode = sampler_mode;
    c->params_set = true;
    c->image.depth_valid = false;
    return alloc_framebuffers(c);
}

int jpt_set_partition(jpt_ctx* c, int32_t rank, int32_t world)
{
    if (!c) return JPT_E_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, JPT_E_INVALID, "need 0 <= rank < world");
    c->rank = rank;
    c->world = world;
    if (c->params_set && c->device >= 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        return alloc_framebuffers(c);
    }
    return JPT_OK;
}

int jpt_accum_reset(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    restart_sum(c, kSumReset);
    return JPT_OK;
}

int jpt_set_progressive_frame_count(jpt_ctx* c, uint32_t next_frame_count)
{
    if (!c) return JPT_E_INVALID;
    if (next_frame_count == 0) return fail(c, JPT_E_INVALID, "frame_count starts at 1 (progressive_rendering.cpp:20)");
    restart_sum(c, kSumPositioned, next_frame_count - 1u);
    return JPT_OK;
}

int jpt_set_denoising_mode(jpt_ctx* c, int32_t mode)
{
    if (!c) return JPT_E_INVALID;
    if (mode != JPT_DENOISE_PROGRESSIVE && mode != JPT_DENOISE_TEMPORAL && mode != JPT_DENOISE_NONE)
        return fail(c, JPT_E_INVALID, "unknown denoising mode");
    // the modes do not share state: the progressive sum and the temporal history both start over
    if (mode != c->denoise) restart_sum(c, kSumReset);
    c->denoise = mode;
    return JPT_OK;
}

int jpt_set_outputs(jpt_ctx* c, uint32_t outputs)
{
    if (!c) return JPT_E_INVALID;
    if (outputs & ~(uint32_t)JPT_OUTPUT_DEPTH) return fail(c, JPT_E_INVALID, "jpt_set_outputs: unknown output bit");
    c->outputs = outputs;   // (takes effect with the next render; a depth image already written stays readable until then)
    return JPT_OK;
}

int jpt_read_ldr_rgba8(jpt_ctx* c, uint8_t* out)
{
    const int rc = read_common(c, out);
    if (rc) return rc;
    // What the reference does every frame (get_image_uniform_buffer, path_tracing_camera.cpp:228-229): through staged_read.
    const ImageSource src = c->image.display_now();
    return read_rows_out(c, src.p, sizeof(uint32_t), 1, src.whole, out);
}

int jpt_readback_ldr_begin(jpt_ctx* c)
{
    if (!c) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    ImageState& im = c->image;
    if (im.ldr_read.pending) return fail(c, JPT_E_STATE, "a read-back is already in flight (call jpt_readback_ldr_end)");
    HIP_TRY(c, hipSetDevice(c->device));
    const ImageSource src = im.display_now();
    im.readback_full = src.whole;
    const size_t px = src.whole ? (size_t)c->width * c->height : (size_t)c->local_rows * c->width;
    {
        const int rc = ensure_ldr_pinned(c);
        if (rc) return rc;
    }
    HIP_TRY(c, im.ldr_read.begin(src.p, px * sizeof(uint32_t), c->stream));
    return JPT_OK;
}

int jpt_readback_ldr_end(jpt_ctx* c, uint8_t* out)
{
    if (!c || !out) return fail(c, JPT_E_INVALID, "null output");
    ImageState& im = c->image;
    if (!im.ldr_read.pending) return fail(c, JPT_E_STATE, "no read-back in flight (call jpt_readback_ldr_begin)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, im.ldr_read.wait());
    const size_t full = (size_t)c->width * c->height;
    if (im.readback_full || c->world == 1) {
        std::memcpy(out, im.ldr_read.buf.p, full * 4);
    } else {
        std::memset(out, 0, full * 4);
        scatter_rows(im.ldr_read.buf.as<const char>(), reinterpret_cast<char*>(out), c->width, c->height, c->rank, c->world, sizeof(uint32_t));
    }
    return JPT_OK;
}

int jpt_read_accum_f32(jpt_ctx* c, float* out)
{
    const int rc = read_common(c, out);
    if (rc) return rc;
    if (c->denoise == JPT_DENOISE_TEMPORAL) {
        // the rgba32f image of this mode is the history image the last pass wrote
        if (!c->reproj.hist_written) return fail(c, JPT_E_STATE, "no temporal pass has run since the last reset");
        return read_out(c, c->reproj.hist_written, (size_t)c->width * c->height * sizeof(float4), out);
    }
    const ImageSource src = c->image.sum_now();
    return read_rows_out(c, src.p, sizeof(float), 4, src.whole, out);
}

int jpt_read_depth_f32(jpt_ctx* c, float* out)
{
    int rc = read_common(c, out);
    if (rc) return rc;
    if (!c->image.depth_valid)
        return fail(c, JPT_E_STATE, (c->outputs & JPT_OUTPUT_DEPTH) ? "no render has written the depth image yet"
                                                                     : "the depth image is switched off (jpt_set_outputs): no render writes it");
    return read_rows_out(c, c->image.d_depth.p, sizeof(float), 1, false, out);
}

void* jpt_device_accum(jpt_ctx* c, size_t* bytes_out)
{
    if (!c) return nullptr;
    if (bytes_out) *bytes_out = c->image.piece_px * sizeof(float4);
    return c->image.d_accum.p;
}

void* jpt_device_ldr(jpt_ctx* c, size_t* bytes_out)
{
    if (!c) return nullptr;
    if (bytes_out) *bytes_out = c->image.piece_px * sizeof(uint32_t);
    return c->image.d_ldr.p;
}

int32_t jpt_local_rows(jpt_ctx* c) { return c ? c->local_rows : 0; }

int jpt_assemble_from_ranks(jpt_ctx* c, const void* device_gathered, int32_t world)
{
    if (!c || !device_gathered) return fail(c, JPT_E_INVALID, "null gathered buffer");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    ImageState& im = c->image;
    if (world != c->world) return fail(c, JPT_E_INVALID, "world differs from jpt_set_partition");
    if (c->denoise != JPT_DENOISE_PROGRESSIVE)
        return fail(c, JPT_E_STATE, "assembling re-derives the progressive display image; the other denoising modes run on one context");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t full = (size_t)c->width * c->height;
    HIP_TRY(c, im.d_full_accum.resize(full));
    HIP_TRY(c, im.d_full_ldr.resize(full));
    launch_assemble(c->stream, (const float4*)device_gathered, im.d_accum.p, c->rank, world, c->width, c->height, im.piece_rows,
                    im.d_full_accum.p, im.d_full_ldr.p, c->frame_count);
    HIP_TRY(c, hipGetLastError());
    im.assembled = true;  // asynchronous on the context's stream; jpt_read_* / jpt_sync wait for it
    return JPT_OK;
}

int jpt_assemble_ldr_from_ranks(jpt_ctx* c, const void* device_gathered, int32_t world)
{
    if (!c || !device_gathered) return fail(c, JPT_E_INVALID, "null gathered buffer");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context");
    if (!c->params_set) return fail(c, JPT_E_STATE, "jpt_set_params not called");
    ImageState& im = c->image;
    if (world != c->world) return fail(c, JPT_E_INVALID, "world differs from jpt_set_partition");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, im.d_full_ldr.resize((size_t)c->width * c->height));
    launch_assemble_ldr(c->stream, (const uint32_t*)device_gathered, im.d_ldr.p, c->rank, world, c->width, c->height, im.piece_rows,
                        im.d_full_ldr.p);
    HIP_TRY(c, hipGetLastError());
    im.assembled_ldr = true;  // asynchronous on the context's stream; jpt_read_ldr_rgba8 / jpt_sync wait for it
    return JPT_OK;
}

}  // extern "C"
