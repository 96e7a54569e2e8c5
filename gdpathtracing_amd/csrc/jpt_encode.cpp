// jpt_encode.cpp -- jpt_encode and the read-backs of its buffer (include/jpt.h; the arithmetic: jpt_encode.h; the kernel:
// jpt_kernels_encode.hip).  The call picks one of the float4 images the context holds, refuses as that image's own read-back refuses
// when it is not there, and queues one kernel on the context's stream into a buffer no other call writes.
#include "jpt_ctx.h"

#include <cstring>
#include <string>

#include "jpt_encode.h"

namespace {

// What jpt_encode reads: where the texels are, how many, what divides them, and the size jpt_get_encoded_info reports
struct EncodeSource {
    const float4* src = nullptr;
    uint64_t n = 0;
    float divisor = 1.0f;
    bool alpha_one = false;
    int32_t width = 0, height = 0;
};

// The state checks of one source, each with the code and the words of the source's own read-back (jpt_display's for the mean)
int resolve_source(jpt_ctx* c, int32_t source, int32_t level, EncodeSource& s)
{
    const PrimaryState& p = c->primary;
    s.width = c->width;
    s.height = c->height;
    s.n = (uint64_t)c->width * (uint64_t)c->height;
    switch (source) {
    case JPT_ENCODE_SOURCE_MEAN: {
        int rc = reads_sum(c, "jpt_encode", ": the mean is of the progressive accumulation", nullptr);   // (the device: jpt_encode has asked)
        if (rc == JPT_OK) rc = sum_ready(c, "jpt_encode");
        if (rc != JPT_OK) return rc;
        s.src = c->image.d_accum.p;
        s.divisor = (float)c->frame_count;
        s.alpha_one = true;
        return JPT_OK;
    }
    case JPT_ENCODE_SOURCE_DENOISED:
        if (!c->post.dn_valid) return fail(c, JPT_E_STATE, "jpt_encode: no jpt_denoise at the current resolution yet");
        s.src = c->post.d_dn_ping.p;
        return JPT_OK;
    case JPT_ENCODE_SOURCE_DISPLAY:
        if (!c->post.disp_valid) return fail(c, JPT_E_STATE, "jpt_encode: no jpt_display at the current resolution yet");
        s.src = c->post.d_disp_f32.p;
        return JPT_OK;
    case JPT_ENCODE_SOURCE_LIGHTMAP:
        if (!c->post.lm_result) return fail(c, JPT_E_STATE, "jpt_encode: no jpt_bake_finish at the current size and bake images yet");
        s.src = c->post.lm_result;
        return JPT_OK;
    case JPT_ENCODE_SOURCE_REFLECTION: {
        if (!p.refl_valid) return fail(c, JPT_E_STATE, "jpt_encode: no jpt_reflection_prefilter of the current reflection probes and size yet");
        if (level != JPT_ENCODE_ALL_LEVELS && (level < 0 || level >= p.refl_made))
            return fail(c, JPT_E_INVALID, "jpt_encode: level must be JPT_ENCODE_ALL_LEVELS or in [0, " + std::to_string(p.refl_made) + ")");
        const uint32_t shift = (uint32_t)cube_log2(p.cube_face);
        if (level == JPT_ENCODE_ALL_LEVELS) {
            s.src = p.d_refl_out.p;
            s.n = refl_out_texels((uint32_t)p.cube_n, shift, (uint32_t)p.refl_made);
            s.width = s.height = p.cube_face;
        } else {
            const uint64_t face = (uint64_t)(p.cube_face >> level);
            s.src = p.d_refl_out.p + refl_out_offset((uint32_t)p.cube_n, shift, (uint32_t)level);
            s.n = (uint64_t)p.cube_n * 6u * face * face;
            s.width = s.height = (int32_t)face;
        }
        return JPT_OK;
    }
    default:   // JPT_ENCODE_SOURCE_PROBE_SH
        if (!p.sh_valid) return fail(c, JPT_E_STATE, "jpt_encode: no jpt_probe_project of the current probes and size yet");
        s.src = p.d_probe_sh.p;
        s.n = 9u * (uint64_t)p.probe_n;
        s.width = 9;
        s.height = p.probe_n;
        return JPT_OK;
    }
}

}  // namespace

extern "C" {

int jpt_encode(jpt_ctx* c, int32_t source, int32_t level, int32_t format)
{
    if (!c) return JPT_E_INVALID;
    if (source < JPT_ENCODE_SOURCE_MEAN || source > JPT_ENCODE_SOURCE_PROBE_SH) return fail(c, JPT_E_INVALID, "jpt_encode: source must be one of JPT_ENCODE_SOURCE_*");
    if (!encode_format_known(format)) return fail(c, JPT_E_INVALID, "jpt_encode: format must be JPT_ENCODE_RGBA16F, _RGB9E5 or _RGBE8");
    if (source == JPT_ENCODE_SOURCE_PROBE_SH && format != JPT_ENCODE_RGBA16F)
        return fail(c, JPT_E_INVALID, "jpt_encode: SH coefficients are signed: JPT_ENCODE_SOURCE_PROBE_SH takes JPT_ENCODE_RGBA16F only");
    if (source != JPT_ENCODE_SOURCE_REFLECTION && level != 0) return fail(c, JPT_E_INVALID, "jpt_encode: level must be 0 for every source but JPT_ENCODE_SOURCE_REFLECTION");
    if (level < JPT_ENCODE_ALL_LEVELS) return fail(c, JPT_E_INVALID, "jpt_encode: level must be JPT_ENCODE_ALL_LEVELS or >= 0");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_encode: host-only context: it runs on the device");
    EncodeSource s;
    const int rc = resolve_source(c, source, level, s);
    if (rc != JPT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)s.n * encode_texel_bytes(format);
    if (c->enc.d_encoded.n < bytes) {
        // (a split read-back in flight may still copy from the old buffer)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->enc.valid = false;
        HIP_TRY(c, c->enc.d_encoded.resize(bytes));
    }
    const bool timed = c->kernel_timing;
    if (timed)
        for (hipEvent_t& e : c->enc.ev)
            if (!e) HIP_TRY(c, hipEventCreate(&e));
    // On the context's stream, as jpt_display: behind the accumulation of every render queued so far and behind the post calls queued
    // before it (also behind the copy of a split read-back in flight, which was queued first); whatever is queued later runs after it.
    if (timed) HIP_TRY(c, hipEventRecord(c->enc.ev[0], c->stream));
    launch_encode(c->stream, format, s.src, s.n, s.divisor, s.alpha_one, c->enc.d_encoded.p);
    if (timed) HIP_TRY(c, hipEventRecord(c->enc.ev[1], c->stream));
    HIP_TRY(c, hipGetLastError());
    c->enc.timed = timed;
    c->enc.info.source = source;
    c->enc.info.format = format;
    c->enc.info.level = level;
    c->enc.info.width = s.width;
    c->enc.info.height = s.height;
    c->enc.info.n_texels = s.n;
    c->enc.info.bytes = bytes;
    c->enc.valid = true;
    return JPT_OK;
}

static int encoded_common(jpt_ctx* c, const char* call, bool have_out)
{
    if (!c) return JPT_E_INVALID;
    if (!have_out) return fail(c, JPT_E_INVALID, std::string(call) + ": null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, std::string(call) + ": host-only context: jpt_encode runs on the device");
    if (!c->enc.valid) return fail(c, JPT_E_STATE, std::string(call) + ": no jpt_encode yet");
    return JPT_OK;
}

int jpt_get_encoded_info(jpt_ctx* c, jpt_encoded_info* out)
{
    const int rc = encoded_common(c, "jpt_get_encoded_info", out != nullptr);
    if (rc) return rc;
    *out = c->enc.info;
    return JPT_OK;
}

int jpt_read_encoded(jpt_ctx* c, void* out, size_t capacity)
{
    int rc = encoded_common(c, "jpt_read_encoded", out != nullptr);
    if (rc) return rc;
    const size_t bytes = (size_t)c->enc.info.bytes;
    if (capacity < bytes) return fail(c, JPT_E_INVALID, "jpt_read_encoded: capacity is " + std::to_string(capacity) + " bytes and the encoded image has " + std::to_string(bytes));
    HIP_TRY(c, hipSetDevice(c->device));
    return read_out(c, c->enc.d_encoded.p, bytes, out);
}

int jpt_readback_encoded_begin(jpt_ctx* c)
{
    const int rc = encoded_common(c, "jpt_readback_encoded_begin", true);
    if (rc) return rc;
    if (c->enc.read.pending) return fail(c, JPT_E_STATE, "jpt_readback_encoded_begin: a read-back is already in flight (call jpt_readback_encoded_end)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->enc.read.begin(c->enc.d_encoded.p, (size_t)c->enc.info.bytes, c->stream));
    return JPT_OK;
}

int jpt_readback_encoded_end(jpt_ctx* c, void* out, size_t capacity)
{
    if (!c) return JPT_E_INVALID;
    if (!out) return fail(c, JPT_E_INVALID, "jpt_readback_encoded_end: null output");
    SplitReadback& rb = c->enc.read;
    if (!rb.pending) return fail(c, JPT_E_STATE, "jpt_readback_encoded_end: no read-back in flight (call jpt_readback_encoded_begin)");
    if (capacity < rb.bytes)   // (the read-back stays in flight: the call may be repeated with room)
        return fail(c, JPT_E_INVALID, "jpt_readback_encoded_end: capacity is " + std::to_string(capacity) + " bytes and the read-back in flight has " +
                                          std::to_string(rb.bytes));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, rb.wait());
    if (rb.bytes) std::memcpy(out, rb.buf.p, rb.bytes);
    return JPT_OK;
}

void* jpt_device_encoded(jpt_ctx* c, size_t* bytes_out)
{
    const bool have = c && c->device >= 0 && c->enc.valid;
    if (bytes_out) *bytes_out = have ? (size_t)c->enc.info.bytes : 0;
    return have ? c->enc.d_encoded.p : nullptr;
}

int jpt_get_encode_timing(jpt_ctx* c, float* ms)
{
    if (!c) return JPT_E_INVALID;
    if (!ms) return fail(c, JPT_E_INVALID, "jpt_get_encode_timing: null output");
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "jpt_get_encode_timing: host-only context: jpt_encode runs on the device");
    if (!c->enc.valid || !c->enc.timed) return fail(c, JPT_E_STATE, "jpt_get_encode_timing: the last jpt_encode did not run under jpt_set_kernel_timing");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->enc.ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->enc.ev[0], c->enc.ev[1]));
    return JPT_OK;
}

}  // extern "C"
