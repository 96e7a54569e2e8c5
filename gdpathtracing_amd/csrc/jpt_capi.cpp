// jpt_capi.cpp -- the C ABI of include/jpt.h over the HIP kernels and the host builder: the ABI version, the context's life cycle, error
// text and stream, the one-line setters and the statistics (the rest of the ABI: the other host files named in jpt_ctx.h).
#include "jpt_ctx.h"

#include <cstring>
#include <new>
#include <string>

#include "jpt_tuning.h"

namespace {

thread_local std::string g_create_error;

}  // namespace

extern "C" {

int jpt_abi_version(void) { return JPT_ABI_VERSION; }

int jpt_create(int device_id, jpt_ctx** out)
{
    if (!out) return JPT_E_INVALID;
    *out = nullptr;
    const bool host_only = device_id == JPT_DEVICE_HOST_ONLY;  // builder-only context: no device is touched
    if (!host_only) {
        // (Six renders in flight want six hardware queues for their streams; the runtime makes GPU_MAX_HW_QUEUES per priority level, four
        // by default, and reads the variable at the process's first HIP call.  That is the HOST's to export before it starts threads --
        // jpt.h "Process environment"; the library never writes the environment, it only measures what it got: six_queues_probe.)
        int n = 0;
        const hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) {
            g_create_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
            return JPT_E_DEVICE;
        }
        if (device_id < 0 || device_id >= n) {
            g_create_error = "device id out of range";
            return JPT_E_INVALID;
        }
    }
    jpt_ctx* c = new (std::nothrow) jpt_ctx();
    if (!c) return JPT_E_DEVICE;
    c->device = host_only ? -1 : device_id;
    std::memset(&c->stats, 0, sizeof c->stats);
    std::memset(&c->camera, 0, sizeof c->camera);
    if (!host_only) {
        hipError_t e;
        if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = c->pipe.create_events()) != hipSuccess) {
            g_create_error = std::string("HIP init: ") + hipGetErrorString(e);
            delete c;
            return JPT_E_DEVICE;
        }
        c->stream = c->own_stream;
        (void)tuning();  // environment switches are read here, once per process
    }
    *out = c;
    return JPT_OK;
}

void jpt_destroy(jpt_ctx* c)
{
    if (!c) return;
    if (c->device < 0) {
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    c->image.destroy();
    c->primary.destroy();
    c->enc.destroy();
    c->upd.destroy_stream();
    c->pipe.destroy();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* jpt_last_error(const jpt_ctx* c) { return c ? c->error.c_str() : g_create_error.c_str(); }

int jpt_set_stream(jpt_ctx* c, void* hip_stream)
{
    if (!c || c->device < 0) return JPT_E_INVALID;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (next != c->stream) {
        // everything this context has queued is ordered by the old stream (uploads, accumulation kernels, the
        // events its helper streams wait on): drain it before work starts appearing on another one
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->pipe.workspaces_touched();
        c->stream = next;
    }
    return JPT_OK;
}

int jpt_get_stream(jpt_ctx* c, void** hip_stream)
{
    if (!c || !hip_stream) return JPT_E_INVALID;
    if (c->device < 0) return fail(c, JPT_E_DEVICE, "host-only context has no stream");
    *hip_stream = (void*)c->stream;
    return JPT_OK;
}

int jpt_set_camera(jpt_ctx* c, const void* camera160)
{
    if (!c || !camera160) return fail(c, JPT_E_INVALID, "null camera");
    std::memcpy(&c->camera, camera160, sizeof(RefCamera));
    c->camera_set = true;
    return JPT_OK;
}

int jpt_set_kernel(jpt_ctx* c, int32_t variant)
{
    if (!c) return JPT_E_INVALID;
    if (variant != JPT_KERNEL_WAVEFRONT && variant != JPT_KERNEL_REFERENCE_LAYOUT) return fail(c, JPT_E_INVALID, "unknown kernel variant");
    c->kernel_variant = variant;
    return JPT_OK;
}

int jpt_set_debug_steps(jpt_ctx* c, int32_t enable)
{
    if (!c) return JPT_E_INVALID;
    c->debug_steps = enable != 0;
    return JPT_OK;
}

int jpt_get_stats(jpt_ctx* c, jpt_stats* out)
{
    if (!c || !out) return JPT_E_INVALID;
    *out = c->stats;
    return JPT_OK;
}

}  // extern "C"
