"""The refusals of the calls over the image itself -- the resolution and the partition, the progressive count, the read-backs, the
assembly (csrc/jpt_image.cpp) -- as far as a host-only context reaches them.  Return code and the whole jpt_last_error text against a
literal table, written down from the library as it was while these calls lived in csrc/jpt_capi.cpp.  CPU only."""
import ctypes as C

import pytest

from gdpathtracing_amd import capi, host

E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # JPT_E_* of include/jpt.h
SOME = (C.c_uint8 * 64)()                   # an output or a gathered buffer nothing ever touches: the calls refuse first

# row -> (how the call is made, the code, the text)
TABLE = {
    "set_params: width < 0": (lambda L, h: L.jpt_set_params(h, -1, 16, 1, capi.ACCUM_REF_LDR8, 0), E_INVALID, "bad resolution"),
    "set_params: height > 65536": (lambda L, h: L.jpt_set_params(h, 16, 65537, 1, capi.ACCUM_REF_LDR8, 0), E_INVALID, "bad resolution"),
    "set_params: max_bounces": (lambda L, h: L.jpt_set_params(h, 16, 16, 65, capi.ACCUM_REF_LDR8, 0), E_INVALID, "max_bounces must be in [0,64]"),
    "set_params: accum_mode": (lambda L, h: L.jpt_set_params(h, 16, 16, 1, 7, 0), E_INVALID, "unknown accum_mode"),
    "set_params: sampler_mode": (lambda L, h: L.jpt_set_params(h, 16, 16, 1, capi.ACCUM_REF_LDR8, 9), E_INVALID, "unknown sampler_mode"),
    "set_params: host-only": (lambda L, h: L.jpt_set_params(h, 16, 16, 1, capi.ACCUM_REF_LDR8, 0), E_DEVICE, "host-only context has no framebuffers"),
    "set_partition: world < 1": (lambda L, h: L.jpt_set_partition(h, 0, 0), E_INVALID, "need 0 <= rank < world"),
    "set_partition: rank < 0": (lambda L, h: L.jpt_set_partition(h, -1, 2), E_INVALID, "need 0 <= rank < world"),
    "set_partition: rank >= world": (lambda L, h: L.jpt_set_partition(h, 2, 2), E_INVALID, "need 0 <= rank < world"),
    "set_progressive_frame_count: 0": (lambda L, h: L.jpt_set_progressive_frame_count(h, 0), E_INVALID, "frame_count starts at 1 (progressive_rendering.cpp:20)"),
    "set_denoising_mode: unknown": (lambda L, h: L.jpt_set_denoising_mode(h, 3), E_INVALID, "unknown denoising mode"),
    "set_outputs: unknown bit": (lambda L, h: L.jpt_set_outputs(h, 2), E_INVALID, "jpt_set_outputs: unknown output bit"),
    "read_ldr_rgba8: null": (lambda L, h: L.jpt_read_ldr_rgba8(h, None), E_INVALID, "null output"),
    "read_ldr_rgba8: no params": (lambda L, h: L.jpt_read_ldr_rgba8(h, SOME), E_STATE, "jpt_set_params not called"),
    "read_accum_f32: null": (lambda L, h: L.jpt_read_accum_f32(h, None), E_INVALID, "null output"),
    "read_accum_f32: no params": (lambda L, h: L.jpt_read_accum_f32(h, SOME), E_STATE, "jpt_set_params not called"),
    "read_depth_f32: null": (lambda L, h: L.jpt_read_depth_f32(h, None), E_INVALID, "null output"),
    "read_depth_f32: no params": (lambda L, h: L.jpt_read_depth_f32(h, SOME), E_STATE, "jpt_set_params not called"),
    "readback_ldr_begin: host-only": (lambda L, h: L.jpt_readback_ldr_begin(h), E_DEVICE, "host-only context"),
    "readback_ldr_end: null": (lambda L, h: L.jpt_readback_ldr_end(h, None), E_INVALID, "null output"),
    "readback_ldr_end: nothing in flight": (lambda L, h: L.jpt_readback_ldr_end(h, SOME), E_STATE, "no read-back in flight (call jpt_readback_ldr_begin)"),
    "assemble_from_ranks: null": (lambda L, h: L.jpt_assemble_from_ranks(h, None, 1), E_INVALID, "null gathered buffer"),
    "assemble_from_ranks: host-only": (lambda L, h: L.jpt_assemble_from_ranks(h, SOME, 1), E_DEVICE, "host-only context"),
    "assemble_ldr_from_ranks: null": (lambda L, h: L.jpt_assemble_ldr_from_ranks(h, None, 1), E_INVALID, "null gathered buffer"),
    "assemble_ldr_from_ranks: host-only": (lambda L, h: L.jpt_assemble_ldr_from_ranks(h, SOME, 1), E_DEVICE, "host-only context"),
}
# the calls of the table on no context at all: the code alone (jpt_last_error(NULL) is jpt_create's)
NO_CONTEXT = {
    "set_params": lambda L: L.jpt_set_params(None, 16, 16, 1, capi.ACCUM_REF_LDR8, 0),
    "set_partition": lambda L: L.jpt_set_partition(None, 0, 1),
    "accum_reset": lambda L: L.jpt_accum_reset(None),
    "set_progressive_frame_count": lambda L: L.jpt_set_progressive_frame_count(None, 1),
    "set_denoising_mode": lambda L: L.jpt_set_denoising_mode(None, capi.DENOISE_PROGRESSIVE),
    "set_outputs": lambda L: L.jpt_set_outputs(None, 0),
    "read_ldr_rgba8": lambda L: L.jpt_read_ldr_rgba8(None, SOME),
    "read_accum_f32": lambda L: L.jpt_read_accum_f32(None, SOME),
    "read_depth_f32": lambda L: L.jpt_read_depth_f32(None, SOME),
    "readback_ldr_begin": lambda L: L.jpt_readback_ldr_begin(None),
    "readback_ldr_end": lambda L: L.jpt_readback_ldr_end(None, SOME),
    "assemble_from_ranks": lambda L: L.jpt_assemble_from_ranks(None, SOME, 1),
    "assemble_ldr_from_ranks": lambda L: L.jpt_assemble_ldr_from_ranks(None, SOME, 1),
}


@pytest.fixture()
def ctx():
    c = host.Context(-1)
    yield c
    c.close()


def refusal(L, h, call):
    L.jpt_set_kernel_timing(h, 0)   # (a call that succeeds and leaves the error text alone: the text below is this call's)
    L.jpt_set_debug_steps(h, 0)
    rc = call(L, h)
    return rc, L.jpt_last_error(h).decode()


@pytest.mark.parametrize("row", list(TABLE))
def test_each_refusal(ctx, row):
    L = capi.lib()
    call, code, text = TABLE[row]
    assert refusal(L, ctx.h, call) == (code, text)


def test_the_order_of_jpt_set_params_refusals(ctx):
    """Every argument wrong at once names the resolution; without it the bounces, then the accumulation, then the sampler, then the device."""
    L = capi.lib()
    args = [-1, 16, 65, 7, 9]
    good = [16, 16, 1, capi.ACCUM_REF_LDR8, 0]
    texts = ["bad resolution", "max_bounces must be in [0,64]", "unknown accum_mode", "unknown sampler_mode"]
    for k, (i, text) in enumerate(zip((0, 2, 3, 4), texts)):
        assert refusal(L, ctx.h, lambda L, h: L.jpt_set_params(h, *args)) == (E_INVALID, text), k
        args[i] = good[i]
    assert refusal(L, ctx.h, lambda L, h: L.jpt_set_params(h, *args)) == (E_DEVICE, "host-only context has no framebuffers")


@pytest.mark.parametrize("name", sorted(NO_CONTEXT))
def test_no_context_is_invalid(hiplib, name):
    assert NO_CONTEXT[name](capi.lib()) == E_INVALID


def test_a_partition_is_accepted_on_a_host_only_context(ctx):
    """jpt_set_partition keeps the rank and the world and makes no framebuffers: the calls that need the whole image see the partition
    (tests/test_post_refusals_host.py), jpt_local_rows stays 0, and a refused partition leaves the accepted one in place."""
    L = capi.lib()
    assert L.jpt_set_partition(ctx.h, 1, 2) == capi.OK
    assert L.jpt_local_rows(ctx.h) == 0
    assert refusal(L, ctx.h, lambda L, h: L.jpt_denoise(h)) == (E_STATE, "jpt_denoise needs the whole image on one context (world == 1)")
    assert L.jpt_set_partition(ctx.h, 3, 2) == E_INVALID
    assert refusal(L, ctx.h, lambda L, h: L.jpt_denoise(h)) == (E_STATE, "jpt_denoise needs the whole image on one context (world == 1)")
    assert L.jpt_set_partition(ctx.h, 0, 1) == capi.OK
    assert refusal(L, ctx.h, lambda L, h: L.jpt_denoise(h)) == (E_DEVICE, "host-only context: jpt_denoise runs on the device")


def test_the_setters_that_need_no_device_are_accepted(ctx):
    L = capi.lib()
    assert L.jpt_accum_reset(ctx.h) == capi.OK
    assert L.jpt_set_progressive_frame_count(ctx.h, 5) == capi.OK
    stats = capi.Stats()
    assert L.jpt_get_stats(ctx.h, C.byref(stats)) == capi.OK and stats.frames == 4
    for mode in (capi.DENOISE_TEMPORAL, capi.DENOISE_NONE, capi.DENOISE_PROGRESSIVE):
        assert L.jpt_set_denoising_mode(ctx.h, mode) == capi.OK
    assert L.jpt_get_stats(ctx.h, C.byref(stats)) == capi.OK and stats.frames == 0
    for outputs in (0, capi.OUTPUT_DEPTH):
        assert L.jpt_set_outputs(ctx.h, outputs) == capi.OK


@pytest.mark.parametrize("call", ["jpt_device_accum", "jpt_device_ldr"])
def test_the_device_pointers_of_no_context_and_of_a_fresh_one(ctx, call):
    L = capi.lib()
    fn = getattr(L, call)
    n = C.c_size_t(77)
    assert fn(None, C.byref(n)) is None and n.value == 77   # (no context: the count is left alone)
    assert fn(None, None) is None
    assert fn(ctx.h, C.byref(n)) is None and n.value == 0
    assert fn(ctx.h, None) is None


def test_the_local_rows_of_no_context_and_of_a_fresh_one(ctx):
    L = capi.lib()
    assert L.jpt_local_rows(None) == 0
    assert L.jpt_local_rows(ctx.h) == 0
