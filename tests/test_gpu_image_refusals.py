"""The refusals of the image's read-backs and assembly that need a device (csrc/jpt_image.cpp): return code and the whole jpt_last_error
text against literal rows, written down from the library as it was while these calls lived in csrc/jpt_capi.cpp.  Cornell, BUILD_SAH,
one bounce, 16 x 16."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4   # JPT_E_* of include/jpt.h
W = H = 16

IN_FLIGHT = "a read-back is already in flight (call jpt_readback_ldr_end)"
NOT_IN_FLIGHT = "no read-back in flight (call jpt_readback_ldr_begin)"
NO_DEPTH_YET = "no render has written the depth image yet"
DEPTH_OFF = "the depth image is switched off (jpt_set_outputs): no render writes it"
NO_TEMPORAL_PASS = "no temporal pass has run since the last reset"
OTHER_WORLD = "world differs from jpt_set_partition"
NOT_PROGRESSIVE = "assembling re-derives the progressive display image; the other denoising modes run on one context"


@pytest.fixture()
def ctx(hiplib):
    sc = scenes.cornell_scene()
    c = host.Context(0)
    c.build_scene(sc, capi.BUILD_SAH)
    c.set_params(W, H, 1, capi.ACCUM_REF_LDR8)
    c.set_camera(scenes.camera_block(sc.camera, W, H))
    yield c
    c.close()


def refusal(c, call):
    L = capi.lib()
    L.jpt_set_kernel_timing(c.h, 0)   # (a call that succeeds and leaves the error text alone: the text below is this call's)
    rc = call(L, c.h)
    return rc, L.jpt_last_error(c.h).decode()


def test_one_split_read_back_in_flight(ctx):
    ctx.render(1, 1)
    want = ctx.read_ldr()
    ctx.readback_ldr_begin()
    assert refusal(ctx, lambda L, h: L.jpt_readback_ldr_begin(h)) == (E_STATE, IN_FLIGHT)
    out = np.zeros((H, W, 4), np.uint8)
    assert capi.lib().jpt_readback_ldr_end(ctx.h, out.ctypes.data) == capi.OK
    assert want.any() and np.array_equal(out, want)
    assert refusal(ctx, lambda L, h: L.jpt_readback_ldr_end(h, out.ctypes.data)) == (E_STATE, NOT_IN_FLIGHT)
    ctx.readback_ldr_begin()   # and the next one is accepted again
    assert np.array_equal(ctx.readback_ldr_end(), want)


def test_the_depth_image_before_a_render_and_switched_off(ctx):
    out = np.zeros((H, W), np.float32)
    read = lambda L, h: L.jpt_read_depth_f32(h, out.ctypes.data)
    assert refusal(ctx, read) == (E_STATE, NO_DEPTH_YET)
    ctx.set_outputs(depth=False)
    assert refusal(ctx, read) == (E_STATE, DEPTH_OFF)
    ctx.render(1, 1)
    assert refusal(ctx, read) == (E_STATE, DEPTH_OFF)
    ctx.set_outputs(depth=True)   # (takes effect with the next render)
    assert refusal(ctx, read) == (E_STATE, NO_DEPTH_YET)
    ctx.render(1, 2)
    assert capi.lib().jpt_read_depth_f32(ctx.h, out.ctypes.data) == capi.OK and out.any()


def test_the_sum_in_temporal_mode_before_a_pass(ctx):
    out = np.zeros((H, W, 4), np.float32)
    ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
    assert refusal(ctx, lambda L, h: L.jpt_read_accum_f32(h, out.ctypes.data)) == (E_STATE, NO_TEMPORAL_PASS)


@pytest.mark.parametrize("call", ["jpt_assemble_from_ranks", "jpt_assemble_ldr_from_ranks"])
@pytest.mark.parametrize("rank,world,asked", [(0, 1, 2), (1, 2, 1), (0, 2, 3)])
def test_assembling_with_another_world_than_the_partition_s(ctx, call, rank, world, asked):
    ctx.set_partition(rank, world)
    piece, _ = ctx.device_accum()   # (some device memory: the call refuses before it reads it)
    assert refusal(ctx, lambda L, h: getattr(L, call)(h, piece, asked)) == (E_INVALID, OTHER_WORLD)


@pytest.mark.parametrize("mode", [capi.DENOISE_TEMPORAL, capi.DENOISE_NONE])
def test_assembling_the_sum_outside_progressive_mode(ctx, mode):
    ctx.set_denoising_mode(mode)
    piece, _ = ctx.device_accum()
    assert refusal(ctx, lambda L, h: L.jpt_assemble_from_ranks(h, piece, 1)) == (E_STATE, NOT_PROGRESSIVE)
    # the world is asked first
    assert refusal(ctx, lambda L, h: L.jpt_assemble_from_ranks(h, piece, 2)) == (E_INVALID, OTHER_WORLD)
