"""What another image size (jpt_set_params) does to the post stages' results -- jpt_denoise, jpt_display, jpt_meter, jpt_noise_estimate and the
variance plane on a camera render; jpt_bake_finish, jpt_bake_finish_directional and the directional planes on a bake render: every read-back
refuses with its own words until the stage has run at the new size, and then gives bit for bit what a context that only ever saw that size
gives.  16 x 8 -> 8 x 8 and 8 x 4 -> 4 x 4: the smallest sizes with more than one 8 x 8 noise tile column before and another pixel count after."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

from test_bake_host import atlas
from test_gpu_bake import bake_ctx
from test_gpu_camera import make_ctx

pytestmark = pytest.mark.gpu

F = np.float32
E_STATE = -4   # JPT_E_STATE


def camera_ctx(sc, w, h):
    ctx = make_ctx(sc, None, w, h)
    try:
        ctx.set_variance(True)
    except Exception:
        ctx.close()
        raise
    return ctx


def run_stages(ctx, sc, w, h):
    """2 frames at the context's size, then the four stages"""
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    ctx.render(2, 1)
    ctx.denoise()
    ctx.display()
    ctx.meter()
    ctx.noise_estimate()


def read_all(ctx):
    """name -> bytes of every read-back of the four stages and of the plane"""
    L = ctx._lib
    meter, noise = capi.MeterResult(), capi.NoiseResult()
    mhist, nhist = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    ctx._ck(L.jpt_read_meter(ctx.h, host.C.byref(meter), host._ptr(mhist)), "jpt_read_meter")
    ctx._ck(L.jpt_read_noise(ctx.h, host.C.byref(noise), host._ptr(nhist)), "jpt_read_noise")
    return {"denoised": ctx.read_denoised().tobytes(), "denoised_ldr": ctx.read_denoised_ldr().tobytes(), "display": ctx.read_display().tobytes(),
            "display_ldr": ctx.read_display_ldr().tobytes(), "meter": bytes(meter) + mhist.tobytes(), "noise": bytes(noise) + nhist.tobytes(),
            "noise_tiles": ctx.read_noise_tiles().tobytes(), "variance": ctx.read_variance().tobytes()}


def refused(ctx, rc, text):
    assert (rc, ctx._lib.jpt_last_error(ctx.h).decode()) == (E_STATE, text)


def test_camera_stages_across_a_change_of_size(hiplib):
    L = hiplib
    sc = scenes.cornell_scene()
    fresh = camera_ctx(sc, 8, 8)
    try:
        run_stages(fresh, sc, 8, 8)
        want = read_all(fresh)
    finally:
        fresh.close()
    ctx = camera_ctx(sc, 16, 8)
    try:
        run_stages(ctx, sc, 16, 8)
        before = read_all(ctx)
        assert len(before["noise_tiles"]) == 2 * 4 and before["variance"] != bytes(16 * 8 * 16)
        # the same size again: the stages' own results stay readable and unchanged
        ctx.set_params(16, 8, 4, capi.ACCUM_HDR_F32)
        out = np.zeros((8, 16, 4), F)
        meter, noise = capi.MeterResult(), capi.NoiseResult()
        mhist = np.zeros(256, np.uint32)
        assert ctx.read_denoised().tobytes() == before["denoised"] and ctx.read_denoised_ldr().tobytes() == before["denoised_ldr"]
        assert ctx.read_display().tobytes() == before["display"] and ctx.read_display_ldr().tobytes() == before["display_ldr"]
        ctx._ck(L.jpt_read_meter(ctx.h, host.C.byref(meter), host._ptr(mhist)), "jpt_read_meter")
        assert bytes(meter) + mhist.tobytes() == before["meter"]
        # (the plane and the estimate are of the frames in the framebuffers, which every jpt_set_params makes anew: they go with them)
        refused(ctx, L.jpt_read_noise(ctx.h, host.C.byref(noise), None), "jpt_read_noise: no jpt_noise_estimate at the current size yet")
        refused(ctx, L.jpt_read_variance_f32(ctx.h, host._ptr(out)), "jpt_read_variance_f32: no render with the switch on at the current size yet")
        # another size: every read-back refuses, each with its own words
        ctx.set_params(8, 8, 4, capi.ACCUM_HDR_F32)
        refused(ctx, L.jpt_read_denoised_f32(ctx.h, host._ptr(out)), "no jpt_denoise at the current resolution yet")
        refused(ctx, L.jpt_read_display_f32(ctx.h, host._ptr(out)), "no jpt_display at the current resolution yet")
        refused(ctx, L.jpt_read_meter(ctx.h, host.C.byref(meter), None), "no jpt_meter since the metering state was reset")
        refused(ctx, L.jpt_read_noise(ctx.h, host.C.byref(noise), None), "jpt_read_noise: no jpt_noise_estimate at the current size yet")
        refused(ctx, L.jpt_read_variance_f32(ctx.h, host._ptr(out)), "jpt_read_variance_f32: no render with the switch on at the current size yet")
        # the stages again at the new size: what a context that only ever saw 8 x 8 gives
        run_stages(ctx, sc, 8, 8)
        got = read_all(ctx)
        assert sorted(got) == sorted(want)
        for name in sorted(want):
            assert got[name] == want[name], name
    finally:
        ctx.close()


def test_bake_stages_across_a_change_of_size(hiplib):
    """(the raw planes stay allocated until the next bake render re-makes them, so jpt_device_bake_directional must not answer them: what the
    read-back refuses, the pointer form gives as null -- PostState::framebuffers_remade forgets what the planes hold)"""
    L = hiplib
    sc, p4, n4 = atlas(8, 4)
    ctx = bake_ctx(sc, p4, n4)
    try:
        ctx.set_bake_directional(True)
        ctx.render(2, 1)
        ctx.bake_finish()
        ctx.bake_finish_directional()
        assert ctx.read_lightmap().shape == (4, 8, 4) and ctx.read_lightmap_directional().shape == (3, 4, 8, 4)
        assert ctx.read_bake_directional().shape == (3, 4, 8, 4)
        for finished in (False, True):
            ptr, nbytes = ctx.device_bake_directional(finished)
            assert ptr and nbytes == 3 * 8 * 4 * 16
        ctx.set_params(4, 4, 4, capi.ACCUM_HDR_F32)
        out = np.zeros((3, 4, 8, 4), F)
        refused(ctx, L.jpt_read_lightmap_f32(ctx.h, host._ptr(out)), "jpt_read_lightmap_f32: no jpt_bake_finish at the current size and bake images yet")
        refused(ctx, L.jpt_read_lightmap_directional_f32(ctx.h, host._ptr(out)),
                "jpt_read_lightmap_directional_f32: no jpt_bake_finish_directional at the current size and bake images yet")
        refused(ctx, L.jpt_read_bake_directional_f32(ctx.h, host._ptr(out)),
                "jpt_read_bake_directional_f32: no bake render with the switch on at the current size yet")
        for finished in (False, True):
            assert ctx.device_bake_directional(finished) == (None, 0), finished
    finally:
        ctx.close()
