"""jpt_bake_finish on the device: the kernels of the whole transform (jpt_debug_bake_finish, device 0) and the context's call against the
numpy restatement (tests/np_lightmap.py) bit for bit, what the call leaves untouched, its place among queued renders, the lifetime of
its images and its refusals.  At most 70 x 41 texels, 2 frames, 4 bounces."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_lightmap as nl
from test_bake_host import atlas
from test_gpu_bake import KERNELS, bake_ctx

pytestmark = pytest.mark.gpu

F = np.float32
E_STATE = -4   # JPT_E_STATE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. the device form equals the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ((33, 17), (32, 32), (70, 41)), ids=lambda s: "%dx%d" % s)
def test_device_form_equals_the_numpy_restatement_bit_for_bit(hiplib, size):
    """test_lightmap_host's images.  70 x 41: three tile columns, partial tiles on both axes, and step-16 taps that still land inside;
    passes 0..6 reach the halo-2 (first), halo-4 and gather kernels; dilate 0, 3 (an odd count: the other of ping / pong) and 64"""
    w, h = size
    mean, p4, n4 = nl.synthetic_case(w, h, seed=w)
    for passes in range(0, 7):
        filtered = nl.finish(mean, p4, n4, passes=passes, dilate=0)
        for dilate in (0, 3, 64):
            want = filtered
            with np.errstate(all="ignore"):
                for _ in range(dilate):
                    want = nl.dilate_pass(want)
            got = host.debug_bake_finish(0, mean, p4, n4, passes=passes, dilate=dilate)
            bad = ~nl.same_bits(got, want)
            assert not bad.any(), "%dx%d passes %d dilate %d: %d values differ, first %s" % (w, h, passes, dilate, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    prm = dict(passes=4, normal_power_log2=0, sigma_distance=1.5, sigma_plane=0.25, sigma_color=0.5, dilate=2)
    assert nl.same_bits(host.debug_bake_finish(0, mean, p4, n4, **prm), nl.finish(mean, p4, n4, **prm)).all()
    assert nl.same_bits(host.debug_bake_finish(0, mean, p4, n4), nl.finish(mean, p4, n4)).all()        # the defaults


# ---- 2. through a context ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_the_context_finishes_its_bake_and_touches_nothing_else(hiplib, kernel):
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)

    def run(finish):
        ctx = bake_ctx(sc, p4, n4, kernel=kernel)
        try:
            ctx.render(2, 1)
            lightmap = None
            if finish:
                ctx.bake_finish()
                lightmap = ctx.read_lightmap()
            return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), lightmap
        finally:
            ctx.close()
    plain, finished = run(False), run(True)
    for a, b in zip(plain[:3], finished[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    with np.errstate(all="ignore"):
        mean = (finished[0] / F(2.0)).astype(F)
    want = nl.finish(mean, p4, n4)
    got = finished[3]
    bad = ~nl.same_bits(got, want)
    assert not bad.any(), "%d values differ, first %s" % (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # and it is a lightmap: the charts covered, a ring around them, something lit, the filter not the identity
    assert (got[..., 3] == 1).any() and (got[..., 3] == 0.5).any() and (got[..., :3] > 0).any()
    assert not np.array_equal(got[got[..., 3] == 1][:, :3], mean[got[..., 3] == 1][:, :3])


# ---- 3. ordering -------------------------------------------------------------------------------------------------------------------------------

def test_a_finish_between_queued_renders_takes_the_first_renders_accumulation(hiplib):
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)
    ctx = bake_ctx(sc, p4, n4)
    try:
        ctx.render(2, 1)
        first = ctx.read_accum()
        ctx.accum_reset()
        ctx.render(2, 1, asynchronous=True)
        ctx.bake_finish()
        ctx.render(2, 3, asynchronous=True)
        got = ctx.read_lightmap()
        both = ctx.read_accum()
    finally:
        ctx.close()
    with np.errstate(all="ignore"):
        want = nl.finish((first / F(2.0)).astype(F), p4, n4)
        later = nl.finish((both / F(4.0)).astype(F), p4, n4)
    assert not np.array_equal(first, both)
    assert nl.same_bits(got, want).all()
    assert not nl.same_bits(got, later).all()


# ---- 4. lifetime, parameters and refusals --------------------------------------------------------------------------------------------------------

def test_lifetime_parameters_and_refusals(hiplib):
    w, h = 32, 32
    sc, p4, n4 = atlas(w, h)
    ctx = bake_ctx(sc, p4, n4)
    L = ctx._lib
    out = np.zeros((h, w, 4), F)

    def refused(rc, call, word=b""):
        assert rc == E_STATE, rc
        msg = L.jpt_last_error(ctx.h)
        assert call in msg and word in msg, msg
    try:
        refused(L.jpt_read_lightmap_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_f32")            # before any finish
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"no frame")
        ctx.render(2, 1)
        with np.errstate(all="ignore"):
            mean = (ctx.read_accum() / F(2.0)).astype(F)
        before = ctx.workspace_bytes()
        ctx.bake_finish()
        assert ctx.workspace_bytes() == before
        assert nl.same_bits(ctx.read_lightmap(), nl.finish(mean, p4, n4)).all()
        # changed parameters take effect at the next call, not before
        ctx.set_bake_finish_params(passes=1, dilate=1, sigma_color=0.5)
        assert nl.same_bits(ctx.read_lightmap(), nl.finish(mean, p4, n4)).all()
        ctx.bake_finish()
        want = nl.finish(mean, p4, n4, passes=1, dilate=1, sigma_color=0.5)
        assert nl.same_bits(ctx.read_lightmap(), want).all() and not nl.same_bits(want, nl.finish(mean, p4, n4)).all()
        ctx.set_bake_finish_params(passes=0, dilate=0)
        ctx.bake_finish()
        assert nl.same_bits(ctx.read_lightmap(), nl.finish(mean, p4, n4, passes=0, dilate=0)).all()
        ctx.set_bake_finish_params()
        # new images: a read before a new finish is refused
        ctx.set_bake_texels(p4[::-1].copy(), n4[::-1].copy())
        refused(L.jpt_read_lightmap_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_f32")
        ctx.bake_finish()                                                                            # (the accumulation is still there)
        assert nl.same_bits(ctx.read_lightmap(), nl.finish(mean, p4[::-1], n4[::-1])).all()
        # the modes it refuses
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.accum_reset()
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"no frame")
        ctx.render(1, 1)
        ctx.bake_finish()
        # another size than the images'
        ctx.set_params(33, 17, 4, capi.ACCUM_HDR_F32)
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"32 x 32")
        refused(L.jpt_read_lightmap_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_f32")
        ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
        ctx.render(1, 1)
        ctx.bake_finish()
        ctx.read_lightmap()
        # without images
        ctx.set_bake_texels(None, None)
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"no bake images")
        refused(L.jpt_read_lightmap_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_f32")
        # a screen partition
        ctx.set_bake_texels(p4, n4)
        ctx.set_partition(1, 2)
        refused(L.jpt_bake_finish(ctx.h), b"jpt_bake_finish", b"whole image on one context")
        ctx.set_partition(0, 1)
        # jpt_denoise keeps refusing a bake context
        ctx.render(1, 1)
        assert L.jpt_denoise(ctx.h) == E_STATE and b"jpt_denoise" in L.jpt_last_error(ctx.h)
        ctx.bake_finish()
        assert np.isfinite(ctx.read_lightmap()).all()
    finally:
        ctx.close()
