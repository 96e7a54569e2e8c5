"""The variance guidance of jpt_denoise on the device: the kernels against the host form of the same functions, the whole call through a
context against the numpy restatement applied to what the context read back, that switching the guidance off gives jpt_denoise's bits
back, its place among queued renders, its refusals, and jpt_display over its image."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_denoise as nd
import np_denoise_var as nv
import np_display as npd

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
LOOK = dict(bloom_levels=4, exposure=2.5, tonemap=capi.TONEMAP_REINHARD, transfer=capi.TRANSFER_SRGB, white=3.0, bloom_threshold=0.6,
            bloom_strength=0.8)


def make_ctx(builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, variance=True):
    sc = scenes.cornell_scene()
    ctx = host.Context(0)
    ctx.build_scene(sc, builder)
    ctx.set_params(W, H, 4, accum)
    ctx.set_kernel(capi.KERNEL_WAVEFRONT)
    ctx.set_camera(scenes.camera_block(sc.camera, W, H))
    if variance:
        ctx.set_variance(True)
    return ctx


def assert_same(got, want, what):
    bad = ~nd.same_bits(got, want)
    assert not bad.any(), "%s: %d values differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- a. the kernels equal the host form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (5, 3), (33, 9), (70, 21)], ids=lambda s: "%dx%d" % s)
def test_device_filter_equals_its_host_form(hiplib, size):
    w, h = size
    for passes in range(1, 7):
        for frames, vprm in ((4, {}), (2, dict(sigma_variance=0.5, variance_floor=1e-3))):
            case = nv.synthetic_case(w, h, seed=w * 10 + passes, frame_count=frames)
            args = dict(params=capi.DenoiseParams(passes=passes), vparams=capi.DenoiseVarianceParams(enable=1, **vprm))
            dev = host.debug_atrous_variance(0, case[0], case[1], frames, *case[2:], **args)
            hst = host.debug_atrous_variance(-1, case[0], case[1], frames, *case[2:], **args)
            assert_same(dev[0], hst[0], "%dx%d passes %d frames %d: image" % (w, h, passes, frames))
            assert_same(dev[1], hst[1], "%dx%d passes %d frames %d: variance" % (w, h, passes, frames))


# ---- b., c. through a context ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accum", [capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8])
@pytest.mark.parametrize("builder", [capi.BUILD_SAH, capi.BUILD_REFERENCE_EXACT])
def test_guided_denoise_equals_the_restatement_applied_to_what_was_read_back(hiplib, builder, accum):
    ctx = make_ctx(builder, accum)
    try:
        ctx.render(4, 1)
        ctx.denoise()
        unguided = ctx.read_denoised(), ctx.read_denoised_ldr()
        with pytest.raises(capi.JptError, match=r"\(-4\).*without jpt_set_denoise_variance"):
            ctx.read_denoised_variance()
        before = ctx.read_accum(), ctx.read_variance(), ctx.read_ldr()
        ctx.set_denoise_variance(enable=1)
        ctx.denoise()
        got = ctx.read_denoised(), ctx.read_denoised_ldr(), ctx.read_denoised_variance()
        after = ctx.read_accum(), ctx.read_variance(), ctx.read_ldr()
        for x, y, name in zip(before, after, ("accumulation", "variance plane", "display image")):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name + " changed by the guided jpt_denoise"
        want, want_v = nv.denoise(after[0], after[1], 4, *ctx.read_guides())
        assert_same(got[0], want, "denoised image")
        assert np.array_equal(got[1], nd.display(want)), "display image of the denoised image"
        assert_same(got[2], want_v, "variance of the last pass")
        assert not np.array_equal(got[0], unguided[0])
        # other parameters, more frames
        ctx.set_denoise_params(passes=3, normal_power_log2=2, sigma_plane=0.1, sigma_color=1.5)
        ctx.set_denoise_variance(enable=1, sigma_variance=1.25, variance_floor=1e-4)
        ctx.render(2, 5)
        ctx.denoise()
        want, want_v = nv.denoise(ctx.read_accum(), ctx.read_variance(), 6, *ctx.read_guides(), passes=3, normal_power_log2=2, sigma_plane=0.1,
                                  sigma_variance=1.25, variance_floor=1e-4)
        assert_same(ctx.read_denoised(), want, "denoised image, other parameters")
        assert_same(ctx.read_denoised_variance(), want_v, "variance of the last pass, other parameters")
    finally:
        ctx.close()


def test_switching_the_guidance_off_gives_jpt_denoise_its_bits_back(hiplib):
    ctx = make_ctx()
    try:
        ctx.render(4, 1)
        ctx.denoise()
        first = ctx.read_denoised(), ctx.read_denoised_ldr()
        ctx.set_denoise_variance(enable=1)
        ctx.denoise()
        assert not np.array_equal(ctx.read_denoised(), first[0])
        ctx.set_denoise_variance()                    # the defaults: off
        ctx.denoise()
        assert_same(ctx.read_denoised(), first[0], "denoised image after the guidance was switched off")
        assert np.array_equal(ctx.read_denoised_ldr(), first[1])
        assert_same(first[0], nd.denoise(ctx.read_accum(), 4, *ctx.read_guides()), "and it is the restatement's")
        with pytest.raises(capi.JptError, match=r"\(-4\).*without jpt_set_denoise_variance"):
            ctx.read_denoised_variance()
    finally:
        ctx.close()


# ---- d. ordering -----------------------------------------------------------------------------------------------------------------------

def test_guided_denoise_between_queued_renders_sees_the_frames_queued_before_it(hiplib):
    a, b = make_ctx(), make_ctx()
    try:
        for ctx in (a, b):
            ctx.set_denoise_variance(enable=1)
        a.render(3, 1, asynchronous=True)
        a.denoise()
        a.render(2, 4, asynchronous=True)
        a.sync()
        b.render(3, 1)
        b.sync()
        b.denoise()
        assert_same(a.read_denoised(), b.read_denoised(), "denoised image")
        assert_same(a.read_denoised_variance(), b.read_denoised_variance(), "variance of the last pass")
        want, want_v = nv.denoise(b.read_accum(), b.read_variance(), 3, *b.read_guides())
        assert_same(a.read_denoised(), want, "denoised image against the restatement of the first render's state")
        assert_same(a.read_denoised_variance(), want_v, "variance against the restatement of the first render's state")
        b.render(2, 4)
        for x, y, name in zip((a.read_accum(), a.read_variance()), (b.read_accum(), b.read_variance()), ("accumulation", "variance plane")):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name + " after the queue"
    finally:
        a.close()
        b.close()


# ---- e. refusals -----------------------------------------------------------------------------------------------------------------------

def test_guided_denoise_refuses_without_a_variance_of_two_frames(hiplib):
    ctx = make_ctx(variance=False)
    try:
        ctx.set_denoise_variance(enable=1)
        ctx.render(2, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_denoise_variance.*switched off \(jpt_set_variance\)"):
            ctx.denoise()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_denoise at the current resolution"):
            ctx.read_denoised()                       # (no fall-back ran)
        ctx.set_variance(True)                        # (a change of the switch restarts the accumulation)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.denoise()
        ctx.render(1, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_denoise_variance.*a variance needs two"):
            ctx.denoise()
        ctx.render(1, 2)
        ctx.denoise()
        assert ctx.read_denoised_variance().shape == (H, W)
        ctx.accum_reset()
        ctx.render(1, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*a variance needs two"):
            ctx.denoise()
        for fields in (dict(sigma_variance=0.0), dict(variance_floor=float("nan")), dict(reserved=3), dict(enable=2)):
            with pytest.raises(capi.JptError, match=r"\(-1\).*jpt_denoise_variance_params"):
                ctx.set_denoise_variance(**fields)
        ctx.set_denoise_variance(enable=0)
        ctx.denoise()                                 # one frame is enough for the fixed tolerance
        # another resolution: the images are gone
        ctx.set_denoise_variance(enable=1)
        ctx.set_params(W + 8, H, 4, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(scenes.cornell_scene().camera, W + 8, H))
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_denoise at the current resolution"):
            ctx.read_denoised_variance()
        ctx.render(2, 1)
        ctx.denoise()
        assert ctx.read_denoised_variance().shape == (H, W + 8)
    finally:
        ctx.close()


# ---- f. jpt_display over the guided image ------------------------------------------------------------------------------------------------

def test_display_of_the_guided_image_equals_the_restatement(hiplib):
    ctx = make_ctx()
    try:
        ctx.set_denoise_variance(enable=1)
        ctx.render(4, 1)
        ctx.denoise()
        guided = ctx.read_denoised()
        assert_same(guided, nv.denoise(ctx.read_accum(), ctx.read_variance(), 4, *ctx.read_guides())[0], "guided image")
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED, **LOOK)
        ctx.display()
        want_f32, want_ldr = npd.display(guided, 1, **LOOK)
        assert_same(ctx.read_display(), want_f32, "display of the guided image")
        assert np.array_equal(ctx.read_display_ldr(), want_ldr)
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED)
        ctx.display()
        assert np.array_equal(ctx.read_display_ldr(), ctx.read_denoised_ldr())
    finally:
        ctx.close()
