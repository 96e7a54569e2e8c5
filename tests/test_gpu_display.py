"""jpt_display on the device: the kernels against the numpy restatement bit for bit (jpt_debug_display), the whole call through a
context against the restatement applied to what the context read back, the two identities with the existing display images, and
that nothing else moves -- the accumulation, the display image, the depth image, the denoised image and later renders are bit for
bit what they are without the call."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_display as nd
from test_display_host import GRADE, SIZES, check_against_restatement

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
SCENES = {"cornell": scenes.cornell_scene, "demo800": lambda: scenes.demo_scene(800)}
LOOK = dict(bloom_levels=4, exposure=2.5, tonemap=capi.TONEMAP_REINHARD, transfer=capi.TRANSFER_SRGB, white=3.0, bloom_threshold=0.6,
            bloom_strength=0.8)


def make_ctx(sc, w=W, h=H, accum=capi.ACCUM_HDR_F32, bounces=3):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, bounces, accum)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    return ctx


# ---- the kernels equal the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", range(7))
def test_device_transform_equals_the_numpy_restatement_bit_for_bit(hiplib, levels):
    for w, h in SIZES:
        for tonemap in (nd.ACES_REF, nd.REINHARD, nd.CLAMP):
            for transfer in (nd.LINEAR, nd.SRGB):
                check_against_restatement(hiplib, 0, w, h, w + levels, bloom_levels=levels, tonemap=tonemap, transfer=transfer, **GRADE)


def test_device_transform_at_full_hd_with_five_levels(hiplib):
    check_against_restatement(hiplib, 0, 1920, 1080, 21, bloom_levels=5, tonemap=nd.REINHARD, transfer=nd.SRGB, **GRADE)
    check_against_restatement(hiplib, 0, 1920, 1080, 22, bloom_levels=5)


# ---- through a context ------------------------------------------------------------------------------------------------------------

def _same_images(got, want, what):
    bad = ~nd.same_bits(got[0], want[0])
    assert not bad.any(), "%s: %d values differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    bad = got[1] != want[1]
    assert not bad.any(), "%s: %d codes differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("accum", [capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_display_through_a_context(hiplib, name, accum):
    ctx = make_ctx(SCENES[name](), accum=accum)
    what = "%s accum %d" % (name, accum)
    try:
        ctx.render(3, 1)
        ctx.denoise()
        # the defaults are the existing display image
        ctx.display()
        assert np.array_equal(ctx.read_display_ldr(), ctx.read_ldr()), what + ": defaults != jpt_read_ldr_rgba8"
        _same_images((ctx.read_display(), ctx.read_display_ldr()), nd.display(ctx.read_accum(), 3), what + ", defaults")
        # the denoised source with the defaults is the denoiser's display image
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED)
        ctx.display()
        assert np.array_equal(ctx.read_display_ldr(), ctx.read_denoised_ldr()), what + ": DENOISED defaults != jpt_read_denoised_rgba8"
        # a look: both outputs equal the restatement applied to the read-backs
        ctx.set_display_params(**LOOK)
        ctx.display()
        _same_images((ctx.read_display(), ctx.read_display_ldr()), nd.display(ctx.read_accum(), 3, **LOOK), what + ", the look on the accumulation")
        assert not np.array_equal(ctx.read_display_ldr(), ctx.read_ldr())
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED, **LOOK)
        ctx.display()
        _same_images((ctx.read_display(), ctx.read_display_ldr()), nd.display(ctx.read_denoised(), 1, **LOOK), what + ", the look on the denoised image")
        # more frames, another frame count
        ctx.render(2, 4)
        ctx.set_display_params(bloom_levels=6, transfer=capi.TRANSFER_SRGB)
        ctx.display()
        _same_images((ctx.read_display(), ctx.read_display_ldr()), nd.display(ctx.read_accum(), 5, bloom_levels=6, transfer=nd.SRGB), what + ", 5 frames")
    finally:
        ctx.close()


def test_display_of_a_sun_lit_render_with_both_mis_modes(hiplib):
    from test_gpu_light_sampling import sun_map
    ctx = make_ctx(scenes.cornell_scene())
    try:
        ctx.set_environment(sun_map())
        ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
        ctx.render(4, 1)
        ctx.set_display_params(**LOOK)
        ctx.display()
        _same_images((ctx.read_display(), ctx.read_display_ldr()), nd.display(ctx.read_accum(), 4, **LOOK), "map + both MIS modes")
    finally:
        ctx.close()


# ---- nothing else moves ------------------------------------------------------------------------------------------------------------

def _images(ctx):
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.read_denoised()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("accumulation", "display", "depth", "denoised")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("accum", [capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8])
def test_display_changes_no_other_buffer_and_no_later_render(hiplib, accum):
    sc = scenes.demo_scene(800)
    a, b = make_ctx(sc, accum=accum), make_ctx(sc, accum=accum)
    try:
        a.set_display_params(**LOOK)
        a.render(2, 1)
        a.denoise()
        before = _images(a)
        a.display()
        _same(_images(a), before, "read-backs around jpt_display")
        a.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED, **LOOK)
        a.display()
        _same(_images(a), before, "read-backs around jpt_display of the denoised image")
        first = 3
        for k in range(3):
            a.render(2, first, asynchronous=True)
            a.display()
            first += 2
        b.render(2, 1)
        first = 3
        for k in range(3):
            b.render(2, first, asynchronous=True)
            first += 2
        a.denoise()
        b.denoise()
        _same(_images(a), _images(b), "a context that never called jpt_display")
        a.display()
        _same(_images(a), _images(b), "after one more jpt_display")
    finally:
        a.close()
        b.close()


def test_display_between_queued_renders_sees_the_frames_queued_before_it(hiplib):
    sc = scenes.cornell_scene()
    a, b = make_ctx(sc), make_ctx(sc)
    try:
        a.set_display_params(**LOOK)
        a.render(2, 1, asynchronous=True)
        a.display()
        a.render(2, 3, asynchronous=True)
        a.sync()
        got = a.read_display(), a.read_display_ldr()
        b.render(2, 1)
        _same_images(got, nd.display(b.read_accum(), 2, **LOOK), "the display image is the first render's")
        b.render(2, 3)
        assert np.array_equal(a.read_accum().view(np.uint8), b.read_accum().view(np.uint8))
        assert not np.array_equal(nd.display(b.read_accum(), 4, **LOOK)[1], got[1])
    finally:
        a.close()
        b.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------

def test_state_errors_and_a_resolution_change_on_a_device_context(hiplib):
    sc = scenes.cornell_scene()
    ctx = host.Context(0)
    try:
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_params not called"):
            ctx.display()
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(W, H, 3, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, W, H))
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.display()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_display at the current resolution"):
            ctx.read_display()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_display at the current resolution"):
            ctx.read_display_ldr()
        ctx.render(1, 1)
        for mode in (capi.DENOISE_TEMPORAL, capi.DENOISE_NONE):
            ctx.set_denoising_mode(mode)
            with pytest.raises(capi.JptError, match=r"\(-4\).*JPT_DENOISE_PROGRESSIVE"):
                ctx.display()
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)     # (a change of mode restarts the accumulation)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.display()
        ctx.render(1, 1)
        ctx.set_debug_steps(True)
        with pytest.raises(capi.JptError, match=r"\(-4\).*DEBUG_STEPS"):
            ctx.display()
        ctx.set_debug_steps(False)
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_denoise at the current resolution"):
            ctx.display()
        ctx.denoise()
        ctx.display()
        assert ctx.read_display().shape == (H, W, 4)
        ctx.set_display_params(bloom_levels=3)
        ctx.accum_reset()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.display()
        ctx.set_partition(0, 2)
        ctx.render(1, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*whole image on one context"):
            ctx.display()
        ctx.set_partition(0, 1)
        ctx.render(1, 1)
        ctx.display()
        ctx.set_params(W + 8, H + 3, 3, capi.ACCUM_HDR_F32)   # another resolution: the old images are gone
        ctx.set_camera(scenes.camera_block(sc.camera, W + 8, H + 3))
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_display at the current resolution"):
            ctx.read_display_ldr()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_display at the current resolution"):
            ctx.read_display()
        ctx.render(2, 1)
        ctx.display()
        got = ctx.read_display(), ctx.read_display_ldr()
        assert got[1].shape == (H + 3, W + 8, 4)
        _same_images(got, nd.display(ctx.read_accum(), 2, bloom_levels=3), "after the resolution change")
        with pytest.raises(capi.JptError, match=r"\(-1\).*bloom_levels"):
            ctx.set_display_params(bloom_levels=7)
        ctx.display()                                            # the refused parameters changed nothing
        _same_images((ctx.read_display(), ctx.read_display_ldr()), got, "after refused parameters")
    finally:
        ctx.close()


def test_parameters_survive_a_scene_change_and_are_not_shared(hiplib):
    a, b = make_ctx(scenes.cornell_scene()), host.Context(0)
    try:
        a.set_display_params(**LOOK)
        a.build_scene(scenes.demo_scene(800), capi.BUILD_SAH)
        a.set_camera(scenes.camera_block(scenes.demo_scene(800).camera, W, H))
        a.accum_reset()
        a.render(2, 1)
        a.display()
        _same_images((a.read_display(), a.read_display_ldr()), nd.display(a.read_accum(), 2, **LOOK), "after a scene change")
        b.share_scene_from(a)
        b.set_params(W, H, 3, capi.ACCUM_HDR_F32)
        b.set_camera(scenes.camera_block(scenes.demo_scene(800).camera, W, H))
        b.render(2, 1)
        b.display()
        assert np.array_equal(b.read_display_ldr(), b.read_ldr()), "the sharing context keeps the defaults"
    finally:
        a.close()
        b.close()
