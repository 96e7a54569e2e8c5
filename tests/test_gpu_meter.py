"""jpt_meter on the device: the kernels against the restatement in every bin and bit (jpt_debug_meter), the call through a context
against the restatement applied to what the context read back, the recurrence over calls, jpt_display's auto-exposure form against
np_display with the product of the two exposures, and that nothing else moves -- renders, read-backs, the workspace and, with the
switch off, jpt_display's images are byte for byte what they are without metering."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_display as nd
import np_meter as nm
from test_meter_host import CLIPS, SIZES, check_against_restatement, same_result

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
LOOK = dict(exposure=1.5, tonemap=capi.TONEMAP_REINHARD, transfer=capi.TRANSFER_SRGB, white=3.0, bloom_threshold=0.6, bloom_strength=0.8)


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def make_ctx(w=W, h=H, sc=None):
    sc = sc or scenes.cornell_scene()
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 3, capi.ACCUM_HDR_F32)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    return ctx


def same_meter(ctx, want, what):
    res, hist = ctx.read_meter()
    bad = np.flatnonzero(hist.astype(np.int64) != np.array(want[0], np.int64))
    assert not len(bad), "%s: %d bins differ, first %s" % (what, len(bad), [(int(b), int(hist[b]), want[0][b]) for b in bad[:4]])
    same_result(res, want[1], what)
    return res


# ---- the kernels equal the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [nm.AVERAGE, nm.CENTER_WEIGHTED])
@pytest.mark.parametrize("size", SIZES)
def test_device_form_equals_the_restatement_in_every_bin_and_bit(L, size, mode):
    img = nm.edge_image(size[0], size[1], seed=size[0])
    for low, high in CLIPS:
        check_against_restatement(L, 0, img, mode=mode, low_permille=low, high_permille=high)
        for adapt in (0.0, 0.25, 1.0):
            check_against_restatement(L, 0, img, prev=0.75, mode=mode, low_permille=low, high_permille=high, adapt=adapt)


def test_device_form_on_empty_and_clamped_images(L):
    black = np.zeros((9, 33, 4), F)
    skipped = np.full((9, 33, 4), np.nan, F)
    for img in (black, skipped):
        _, res = check_against_restatement(L, 0, img)
        assert res["flags"] == nm.EMPTY | nm.FIRST and res["exposure"] == 1.0
        _, res = check_against_restatement(L, 0, img, prev=3.5, adapt=0.25)
        assert res["flags"] == nm.EMPTY and res["exposure"] == 3.5
    _, res = check_against_restatement(L, 0, np.full((9, 33, 4), 1e-4, F))
    assert res["exposure"] == 64.0
    _, res = check_against_restatement(L, 0, np.full((9, 33, 4), 500.0, F))
    assert res["exposure"] == 1.0 / 64.0


@pytest.mark.parametrize("value", [0.18, 1.0])
@pytest.mark.parametrize("mode", [nm.AVERAGE, nm.CENTER_WEIGHTED])
def test_a_flat_image_lands_in_one_bin(L, value, mode):
    """every lane of every wave names the same bin"""
    img = np.full((64, 64, 4), value, F)
    hist, res = check_against_restatement(L, 0, img, mode=mode)
    total = 4096 + (3 * 1024 if mode == nm.CENTER_WEIGHTED else 0)
    assert np.count_nonzero(hist) == 1 and int(hist.sum()) == total and res["weight"] == total
    # ... and with one pixel of another bin in the middle of a wave, and one skipped
    img[10, 37, :3] = 40.0
    img[33, 5, :3] = np.nan
    hist, _ = check_against_restatement(L, 0, img, mode=mode)
    assert np.count_nonzero(hist) == 2


def test_many_blocks_and_short_rows(L):
    """2048 x 3: the sum of the bins is the number of counted pixels times their weights"""
    img = nm.edge_image(2048, 3, seed=5)
    counted = nm.bins_of(img) >= 0
    assert 0 < (~counted).sum()
    hist, res = check_against_restatement(L, 0, img)
    assert int(hist.sum()) == int(counted.sum()) == res["weight"]
    hist, res = check_against_restatement(L, 0, img, mode=nm.CENTER_WEIGHTED)
    assert int(hist.sum()) == int((nm.weights_of(3, 2048, nm.CENTER_WEIGHTED) * counted).sum()) == res["weight"]


# ---- through a context ------------------------------------------------------------------------------------------------------------

def test_meter_through_a_context_and_the_recurrence(hiplib):
    ctx = make_ctx()
    try:
        ctx.render(2, 1)
        acc = ctx.read_accum()
        ctx.meter()
        first = same_meter(ctx, nm.meter(acc, 2), "the accumulation, 2 frames")
        assert first["flags"] == nm.FIRST and first["weight"] > 0
        res_only, no_hist = ctx.read_meter(histogram=False)
        assert no_hist is None and res_only == first
        # the recurrence, bit for bit, with other parameters (which do not reset the state)
        prm = dict(mode=nm.CENTER_WEIGHTED, low_permille=200, high_permille=950, key=0.5, adapt=0.25)
        ctx.set_meter_params(**prm)
        prev = first["exposure"]
        for k in range(2):
            ctx.meter()
            res = same_meter(ctx, nm.meter(acc, 2, prev, **prm), "call %d of the recurrence" % (k + 2))
            assert res["flags"] == 0 and res["exposure"] != prev
            prev = res["exposure"]
        ctx.meter_reset()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_meter since"):
            ctx.read_meter()
        ctx.meter()
        res = same_meter(ctx, nm.meter(acc, 2, None, **prm), "after jpt_meter_reset")
        assert res["flags"] == nm.FIRST and nm.bits(res["exposure"]) == nm.bits(res["target"])
        # the denoised source, fc = 1
        ctx.set_meter_params(source=capi.DISPLAY_SOURCE_DENOISED)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_denoise at the current resolution"):
            ctx.meter()
        ctx.denoise()
        ctx.meter()
        same_meter(ctx, nm.meter(ctx.read_denoised(), 1, res["exposure"]), "the denoised image")
        # more frames: the frame count follows
        ctx.set_meter_params()
        ctx.render(3, 3)
        ctx.meter_reset()
        ctx.meter()
        same_meter(ctx, nm.meter(ctx.read_accum(), 5), "5 frames")
    finally:
        ctx.close()


@pytest.mark.parametrize("levels", [0, 2])
def test_auto_exposure_is_the_product_of_the_two_exposures(hiplib, levels):
    ctx = make_ctx()
    look = dict(LOOK, bloom_levels=levels)
    try:
        ctx.render(2, 1)
        ctx.set_display_params(**look)
        ctx.set_auto_exposure(True)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_meter ran"):
            ctx.display()
        ctx.set_meter_params(key=0.6)
        ctx.meter()
        ctx.display()
        metered = ctx.read_meter()[0]["exposure"]
        assert metered != 1.0
        acc = ctx.read_accum()
        want = nd.display(acc, 2, **dict(look, exposure=F(look["exposure"]) * F(metered)))
        got = ctx.read_display(), ctx.read_display_ldr()
        assert nd.same_bits(got[0], want[0]).all() and np.array_equal(got[1], want[1])
        # queued: the display reads the state the jpt_meter before it on the stream left, not a later one
        ctx.set_meter_params(key=0.6, adapt=0.25, min_exposure=32.0)
        ctx.render(1, 3, asynchronous=True)
        ctx.meter()
        ctx.display()
        ctx.set_meter_params(key=0.05, adapt=1.0)
        ctx.meter()
        ctx.sync()
        got = ctx.read_display(), ctx.read_display_ldr()
        acc = ctx.read_accum()
        second = nm.meter(acc, 3, metered, key=0.6, adapt=0.25, min_exposure=32.0)[1]["exposure"]
        want = nd.display(acc, 3, **dict(look, exposure=F(look["exposure"]) * F(second)))
        assert nd.same_bits(got[0], want[0]).all() and np.array_equal(got[1], want[1])
        same_meter(ctx, nm.meter(acc, 3, second, key=0.05), "the later jpt_meter")
        # off again: the parameter alone
        ctx.set_auto_exposure(False)
        ctx.display()
        want = nd.display(acc, 3, **look)
        got = ctx.read_display(), ctx.read_display_ldr()
        assert nd.same_bits(got[0], want[0]).all() and np.array_equal(got[1], want[1])
        # a reset of the state: auto-exposure has nothing to read
        ctx.set_auto_exposure(True)
        ctx.meter_reset()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_meter ran"):
            ctx.display()
    finally:
        ctx.close()


# ---- nothing else moves ------------------------------------------------------------------------------------------------------------

def _images(ctx):
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("accumulation", "display", "depth")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs" % (what, name)


def test_metering_changes_no_other_buffer_no_later_render_and_no_display(hiplib):
    sc = scenes.cornell_scene()
    a, b = make_ctx(sc=sc), make_ctx(sc=sc)
    look = dict(LOOK, bloom_levels=2)
    try:
        a.set_meter_params(mode=nm.CENTER_WEIGHTED, adapt=0.5)
        a.render(2, 1)
        before = _images(a)
        a.meter()
        _same(_images(a), before, "read-backs around jpt_meter")
        first = 3
        for k in range(3):
            a.render(2, first, asynchronous=True)
            a.meter()
            first += 2
        b.render(2, 1)
        first = 3
        for k in range(3):
            b.render(2, first, asynchronous=True)
            first += 2
        _same(_images(a), _images(b), "a context that never called jpt_meter")
        assert a.workspace_bytes() == b.workspace_bytes()
        # with the switch off, jpt_display is what it is on a context that never heard of metering
        a.set_display_params(**look)
        b.set_display_params(**look)
        a.display()
        b.display()
        assert np.array_equal(a.read_display().view(np.uint8), b.read_display().view(np.uint8))
        assert np.array_equal(a.read_display_ldr(), b.read_display_ldr())
        a.meter()
        _same(_images(a), _images(b), "after one more jpt_meter")
        assert a.workspace_bytes() == b.workspace_bytes()
    finally:
        a.close()
        b.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------

def test_state_errors_a_resolution_change_and_a_single_pixel(hiplib):
    sc = scenes.cornell_scene()
    ctx = host.Context(0)
    try:
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_params not called"):
            ctx.meter()
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(W, H, 3, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, W, H))
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.meter()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_meter since"):
            ctx.read_meter()
        ctx.render(1, 1)
        for mode in (capi.DENOISE_TEMPORAL, capi.DENOISE_NONE):
            ctx.set_denoising_mode(mode)
            with pytest.raises(capi.JptError, match=r"\(-4\).*JPT_DENOISE_PROGRESSIVE"):
                ctx.meter()
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)     # (a change of mode restarts the accumulation)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.meter()
        ctx.render(1, 1)
        ctx.set_debug_steps(True)
        with pytest.raises(capi.JptError, match=r"\(-4\).*DEBUG_STEPS"):
            ctx.meter()
        ctx.set_debug_steps(False)
        ctx.set_partition(0, 2)
        ctx.render(1, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*whole image on one context"):
            ctx.meter()
        ctx.set_partition(0, 1)
        ctx.render(1, 1)
        ctx.meter()
        assert ctx.read_meter()[0]["flags"] == nm.FIRST
        with pytest.raises(capi.JptError, match=r"\(-1\).*high_permille"):
            ctx.set_meter_params(low_permille=500, high_permille=400)
        ctx.meter()                                              # the refused parameters changed nothing
        assert ctx.read_meter()[0]["flags"] == 0
        ctx.set_params(1, 1, 3, capi.ACCUM_HDR_F32)              # another resolution resets the state; a 1 x 1 image works
        ctx.set_camera(scenes.camera_block(sc.camera, 1, 1))
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_meter since"):
            ctx.read_meter()
        ctx.render(2, 1)
        ctx.meter()
        res = same_meter(ctx, nm.meter(ctx.read_accum(), 2), "1 x 1")
        assert res["flags"] & nm.FIRST and res["weight"] <= 1
    finally:
        ctx.close()
