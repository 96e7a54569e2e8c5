"""The history of jpt_denoise (jpt_set_denoise_history) on the device: history_kernel against the numpy restatement on the synthetic
cases of the host test, the whole call through a context against the restatement applied to what the context read back, a standing
camera against the progressive mean, that nothing else moves and the history-less call keeps its bits, the refusals, what drops the
history, the readers of the denoised image, and what the history gains under a moving camera."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_denoise as nd
import np_denoise_history as nh
import np_denoise_var as nv
import np_encode as ne
import np_meter as nm
from test_denoise_history_host import SIZES, U, stage_cases
from test_encode_host import lib_bits
from test_gpu_meter import same_meter

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)


def view(sc, w, h, step):
    """the scene's camera after `step` steps of a path that translates and turns"""
    t = np.asarray(sc.camera.transform, np.float64)
    basis, origin = scenes.rot_y(0.7 * step) @ t[:9].reshape(3, 3), t[9:] + step * np.array([0.06, 0.02, -0.05])
    return scenes.camera_block(scenes.CameraDesc(scenes.transform12(basis, origin), sc.camera.fov_deg, sc.camera.near, sc.camera.far), w, h)


def make_ctx(w=W, h=H, kernel=capi.KERNEL_WAVEFRONT, history=True, **fields):
    sc = scenes.cornell_scene()
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
    ctx.set_kernel(kernel)
    ctx.set_camera(view(sc, w, h, 0))
    if history:
        ctx.set_denoise_history(enable=1, **fields)
    return ctx, sc


def frame(ctx, cam, n, first):
    """the interactive loop's step: the camera, a fresh accumulation of n frames, the denoise"""
    ctx.set_camera(cam)
    ctx.accum_reset()
    ctx.render(n, first)
    ctx.denoise()


def same_view(a, b):
    return a is not None and a["vp"].tobytes() == b["vp"].tobytes() and a["position"].tobytes() == b["position"].tobytes()


def assert_same(got, want, what):
    bad = ~nd.same_bits(got, want)
    assert not bad.any(), "%s: %d values differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- a. the kernel equals the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES + [(64, 17)], ids=lambda s: "%dx%d" % s)
def test_device_stage_equals_the_numpy_restatement_bit_for_bit(hiplib, size):
    stage_cases(0, *size)


# ---- b. through a context ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_history_calls_equal_the_restatement_applied_to_what_was_read_back(hiplib, kernel, frames):
    """eight calls: the camera translates and turns for five and stands for three"""
    ctx, sc = make_ctx(kernel=kernel)
    try:
        prev, prev_cam, lengths = None, None, []
        for i in range(8):
            cam = view(sc, W, H, min(i, 4))
            frame(ctx, cam, frames, i * frames)
            acc, g = ctx.read_accum(), ctx.read_guides()
            same = same_view(prev_cam, cam)
            assert same == (i >= 5)
            iv, a, b = nh.step(acc, frames, *g, prev=prev, prev_vp=None if prev_cam is None else prev_cam["vp"], same_view=same)
            want, want_v = nh.filter_iv(iv, *g)
            got_iv, got_n = ctx.read_denoise_history()
            assert_same(got_iv, iv, "call %d: (m, v_0)" % i)
            assert_same(got_n, a[..., 3], "call %d: the history length" % i)
            assert_same(ctx.read_denoised(), want, "call %d: the denoised image" % i)
            assert np.array_equal(ctx.read_denoised_ldr(), nd.display(want)), "call %d: its display image" % i
            assert_same(ctx.read_denoised_variance(), want_v, "call %d: the variance of the last pass" % i)
            prev, prev_cam = (a, b, g[0]), cam
            lengths.append(float(np.median(got_n[got_n > 0])))
        print("median history length per call:", lengths)
        assert lengths[0] == frames and lengths[-1] > 5 * frames     # the history follows the surfaces through the moves
    finally:
        ctx.close()


@pytest.mark.parametrize("passes", [1, 2, 4])
def test_one_two_and_four_filter_passes_equal_the_restatement(hiplib, passes):
    """one pass: the first pass is the last one (remodulation, display image and variance plane from atrous_var_pre_kernel<true>); two
    and four: an even count, the other ping-pong parity"""
    ctx, sc = make_ctx()
    try:
        prm = dict(passes=passes, normal_power_log2=4, sigma_plane=0.05)
        ctx.set_denoise_params(sigma_color=4.0, **prm)
        ctx.set_denoise_variance(enable=0, sigma_variance=1.5, variance_floor=1e-4)
        prev, prev_cam = None, None
        for i in range(3):
            cam = view(sc, W, H, i)
            frame(ctx, cam, 2, 2 * i)
            g = ctx.read_guides()
            iv, a, b = nh.step(ctx.read_accum(), 2, *g, prev=prev, prev_vp=None if prev_cam is None else prev_cam["vp"], normal_power_log2=4)
            want, want_v = nh.filter_iv(iv, *g, sigma_variance=1.5, variance_floor=1e-4, **prm)
            assert_same(ctx.read_denoise_history()[0], iv, "call %d: (m, v_0)" % i)
            assert_same(ctx.read_denoised(), want, "call %d: the denoised image" % i)
            assert np.array_equal(ctx.read_denoised_ldr(), nd.display(want)), "call %d: its display image" % i
            assert_same(ctx.read_denoised_variance(), want_v, "call %d: the variance of the last pass" % i)
            prev, prev_cam = (a, b, g[0]), cam
    finally:
        ctx.close()


def test_a_standing_camera_integrates_the_progressive_mean(hiplib):
    """16 calls of one frame each against one accumulation of the same 16 frames: m * amod against sum / 16.  The bound: the
    sequential mean's step rounds four times on values <= 2 B (test_denoise_history_host), |m - mean| <= 8 k u B with B the largest
    demodulated sample of the pixel's frames; both sides carry the demodulation's own two roundings (3 u B more), and the progressive
    sum of k frames its k - 1 roundings, (k - 1) u B; times amod: |m * amod - sum / k| <= (9 k + 3) u B amod, B amod <= the largest
    frame value of the pixel, bounded here by the largest over the image."""
    k = 16
    ctx, sc = make_ctx(max_history=64)
    ref, _ = make_ctx(history=False)
    try:
        cam = view(sc, W, H, 0)
        peak = 0.0
        for i in range(k):
            frame(ctx, cam, 1, i)
            peak = max(peak, float(ctx.read_accum()[..., :3].max()))
        ref.render(k, 0)
        mean = ref.read_accum()[..., :3].astype(np.float64) / k
        iv, n = ctx.read_denoise_history()
        hit = n > 0
        assert (n[hit] == k).all() and np.array_equal(hit, ctx.read_guides()[0][..., 3] >= 0) and hit.sum() > 500
        got = iv[..., :3].astype(np.float64) * nd.amod(ctx.read_guides()[2])
        err = np.abs(got - mean)[hit].max()
        print("standing camera: |m * amod - mean| max %.3g, bound %.3g (largest frame value %.3g)" % (err, (9 * k + 3) * U * peak, peak))
        assert err <= (9 * k + 3) * U * peak
    finally:
        ctx.close()
        ref.close()


# ---- c. nothing else moves -------------------------------------------------------------------------------------------------------------------

def test_history_off_keeps_jpt_denoise_its_bits_and_no_render_sees_the_calls(hiplib):
    ctx, sc = make_ctx()
    plain, _ = make_ctx(history=False)
    try:
        ctx.set_variance(True)
        plain.set_variance(True)
        for i in range(4):
            cam = view(sc, W, H, i)
            frame(ctx, cam, 2, 2 * i)
            plain.set_camera(cam)
            plain.accum_reset()
            plain.render(2, 2 * i)
            for name, a, b in (("accumulation", ctx.read_accum(), plain.read_accum()), ("display image", ctx.read_ldr(), plain.read_ldr()),
                               ("depth image", ctx.read_depth(), plain.read_depth()), ("variance plane", ctx.read_variance(), plain.read_variance())):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s of render %d differs from the sequence without jpt_denoise" % (name, i)
        history = ctx.read_denoise_history()
        ctx.set_denoise_history()                       # the defaults: off
        ctx.denoise()
        assert_same(ctx.read_denoised(), nd.denoise(ctx.read_accum(), 2, *ctx.read_guides()), "jpt_denoise after history calls")
        ctx.set_denoise_variance(enable=1)
        ctx.denoise()
        want, want_v = nv.denoise(ctx.read_accum(), ctx.read_variance(), 2, *ctx.read_guides())
        assert_same(ctx.read_denoised(), want, "the guided jpt_denoise after history calls")
        assert_same(ctx.read_denoised_variance(), want_v, "its variance")
        with pytest.raises(capi.JptError, match=r"\(-4\).*since the history was dropped"):
            ctx.read_denoise_history()                  # switching drops it
        # on again: a first call; other parameters with the same switch keep the history
        ctx.set_denoise_variance()
        ctx.set_denoise_history(enable=1)
        cam = view(sc, W, H, 3)
        frame(ctx, cam, 1, 20)
        first = ctx.read_denoise_history()
        g0, acc0 = ctx.read_guides(), ctx.read_accum()
        set0 = nh.step(acc0, 1, *g0)
        ctx.set_denoise_history(enable=1, max_history=16)    # (other parameters, the same switch: kept)
        cam2 = view(sc, W, H, 4)
        frame(ctx, cam2, 1, 21)
        iv, a, b = nh.step(ctx.read_accum(), 1, *ctx.read_guides(), prev=(set0[1], set0[2], g0[0]), prev_vp=cam["vp"], max_history=16)
        got = ctx.read_denoise_history()
        assert_same(got[0], iv, "(m, v_0) after another view")
        assert_same(got[1], a[..., 3], "the history length after another view")
        assert_same(first[0], set0[0], "the first call's (m, v_0)")
        assert history[1].max() >= 2
    finally:
        ctx.close()
        plain.close()


# ---- d. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_what_a_history_call_refuses(hiplib):
    ctx, sc = make_ctx()
    try:
        ctx.render(1, 0)
        ctx.set_lens(0.05, 5.0)
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_denoise_history on: the lens radius"):
            ctx.denoise()
        ctx.set_lens(0.0, 5.0)
        ctx.set_camera_model(capi.CAMERA_PROJECTIVE)
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_denoise_history on: the camera model"):
            ctx.denoise()
        ctx.set_camera_model(capi.CAMERA_PINHOLE)
        texels = np.zeros((H, W, 4), F)
        ctx.set_bake_texels(texels, texels)
        with pytest.raises(capi.JptError, match=r"\(-4\).*bake images"):
            ctx.denoise()
        ctx.set_bake_texels(None, None)
        ctx.set_probes(np.zeros((1, 3), F), 8, 4, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*holds probes"):
            ctx.denoise()
        ctx.set_probes(None)
        ctx.set_reflection_probes(np.zeros((1, 3), F), 8, 1)
        with pytest.raises(capi.JptError, match=r"\(-4\).*reflection probes"):
            ctx.denoise()
        ctx.set_reflection_probes(None)
        with pytest.raises(capi.JptError, match=r"\(-4\).*since the history was dropped|no jpt_denoise at the current resolution"):
            ctx.read_denoise_history()                  # (nothing ran)
        ctx.denoise()
        with pytest.raises(capi.JptError, match=r"\(-4\).*would count them twice"):
            ctx.denoise()
        ctx.render(1, 1)                                # more frames on the same accumulation: still the frames of the call before
        with pytest.raises(capi.JptError, match=r"\(-4\).*would count them twice"):
            ctx.denoise()
        ctx.denoise_history_reset()                     # the reset releases the frames with the history that counted them
        ctx.denoise()
        n = ctx.read_denoise_history()[1]
        assert set(np.unique(n)) == {0.0, 2.0}
        with pytest.raises(capi.JptError, match=r"\(-4\).*would count them twice"):
            ctx.denoise()
        ctx.set_denoising_mode(capi.DENOISE_NONE)      # a change of the mode restarts the accumulation, as jpt_accum_reset does
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.denoise()
        ctx.render(1, 5)
        ctx.denoise()
        ctx.accum_reset()
        with pytest.raises(capi.JptError, match=r"\(-4\).*no frame accumulated"):
            ctx.denoise()
        ctx.render(1, 2)
        ctx.denoise()
        for fields in (dict(enable=2), dict(max_history=0), dict(min_history=40), dict(sigma_plane=0.0), dict(reserved=(0, 0, 0, 1))):
            with pytest.raises(capi.JptError, match=r"\(-1\).*jpt_denoise_history_params"):
                ctx.set_denoise_history(**fields)
        # a partition
        ctx.set_partition(0, 2)
        ctx.render(1, 3)
        with pytest.raises(capi.JptError, match=r"\(-4\).*whole image on one context"):
            ctx.denoise()
    finally:
        ctx.close()


# ---- e. what drops the history -------------------------------------------------------------------------------------------------------------

def test_another_size_and_the_reset_drop_the_history_and_a_moved_instance_starts_over(hiplib):
    ctx, sc = make_ctx()
    try:
        cam = view(sc, W, H, 0)
        for i in range(3):
            frame(ctx, cam, 2, 2 * i)
        n = ctx.read_denoise_history()[1]
        hit = n > 0
        assert (n[hit] == 6).all()
        ctx.denoise_history_reset()
        with pytest.raises(capi.JptError, match=r"\(-4\).*since the history was dropped"):
            ctx.read_denoise_history()
        frame(ctx, cam, 2, 6)
        n = ctx.read_denoise_history()[1]
        assert (n[hit] == 2).all() and (n[~hit] == 0).all()
        frame(ctx, cam, 2, 8)
        assert (ctx.read_denoise_history()[1][hit] == 4).all()
        # another size and back
        ctx.set_params(W + 8, H, 4, capi.ACCUM_HDR_F32)
        with pytest.raises(capi.JptError, match=r"\(-4\).*no jpt_denoise at the current resolution"):
            ctx.read_denoise_history()
        ctx.set_params(W, H, 4, capi.ACCUM_HDR_F32)
        frame(ctx, cam, 2, 10)
        n = ctx.read_denoise_history()[1]
        assert (n[hit] == 2).all() and (n[~hit] == 0).all()
        # a moved instance: its pixels, before and after, start over; the rest go on
        frame(ctx, cam, 2, 12)
        before = ctx.read_guides()
        t = np.stack([np.asarray(inst.transform, F) for inst in sc.instances])
        t[2, 9:12] += np.array([0.9, 0.0, 0.4], F)            # the short block
        ctx.refit_tlas(t)
        frame(ctx, cam, 2, 14)
        after = ctx.read_guides()
        n = ctx.read_denoise_history()[1]
        # its pixels: where the surface seen before fails the documented test against the surface seen now
        moved = (nh._geom_weight(after[0], after[1], before[0], before[1], 6, 0.05) == 0) & (after[0][..., 3] >= 0)
        still = (after[0].view(np.uint32) == before[0].view(np.uint32)).all(-1) & hit
        print("refit: %d pixels changed surface, %d kept theirs" % (int(moved.sum()), int(still.sum())))
        assert moved.sum() > 20 and (n[moved] == 2).all()
        # the rest: the same first hit under the same view is the same-view tap of its own texel (rz = 0, (n . n)^64 > 0): N = 4 + 2
        assert still.sum() > 500 and (n[still] == 6).all()
    finally:
        ctx.close()


# ---- f. the readers of the denoised image ------------------------------------------------------------------------------------------------------

def test_display_meter_and_encode_read_the_history_calls_image(hiplib):
    ctx, sc = make_ctx()
    try:
        for i in range(2):
            frame(ctx, view(sc, W, H, i), 1, i)
        image = ctx.read_denoised()
        ctx.set_display_params(source=capi.DISPLAY_SOURCE_DENOISED)
        ctx.display()
        assert np.array_equal(ctx.read_display_ldr(), ctx.read_denoised_ldr())
        ctx.set_meter_params(source=capi.DISPLAY_SOURCE_DENOISED)
        ctx.meter()
        same_meter(ctx, nm.meter(image, 1), "the history call's image")
        ctx.encode(capi.ENCODE_SOURCE_DENOISED, capi.ENCODE_RGBA16F)
        got = lib_bits(ctx.read_encoded(), capi.ENCODE_RGBA16F)
        want = ne.encode(image.reshape(-1, 4), capi.ENCODE_RGBA16F, 1.0, False)
        assert got.tobytes() == want.tobytes()
    finally:
        ctx.close()


# ---- g. what it gains --------------------------------------------------------------------------------------------------------------------------

def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64)[..., :3] - b) ** 2)))


def test_under_a_moving_camera_the_history_is_closer_to_a_long_render(hiplib):
    """96 x 64, 16 one-frame steps along the camera path; the truth is 4096 frames at the last camera, whose own standard error (the
    percentile of jpt_noise_estimate, and the RMS of sqrt(M2 / (k (k - 1))) over the image) is far below the differences compared"""
    w, h, steps, truth_frames = 96, 64, 16, 4096
    ctx, sc = make_ctx(w, h)
    truth, _ = make_ctx(w, h, history=False)
    try:
        for i in range(steps):
            frame(ctx, view(sc, w, h, i * 0.5), 1, i)
        with_history = ctx.read_denoised()
        raw = ctx.read_accum()
        ctx.set_denoise_history()
        ctx.denoise()
        unguided = ctx.read_denoised()
        truth.set_variance(True)
        truth.set_camera(view(sc, w, h, (steps - 1) * 0.5))
        truth.render(truth_frames, 1000)
        truth.noise_estimate()
        noise = truth.read_noise(histogram=False)[0]
        want = truth.read_accum()[..., :3].astype(np.float64) / truth_frames
        se = float(np.sqrt(np.mean(truth.read_variance()[..., :3].astype(np.float64) / (truth_frames * (truth_frames - 1.0)))))
        r_raw, r_unguided, r_history = rmse(raw, want), rmse(unguided, want), rmse(with_history, want)
        print("RMSE against %d frames (their standard error: RMS %.4g, relative percentile %.4g): raw %.5f, jpt_denoise %.5f, with history %.5f; "
              "ratios %.3f and %.3f" % (truth_frames, se, noise["error"], r_raw, r_unguided, r_history, r_history / r_raw, r_history / r_unguided))
        assert se < 0.1 * min(r_raw - r_history, abs(r_unguided - r_history), r_history)
        assert r_history < r_unguided and r_history < r_raw
    finally:
        ctx.close()
        truth.close()
