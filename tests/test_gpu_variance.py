"""Per-pixel noise on the device (jpt_set_variance, jpt_noise_estimate, jpt_render_converge): the plane of second moments against the
numpy restatement (tests/np_variance.py) bit for bit over the frames the device's own one-frame renders give -- both accumulation
modes, every lighting family, three builders, longer, continued and queued renders, frame groups, other primaries, two ranks --, what
the switch leaves untouched (the pinhole's lost sky cull included), the estimate against the restatement applied to the planes read
back, the convergence loop and the refusals.  33 x 17 or 32 x 32 pixels, 4 bounces."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, partition, scenes

import np_bake as nb
import np_variance as nv
import test_variance_host as tvh
from test_bake_host import atlas
from test_gpu_camera import make_ctx
from test_gpu_transmission import glass_random_scene, np_sum

pytestmark = pytest.mark.gpu

F = np.float32
E_DEVICE, E_STATE = -2, -4   # JPT_E_DEVICE, JPT_E_STATE
ACCUMS = (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8)
TX = capi.MATERIAL_EXT_TRANSMISSION
W, H = 33, 17
# name -> (scene, make_ctx's keywords): the soup stands in front of the sky, so its pinhole renders have a sky cull to lose
CASES = {
    "sky": (glass_random_scene, dict(lighting="sky")),
    "map_mis": (glass_random_scene, dict(lighting="map_mis")),
    "emitters": (scenes.cornell_scene, dict(lighting="emitters")),
    "glass": (glass_random_scene, dict(lighting="sky", flags=TX)),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def differing(got, want):
    """a message naming the first values whose bits differ, or None"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    k = tuple(bad[0])
    return "%d values differ, first %s: %r vs %r" % (len(bad), bad[:3].tolist(), got[k], want[k])


def var_ctx(scene, w=W, h=H, cam=None, **kw):
    """test_gpu_camera.make_ctx with the switch on"""
    ctx = make_ctx(scene, cam, w, h, **kw)
    try:
        ctx.set_variance(True)
    except Exception:
        ctx.close()
        raise
    return ctx


def device_frames(scene, n, w=W, h=H, first=1, prepare=None, **kw):
    """the values of frames first .. first + n - 1 as the accumulation adds them, read from one-frame renders after a reset with the
    switch off: the render path that exists without this feature (for the pinhole, with its sky cull).  [n, H, W, 3]"""
    ctx = make_ctx(scene, None, w, h, **kw)
    try:
        if prepare:
            prepare(ctx)
        out = []
        for f in range(n):
            ctx.accum_reset()
            ctx.render(1, first + f)
            out.append(ctx.read_accum()[..., :3].copy())
        return np.stack(out)
    finally:
        ctx.close()


def check_planes(ctx, frames, ldr8, what, frame_count=1, prev=None):
    """the context's plane and accumulation against numpy over `frames`, continued from prev = (sum, m2); returns the new (sum, m2)"""
    s, m2 = nv.moments(frames, ldr8, frame_count=frame_count, prev_sum=None if prev is None else prev[0], prev_m2=None if prev is None else prev[1])
    why = differing(ctx.read_variance(), nv.plane(m2))
    assert why is None, "%s: the plane: %s" % (what, why)
    why = differing(ctx.read_accum()[..., :3], s)
    assert why is None, "%s: the accumulation: %s" % (what, why)
    return s, m2


# ---- 6. per-frame values from the device's one-frame renders ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("accum", ACCUMS)
def test_the_plane_equals_numpy(hiplib, accum, case):
    make, kw = CASES[case]
    sc = make()
    ldr8 = accum == capi.ACCUM_REF_LDR8
    fr = device_frames(sc, 5, accum=accum, **kw)
    ctx = var_ctx(sc, accum=accum, **kw)
    try:
        ctx.render(5, 1)
        s, m2 = check_planes(ctx, fr, ldr8, case)
        assert differing(s, np_sum(list(fr), ldr8)) is None
        got = ctx.read_variance()
        ptr, nbytes = ctx.device_variance()
        assert ptr and nbytes == got.nbytes and got.shape == (H, W, 4)
        assert (got[..., :3] > 0).any() and (got >= 0).all() and (_bits(got[..., 3]) == 0).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT])
def test_the_plane_equals_numpy_on_three_builders(hiplib, builder):
    sc = glass_random_scene()
    fr = device_frames(sc, 4, builder=builder, accum=capi.ACCUM_REF_LDR8)
    ctx = var_ctx(sc, builder=builder, accum=capi.ACCUM_REF_LDR8)
    try:
        ctx.render(4, 1)
        check_planes(ctx, fr, True, "builder %d" % builder)
    finally:
        ctx.close()


# ---- 7. render lengths and routes ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames16(hiplib):
    """accum -> (scene, the values of frames 1 .. 16 at 33 x 17 from the device's one-frame renders)"""
    sc = glass_random_scene()
    return {accum: (sc, device_frames(sc, 16, accum=accum)) for accum in ACCUMS}


@pytest.mark.parametrize("accum", ACCUMS)
def test_longer_continued_and_queued_renders(hiplib, frames16, accum):
    """3 frames (the per-frame loop), 4 and 8 (the 16-byte loads), each continued by a second render; five one-frame renders in a row;
    then queued renders without a sync between them (the slots' route)"""
    sc, fr = frames16[accum]
    ldr8 = accum == capi.ACCUM_REF_LDR8
    ctx = var_ctx(sc, accum=accum)
    try:
        for n, more in ((3, 3), (4, 4), (8, 3)):
            ctx.accum_reset()
            ctx.render(n, 1)
            first = check_planes(ctx, fr[:n], ldr8, "%d frames" % n)
            ctx.render(more, 1 + n)
            check_planes(ctx, fr[n:n + more], ldr8, "%d + %d frames" % (n, more), frame_count=n + 1, prev=first)
        ctx.accum_reset()
        state = None
        for f in range(5):
            ctx.render(1, 1 + f)
            state = check_planes(ctx, fr[f:f + 1], ldr8, "one-frame render %d" % f, frame_count=f + 1, prev=state)
        assert (_bits(nv.plane(nv.moments(fr[:1], ldr8)[1])) == 0).all()
        ctx.accum_reset()
        state, at = None, 0
        for n in (4, 3, 8, 1):
            ctx.render(n, 1 + at, asynchronous=True)
            state = nv.moments(fr[at:at + n], ldr8, frame_count=at + 1, prev_sum=None if state is None else state[0], prev_m2=None if state is None else state[1])
            at += n
        why = differing(ctx.read_variance(), nv.plane(state[1]))
        assert why is None, "queued: %s" % why
        assert differing(ctx.read_accum()[..., :3], np_sum(list(fr[:16]), ldr8)) is None
        whole = nv.moments(fr, ldr8)
        assert differing(state[1], whole[1]) is None       # (the update does not depend on how the frames are cut into renders)
    finally:
        ctx.close()


@pytest.mark.parametrize("accum", ACCUMS)
def test_five_frames_in_one_render(hiplib, accum):
    """5 frames in one blocking render, continued by 5 more, then both queued: under JPT_GROUPS=3 / 2 (the parent test below) the groups
    are of unequal size and every group's values live in a block of their own, which the kernel must find as wf2_accumulate does"""
    sc = glass_random_scene()
    ldr8 = accum == capi.ACCUM_REF_LDR8
    fr = device_frames(sc, 10, accum=accum)
    ctx = var_ctx(sc, accum=accum)
    try:
        ctx.render(5, 1)
        first = check_planes(ctx, fr[:5], ldr8, "5 frames")
        ctx.render(5, 6)
        both = check_planes(ctx, fr[5:], ldr8, "5 + 5 frames", frame_count=6, prev=first)
        ctx.accum_reset()
        ctx.render(5, 1, asynchronous=True)
        ctx.render(5, 6, asynchronous=True)
        assert differing(ctx.read_variance(), nv.plane(both[1])) is None
    finally:
        ctx.close()


@pytest.mark.parametrize("switch", ["JPT_GROUPS=3", "JPT_GROUPS=2 JPT_PIPE_SLOTS=2"])
def test_frame_groups_give_the_same_plane(hiplib, switch):
    """the switches are read once per process: a fresh child process (tests/test_gpu_bake_dir.py does the same)"""
    env = dict(os.environ)
    for kv in switch.split():
        k, v = kv.split("=")
        env[k] = v
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_five_frames_in_one_render"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout


# ---- 8. other primaries and two ranks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("primary", ["lens", "equirect"])
def test_lens_and_equirect_renders(hiplib, primary):
    sc = glass_random_scene()

    def prepare(ctx):
        if primary == "lens":
            ctx.set_lens(0.05, 6.0)
        else:
            ctx.set_camera_model(capi.CAMERA_EQUIRECT)
    fr = device_frames(sc, 6, w=32, h=32, prepare=prepare)
    ctx = var_ctx(sc, w=32, h=32)
    try:
        prepare(ctx)
        ctx.render(4, 1)
        first = check_planes(ctx, fr[:4], False, primary)
        ctx.render(2, 5)
        check_planes(ctx, fr[4:], False, primary + " continued", frame_count=5, prev=first)
    finally:
        ctx.close()


def test_a_bake_render_with_empty_texels(hiplib):
    """the plane is defined for a texel without a surface (its frames are what the accumulation adds: zeros), and the estimate does not
    count it"""
    sc, p4, n4 = atlas(W, H)
    valid = nb.texel_valid(n4)
    assert 0 < valid.sum() < W * H

    def prepare(ctx):
        ctx.set_bake_texels(p4, n4)
    fr = device_frames(sc, 4, prepare=prepare, accum=capi.ACCUM_REF_LDR8)
    ctx = var_ctx(sc, accum=capi.ACCUM_REF_LDR8)
    try:
        prepare(ctx)
        ctx.render(4, 1)
        check_planes(ctx, fr, True, "bake")
        s, m = ctx.read_accum(), ctx.read_variance()
        assert (m[~valid] == 0).all() and (m[valid][:, :3] > 0).any()
        ctx.noise_estimate()
        (res, hist), tiles = ctx.read_noise(), ctx.read_noise_tiles()
        want = nv.estimate(s, m, 4, valid=valid)
        assert nv.same_result(res, want[0]) is None and np.array_equal(hist, want[1]) and differing(tiles, want[2]) is None
        assert res["counted"] == int(valid.sum()) == int(hist.sum())
        assert nv.estimate(s, m, 4)[0]["counted"] == W * H          # (without the mask the empty texels would count)
    finally:
        ctx.close()


def test_two_partitions_equal_one_context(hiplib):
    sc = glass_random_scene()      # 33 x 17: three 8-row strips, the last one short
    one = var_ctx(sc, accum=capi.ACCUM_REF_LDR8)
    try:
        one.render(4, 1)
        one.render(3, 5)
        want = one.read_variance()
    finally:
        one.close()
    got = np.zeros_like(want)
    seen = np.zeros(H, bool)
    for r in range(2):
        part = var_ctx(sc, accum=capi.ACCUM_REF_LDR8, rank=r, world=2)
        try:
            part.render(4, 1)
            part.render(3, 5)
            rows = partition.rows_of_rank(H, r, 2)
            plane = part.read_variance()
            other = np.setdiff1d(np.arange(H), rows)
            assert plane.shape == (H, W, 4) and (plane[other] == 0).all()       # (scattered to image rows, as read_accum)
            assert part.device_variance()[1] == len(rows) * W * 16
            got[rows] = plane[rows]
            seen[rows] = True
        finally:
            part.close()
    assert seen.all() and np.array_equal(_bits(got), _bits(want)) and (want[..., :3] > 0).any()


# ---- 9. nothing else moves ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accum", ACCUMS)
def test_the_switch_leaves_every_other_image_alone(hiplib, accum):
    sc = glass_random_scene()

    def run(on):
        ctx = make_ctx(sc, None, W, H, accum=accum)
        try:
            if on:
                ctx.set_variance(True)
            else:
                # the pinhole's sky cull is there to be lost: a counted render of the same frames says so
                ctx.render(2, 1, counted=True)
                assert ctx.stats()["sky_culled"] > 0
                ctx.accum_reset()
            ctx.render(2, 1)
            ctx.render(3, 3, asynchronous=True)
            ctx.render(4, 6, asynchronous=True)
            out = ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes()
            if not on:
                plane = np.zeros((H, W, 4), F)
                assert ctx._lib.jpt_read_variance_f32(ctx.h, host._ptr(plane)) == E_STATE
                msg = ctx._lib.jpt_last_error(ctx.h)
                assert b"jpt_read_variance_f32" in msg and b"switched off" in msg, msg
                assert ctx.device_variance() == (None, 0)
            else:
                assert (ctx.read_variance()[..., :3] != 0).any()
            return out
        finally:
            ctx.close()
    off, on = run(False), run(True)
    for a, b in zip(off[:3], on[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert off[3] == on[3]


def test_the_switch_resets_the_accumulation(hiplib):
    sc = glass_random_scene()
    ctx = make_ctx(sc, None, 32, 32)
    try:
        ctx.render(2, 1)
        assert ctx.stats()["frames"] == 2
        ctx.set_variance(False)          # no change of the value: nothing happens
        assert ctx.stats()["frames"] == 2
        ctx.set_variance(True)
        assert ctx.stats()["frames"] == 0
        ctx.render(2, 1)
        two = ctx.read_variance()
        ctx.set_variance(True)           # again no change
        assert ctx.stats()["frames"] == 2 and np.array_equal(_bits(ctx.read_variance()), _bits(two))
        ctx.build_scene(sc, capi.BUILD_SAH)          # the switch survives a commit
        ctx.accum_reset()
        ctx.render(2, 1)
        assert np.array_equal(_bits(ctx.read_variance()), _bits(two))
    finally:
        ctx.close()


# ---- 10. the estimate -----------------------------------------------------------------------------------------------------------------------------

def check_context_estimate(ctx, fc, **params):
    s, m = ctx.read_accum(), ctx.read_variance()
    ctx.set_noise_params(**params)
    ctx.noise_estimate()
    (res, hist), tiles = ctx.read_noise(), ctx.read_noise_tiles()
    want = nv.estimate(s, m, fc, **params)
    why = nv.same_result(res, want[0])
    assert why is None, (fc, why)
    assert np.array_equal(hist, want[1]) and differing(tiles, want[2]) is None, fc
    ptr, nbytes = ctx.device_noise_tiles()
    assert ptr and nbytes == tiles.nbytes
    return res, hist, tiles


@pytest.mark.parametrize("accum", ACCUMS)
def test_the_estimate_equals_numpy_over_the_planes_read_back(hiplib, accum):
    sc = scenes.cornell_scene()
    ctx = var_ctx(sc, accum=accum, lighting="emitters")
    try:
        done = 0
        for more in (1, 1, 2, 12):
            ctx.render(more, 1 + done)
            done += more
            res, hist, tiles = check_context_estimate(ctx, done, threshold=0.125, allowed_permille=250)
            assert bool(res["flags"] & nv.EMPTY) == (done < 2) and res["counted"] == W * H == int(hist.sum())
            # a second call without a render in between: the working sets were left cleared
            again = check_context_estimate(ctx, done, threshold=0.125, allowed_permille=250)
            assert np.array_equal(again[1], hist) and nv.same_result(again[0], res) is None
        assert res["max_error"] > 0 and res["error"] > 0
    finally:
        ctx.close()


def test_device_form_of_the_estimator_equals_the_host_form(hiplib):
    tvh.estimator_cases(0)
    tvh.test_a_threshold_between_two_pixel_values_flips_the_answer(0)


def test_more_tiles_than_one_trip_of_either_kernel(hiplib):
    """1000 x 523: 125 x 66 = 8250 tiles, more than the estimate's 2048 blocks of four take in one trip and 33 trips of the resolve's
    walk over the map, with two tiles left over; a threshold below zero, which every tile (and nothing else) is above"""
    s, m, valid = tvh.planes(1000, 523, 3)
    tvh.spoil(s, m, valid)
    for params in (dict(), dict(threshold=-1.0)):
        res, hist, tiles = tvh.check_estimate(0, s, m, 6, valid, **params)
    assert res["tiles_above"] == tiles.size == 8250 and res["above"] == res["counted"] == int(hist.sum())


# ---- 11. render_converge --------------------------------------------------------------------------------------------------------------------------

def test_render_converge(hiplib):
    sc = scenes.cornell_scene()
    kw = dict(accum=capi.ACCUM_REF_LDR8, lighting="emitters")
    ctx = var_ctx(sc, **kw)
    try:
        # a huge threshold: the first step that reaches two frames
        ctx.set_noise_params(threshold=1e30)
        for per, want in ((1, 2), (2, 2), (3, 3)):
            ctx.accum_reset()
            done, res = ctx.render_converge(per, 9, 1)
            assert done == want and res["flags"] == nv.CONVERGED and ctx.stats()["frames"] == want, (per, done, res)
        # threshold 0 on a scene with an emitter: to max_frames exactly, the last step shortened
        ctx.set_noise_params(threshold=0.0)
        ctx.accum_reset()
        done, res = ctx.render_converge(3, 7, 1)
        assert done == 7 and ctx.stats()["frames"] == 7 and res["flags"] == 0 and res["above"] > 0, (done, res)
        # a middle threshold: where numpy over the device's frames first says converged
        per, most = 2, 16
        fr = device_frames(sc, most, **kw)
        steps = []
        for t in range(per, most + 1, per):
            s, m2 = nv.moments(fr[:t], True)
            steps.append((t, s, nv.plane(m2)))
        chosen = None
        for t, s, m in steps[1:-1]:
            params = dict(threshold=float(nv.estimate(s, m, t)[0]["error"]), allowed_permille=50)
            first = next((u for u, su, mu in steps if nv.estimate(su, mu, u, **params)[0]["flags"] & nv.CONVERGED), None)
            if first is not None and per < first < most:
                chosen = (params, first)
                break
        assert chosen, "no threshold stops these frames strictly between the first step and the last"
        params, first = chosen
        ctx.set_noise_params(**params)
        ctx.accum_reset()
        done, res = ctx.render_converge(per, most, 1)
        want = nv.estimate(*[(s, m) for t, s, m in steps if t == first][0], first, **params)[0]
        assert done == first and nv.same_result(res, want) is None, (done, first, res, want)
        print("render_converge: threshold %.4f stops after %d of %d frames, %d of %d pixels above" % (params["threshold"], done, most, res["above"], res["counted"]))
    finally:
        ctx.close()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_what_is_refused_and_why(hiplib):
    sc = glass_random_scene()
    ctx = make_ctx(sc, None, 32, 32)
    L = ctx._lib
    out = np.zeros((32, 32, 4), F)
    res = capi.NoiseResult()

    def refused(rc, *words):
        assert rc == E_STATE, rc
        msg = L.jpt_last_error(ctx.h)
        for word in words:
            assert word in msg, msg

    def render_refused(*words):
        refused(L.jpt_render(ctx.h, 1, 1), b"jpt_set_variance", *words)
        refused(L.jpt_render_async(ctx.h, 1, 1), b"jpt_set_variance", *words)
    try:
        # the switch off: no plane to read or to estimate from
        ctx.render(2, 1)
        refused(L.jpt_noise_estimate(ctx.h), b"jpt_noise_estimate", b"switched off")
        refused(L.jpt_read_variance_f32(ctx.h, host._ptr(out)), b"jpt_read_variance_f32", b"switched off")
        refused(L.jpt_read_noise(ctx.h, host.C.byref(res), None), b"jpt_read_noise", b"no jpt_noise_estimate")
        refused(L.jpt_render_converge(ctx.h, 1, 2, 1, None, None), b"jpt_render_converge", b"switched off")
        ctx.set_variance(True)
        # no render yet
        refused(L.jpt_noise_estimate(ctx.h), b"jpt_noise_estimate", b"no render with the switch on")
        refused(L.jpt_read_variance_f32(ctx.h, host._ptr(out)), b"jpt_read_variance_f32", b"no render with the switch on")
        assert ctx.device_variance() == (None, 0) and ctx.device_noise_tiles() == (None, 0)
        # the renders it refuses
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        render_refused(b"reference-layout")
        ctx.set_kernel(capi.KERNEL_WAVEFRONT)
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        render_refused(b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_NONE)
        render_refused(b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        render_refused(b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.render(2, 1)
        ctx.read_variance()
        refused(L.jpt_read_noise_tiles_f32(ctx.h, host._ptr(out)), b"jpt_read_noise_tiles_f32", b"no jpt_noise_estimate")
        ctx.noise_estimate()
        assert ctx.read_noise()[0]["counted"] == 32 * 32
        # jpt_meter's refusals
        ctx.set_debug_steps(True)
        refused(L.jpt_noise_estimate(ctx.h), b"jpt_noise_estimate", b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.set_denoising_mode(capi.DENOISE_NONE)
        refused(L.jpt_noise_estimate(ctx.h), b"jpt_noise_estimate", b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        # two ranks: the estimate needs the whole image
        ctx.set_partition(0, 2)
        ctx.render(2, 1)
        refused(L.jpt_noise_estimate(ctx.h), b"jpt_noise_estimate", b"world == 1")
        ctx.set_partition(0, 1)
        # another size: the plane and the estimate of the old one are gone
        ctx.set_params(24, 16, 4, capi.ACCUM_HDR_F32)
        refused(L.jpt_read_variance_f32(ctx.h, host._ptr(out)), b"jpt_read_variance_f32", b"no render with the switch on")
        refused(L.jpt_read_noise(ctx.h, host.C.byref(res), None), b"jpt_read_noise")
        ctx.set_camera(scenes.camera_block(sc.camera, 24, 16))
        ctx.render(3, 1)
        ctx.noise_estimate()
        assert ctx.read_noise()[0]["counted"] == 24 * 16 and ctx.read_noise_tiles().shape == (2, 3)
    finally:
        ctx.close()
    # a host-only context
    hctx = host.Context(-1)
    try:
        assert L.jpt_noise_estimate(hctx.h) == E_DEVICE and b"host-only" in L.jpt_last_error(hctx.h)
        assert L.jpt_set_variance(hctx.h, 1) == E_DEVICE and b"jpt_set_variance" in L.jpt_last_error(hctx.h)
    finally:
        hctx.close()
