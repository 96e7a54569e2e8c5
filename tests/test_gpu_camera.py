"""The camera models on the device (jpt_set_camera_model): the device's ray generation and whole paths against the numpy
restatement (tests/np_camera.py), the wavefront kernels against the audit kernel under every lighting, a constant map seen through
the panorama, what PINHOLE leaves unchanged, counters, queued renders, the set-aside route, ranks, the guides, picking, refusals
and the post passes.  32 x 32 or 33 x 17 pixels, 2 frames, 4 bounces unless a test says why not."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, partition, scenes

import np_camera as nc
import np_denoise as nd
from test_camera_host import camera_blocks, soup_scene, soup_view
from test_gpu_transmission import glass_random_scene, np_sum, sun_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
E_STATE = -4   # JPT_E_STATE
MODELS = (capi.CAMERA_PROJECTIVE, capi.CAMERA_EQUIRECT)
SIZE = {capi.CAMERA_PROJECTIVE: (33, 17), capi.CAMERA_EQUIRECT: (32, 32)}   # the whole-path tests: each model at one of the two sizes


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b)))


def records_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def make_ctx(scene, cam, w, h, builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, bounces=4, kernel=capi.KERNEL_WAVEFRONT, lighting="sky", model=None,
             flags=None, env=None, rank=0, world=1):
    """a context on device 0 with `cam` (a camera block; None: the scene's perspective camera) and, unless None, the model set"""
    ctx = host.Context(0)
    try:
        ctx.build_scene(scene, builder)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_kernel(kernel)
        if world != 1:
            ctx.set_partition(rank, world)
        ctx.set_camera(scenes.camera_block(scene.camera, w, h) if cam is None else cam)
        if lighting.startswith("map") or env is not None:
            ctx.set_environment(sun_map() if env is None else env)
            if "mis" in lighting:
                ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        if "emitters" in lighting:
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
        if flags is not None:
            ctx.set_material_extensions(flags)
        if model is not None:
            ctx.set_camera_model(model)
    except Exception:
        ctx.close()
        raise
    return ctx


# ---- 1. the device's ray generation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(32, 32), (33, 17)])
@pytest.mark.parametrize("model", MODELS)
def test_device_ray_generation_equals_numpy(hiplib, model, size):
    w, h = size
    for frame in (1, 78):
        for name, cam in camera_blocks(w, h, frame):
            o, d = host.debug_camera_rays(0, cam, w, h, frame, model)
            _, wo, wd = nc.camera_rays(cam, w, h, model)
            assert np.array_equal(_u32(o).reshape(-1, 3), _u32(wo)) and np.array_equal(_u32(d).reshape(-1, 3), _u32(wd)), (name, frame)
    cam = camera_blocks(w, h, 5)[0][1]
    o, d = host.debug_camera_rays(0, cam, w, h, 5, capi.CAMERA_PINHOLE)
    lo, ld = host.debug_lens_rays(0, cam, w, h, 5, 0.0, 1.0)
    assert np.array_equal(_u32(o), _u32(lo)) and np.array_equal(_u32(d), _u32(ld))


# ---- 2. whole paths against numpy -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup_want(oracle):
    """per model: (scene, camera block, the two frames under the sky, the last frame's depth, the two frames under sun_map())"""
    out = {}
    for model in MODELS:
        w, h = SIZE[model]
        sc, cam = soup_view(model, w, h)
        ref = oracle.build_scene(sc)
        cam = cam.copy()
        sky, env, depth = [], [], None
        for f in range(2):
            cam["frame_index"] = 1 + f
            img, depth = nc.trace_frame(ref, cam, w, h, 4, model)
            sky.append(img)
            env.append(nc.trace_frame(ref, cam, w, h, 4, model, rgb=sun_map())[0])
        cam["frame_index"] = 0
        out[model] = (sc, cam, sky, depth, env)
    return out


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT])
@pytest.mark.parametrize("model", MODELS)
def test_whole_paths_equal_numpy(hiplib, soup_want, model, builder):
    sc, cam, frames, want_depth, _ = soup_want[model]
    w, h = SIZE[model]
    far, near = F(cam["far"]), F(cam["near"])
    sky = want_depth == far / (far - near) * (F(1.0) - near / far)
    assert 0.1 <= sky.mean() <= 0.9, sky.mean()   # (test_camera_host asserts the view's mix; this is the frame compared here)
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        want = np_sum(frames, accum == capi.ACCUM_REF_LDR8)
        for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
            ctx = make_ctx(sc, cam, w, h, builder, accum, 4, kernel, model=model)
            try:
                ctx.render(2, 1)
                got, depth = ctx.read_accum()[..., :3], ctx.read_depth()
            finally:
                ctx.close()
            bad = np.argwhere(~same(got, want).all(axis=-1))
            assert len(bad) == 0, "model %d accum %d kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                model, accum, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            assert np.array_equal(_u32(depth), _u32(want_depth)), "depth: model %d accum %d kernel %d builder %d" % (model, accum, kernel, builder)


@pytest.mark.parametrize("model", MODELS)
def test_whole_paths_under_a_map_equal_numpy(hiplib, soup_want, model):
    """wf2_primary_env_cam: every primary walk is queued, and the misses look the map up (np_env.env_radiance)"""
    sc, cam, _, _, frames = soup_want[model]
    w, h = SIZE[model]
    want = np_sum(frames, False)
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        ctx = make_ctx(sc, cam, w, h, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, kernel, "map", model)
        try:
            ctx.render(2, 1)
            got = ctx.read_accum()[..., :3]
        finally:
            ctx.close()
        bad = np.argwhere(~same(got, want).all(axis=-1))
        assert len(bad) == 0, "model %d kernel %d: %d pixels differ, first %s: %s vs %s" % (
            model, kernel, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 3. every family: the wavefront kernels against the audit kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ["map", "map_mis", "emitters", "map_mis_emitters", "glass"])
@pytest.mark.parametrize("model", MODELS)
def test_wavefront_equals_reference_layout_under_every_lighting(hiplib, model, lighting):
    """Cornell through its own perspective matrix (PROJECTIVE: the pinhole's directions from the near plane; EQUIRECT: the box all
    around); glass: the partly transmissive soup under every light"""
    glass = lighting == "glass"
    sc = glass_random_scene() if glass else scenes.cornell_scene()
    w, h = SIZE[model]
    out = {}
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        for m in (model, None):
            ctx = make_ctx(sc, None, w, h, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, kernel, "map_mis_emitters" if glass else lighting, m,
                           flags=capi.MATERIAL_EXT_TRANSMISSION if glass else None)
            try:
                ctx.render(2, 1)
                out[kernel, m is not None] = (ctx.read_accum(), ctx.read_depth())
            finally:
                ctx.close()
    for with_model in (True, False):
        a, b = out[capi.KERNEL_WAVEFRONT, with_model], out[capi.KERNEL_REFERENCE_LAYOUT, with_model]
        assert same(a[0], b[0]).all(), "%s model %s: %d pixels differ" % (lighting, with_model, int((~same(a[0], b[0])).any(axis=-1).sum()))
        assert np.array_equal(_u32(a[1]), _u32(b[1]))
    changed = (~same(out[capi.KERNEL_WAVEFRONT, True][0], out[capi.KERNEL_WAVEFRONT, False][0])).any(axis=-1).mean()
    assert changed > 0.03, changed
    assert (out[capi.KERNEL_WAVEFRONT, True][0][..., :3] > 0).any()


# ---- 4. a constant map through the panorama -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_a_constant_map_gives_a_constant_panorama(hiplib, kernel):
    base = scenes.cornell_scene()
    sc = scenes.Scene("empty", [], [], base.materials, base.camera)
    for w, h in ((32, 32), (33, 17)):
        ctx = make_ctx(sc, None, w, h, model=capi.CAMERA_EQUIRECT, kernel=kernel, env=np.full((4, 8, 3), 0.5, F))
        try:
            ctx.render(2, 1)
            got = ctx.read_accum()
        finally:
            ctx.close()
        assert (got[..., :3] == F(1.0)).all(), np.unique(got[..., :3])


# ---- 5. PINHOLE means the default --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_pinhole_renders_are_the_default_bits(hiplib, kernel):
    sc = soup_scene()

    def render(steps):
        """`steps`: models set one after another, a render after each but the last discarded by a reset"""
        ctx = make_ctx(sc, None, 48, 32, accum=capi.ACCUM_REF_LDR8, kernel=kernel)
        try:
            for k, m in enumerate(steps):
                ctx.set_camera_model(m)
                if k + 1 < len(steps):
                    ctx.render(1, 1)
                    ctx.accum_reset()
            ctx.render(3, 1)
            return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes()
        finally:
            ctx.close()
    want = render([])
    for steps in ([capi.CAMERA_PINHOLE], [capi.CAMERA_PROJECTIVE, capi.CAMERA_PINHOLE], [capi.CAMERA_EQUIRECT, capi.CAMERA_PROJECTIVE, capi.CAMERA_PINHOLE]):
        got = render(steps)
        assert all(np.array_equal(g, w_) for g, w_ in zip(got[:3], want[:3])) and got[3] == want[3], steps
    for m in MODELS:
        other = render([m])
        assert not np.array_equal(other[0], want[0])
        assert other[3] == want[3], "jpt_get_workspace_bytes: model %d %d, pinhole %d" % (m, other[3], want[3])


# ---- 6. counters and queued renders -------------------------------------------------------------------------------------------------------------

def test_a_counted_render_under_a_model_culls_nothing(hiplib):
    sc = soup_scene()
    culled = {}
    for m in (None,) + MODELS:
        ctx = make_ctx(sc, None, 64, 64, model=m)
        try:
            ctx.render(2, 1, counted=True)
            st = ctx.stats()
            culled[m] = st["sky_culled"]
            assert st["rays"] >= 64 * 64 * 2
        finally:
            ctx.close()
    assert culled[None] > 0 and culled[capi.CAMERA_PROJECTIVE] == 0 and culled[capi.CAMERA_EQUIRECT] == 0, culled


def test_queued_renders_keep_the_model_of_their_call(hiplib):
    """three renders with three models, the model set between them: queued without a sync they give what the same calls give
    blocking -- each render took the model of its own call by value"""
    sc = soup_scene()
    w, h = 96, 64
    order = [capi.CAMERA_PROJECTIVE, capi.CAMERA_PINHOLE, capi.CAMERA_EQUIRECT]

    def run(asynchronous, which):
        ctx = make_ctx(sc, None, w, h, accum=capi.ACCUM_REF_LDR8)
        try:
            for k, m in enumerate(which):
                ctx.set_camera_model(m)
                ctx.render(2, 5 + 2 * k, asynchronous=asynchronous)
            return ctx.read_accum(), ctx.read_ldr()
        finally:
            ctx.close()
    want, got = run(False, order), run(True, order)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for other in ([capi.CAMERA_PINHOLE] * 3, [order[0]] * 3, order[::-1]):   # (and the model of each call matters)
        assert not np.array_equal(run(True, other)[0], want[0])


# ---- 7. the set-aside route ---------------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from gdpathtracing_amd import capi
import test_gpu_camera as t
ctx = t.make_ctx(t.tied_scene(), None, 96, 64, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, capi.KERNEL_WAVEFRONT, model=capi.CAMERA_PROJECTIVE)
ctx.render(2, 1)
np.save(sys.argv[2], ctx.read_accum())
st = ctx.stats()
ctx.close()
print(json.dumps({"set_aside": st["set_aside"], "dropped": st["set_aside_dropped"]}))
"""


def tied_scene():
    """test_gpu_lens.tied_scene: the fuzz soup with coincident triangles (exact distance ties) and the cracks of its reference tree"""
    return scenes.random_scene(4, coincident=True, textured=False)


def test_set_aside_paths_of_a_projective_render_are_finished_exactly(hiplib, tmp_path):
    """(a process of its own: the set-aside capacity is read from the environment once)"""
    ctx = make_ctx(tied_scene(), None, 96, 64, capi.BUILD_REFERENCE_EXACT, capi.ACCUM_HDR_F32, 4, capi.KERNEL_WAVEFRONT, model=capi.CAMERA_PROJECTIVE)
    try:
        ctx.render(2, 1)
        want = ctx.read_accum()
    finally:
        ctx.close()
    env = dict(os.environ)
    env["JPT_SET_ASIDE_CAP"] = "1000000"
    path = str(tmp_path / "sah.npy")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads(r.stdout.strip().splitlines()[-1])
    print("set aside / dropped:", st)
    assert st["set_aside"] > 0 and st["dropped"] == 0, st
    got = np.load(path)
    assert same(got, want).all(), "%d pixels differ" % int((~same(got, want)).any(axis=-1).sum())


# ---- 8. ranks -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
def test_two_partitions_and_multi_equal_one_context(hiplib, model):
    w, h = 96, 40
    sc, cam = soup_view(model, w, h)
    one = make_ctx(sc, cam, w, h, accum=capi.ACCUM_REF_LDR8, model=model)
    m = host.MultiContext([0, 0])
    try:
        one.render(4, 1)
        want, want_ldr = one.read_accum(), one.read_ldr()
        got = np.zeros_like(want)
        for r in range(2):
            part = make_ctx(sc, cam, w, h, accum=capi.ACCUM_REF_LDR8, model=model, rank=r, world=2)
            try:
                part.render(4, 1)
                rows = partition.rows_of_rank(h, r, 2)
                got[rows] = part.read_accum()[rows]
            finally:
                part.close()
        assert np.array_equal(got, want)
        m.build_scene(sc)
        m.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
        m.set_camera(cam)
        m.set_camera_model(model)
        m.render(4, 1)
        assert np.array_equal(m.read_accum(), want)
        assert np.array_equal(m.read_ldr(), want_ldr)
    finally:
        m.close()
        one.close()


# ---- 9. the guides, the post passes and picking ---------------------------------------------------------------------------------------------------

def test_guides_of_an_orthographic_render_are_the_models_centre_rays(oracle, hiplib, monkeypatch):
    """np_denoise's guides with np_camera's centre rays in place of the pinhole's: position (and the distance from the ray's own
    origin) and normal as bits, ties as guides_match treats them; then jpt_denoise, jpt_display and jpt_meter on the render"""
    model = capi.CAMERA_PROJECTIVE
    w, h = 33, 17
    sc, cam = soup_view(model, w, h)
    ref = oracle.build_scene(sc)
    ctx = make_ctx(sc, cam, w, h, model=model)
    try:
        ctx.render(2, 1)
        ctx.denoise()
        guides = ctx.read_guides()
        den = ctx.read_denoised()
        ctx.display()
        ldr = ctx.read_display_ldr()
        ctx.meter()
        res, hist = ctx.read_meter()
        ctx.set_camera_model(capi.CAMERA_PINHOLE)
        ctx.denoise()
        pinhole_guides = ctx.read_guides()
    finally:
        ctx.close()
    monkeypatch.setattr(nd, "centre_rays", lambda c, ww, hh: nc.centre_rays(c, ww, hh, model))
    matched, best = nd.guides_match(ref, cam, w, h, *guides)
    hit = best < F(1e9)
    assert matched.all(), "%d of %d guide texels differ" % (int((~matched).sum()), len(matched))
    assert 0.25 <= hit.mean() <= 0.75, hit.mean()
    assert np.array_equal(guides[0][..., 3].reshape(-1) >= 0, hit)
    assert not np.array_equal(_u32(guides[0]), _u32(pinhole_guides[0]))   # (the pinhole's guides are another view's)
    assert den.shape[:2] == (h, w) and np.isfinite(den).all() and ldr.shape[:2] == (h, w) and (ldr[..., :3] > 0).any()
    assert int(hist.sum()) > 0 and np.isfinite(res["exposure"])


@pytest.mark.parametrize("model", MODELS)
def test_pixel_queries_follow_the_model(hiplib, model):
    w, h = SIZE[model]
    sc, cam = soup_view(model, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(3)
    xy = np.concatenate([np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=1),
                         rng.uniform((-2.0, -2.0), (w + 2.0, h + 2.0), size=(300, 2))]).astype(F)   # centres, then positions on and off the screen
    o, d = nc.raster_rays(cam, w, h, model, xy[:, 0], xy[:, 1])
    ctx = make_ctx(sc, cam, w, h, model=model)
    try:
        got = ctx.query_pixels(xy)
        want, _ = ctx.query_rays(o, d)
        ctx.set_camera_model(capi.CAMERA_PINHOLE)
        pinhole = ctx.query_pixels(xy)
    finally:
        ctx.close()
    valid = (got["flags"] & capi.HIT_VALID) != 0
    assert records_equal(got, want)
    assert 0.1 <= valid[:w * h].mean() <= 0.9, valid[:w * h].mean()
    assert not records_equal(got, pinhole)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_lens_and_temporal_mode_are_refused_and_debug_steps_ignores_the_model(hiplib):
    sc = soup_scene()
    for model in MODELS:
        ctx = make_ctx(sc, None, 32, 32, model=model)
        try:
            ctx.set_lens(0.25, 6.5)
            assert ctx._lib.jpt_render(ctx.h, 1, 1) == E_STATE and b"lens" in ctx._lib.jpt_last_error(ctx.h).lower()
            assert ctx._lib.jpt_render_async(ctx.h, 1, 1) == E_STATE
            ctx.set_lens(0.0, 1.0)
            ctx.render(1, 1)
            ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
            assert ctx._lib.jpt_render(ctx.h, 1, 1) == E_STATE and b"temporal" in ctx._lib.jpt_last_error(ctx.h).lower()
            ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
            bad = scenes.camera_block(sc.camera, 32, 32).copy()
            ivp = bad["ivp"].copy()
            ivp.reshape(-1)[:] = 0.0 if model == capi.CAMERA_EQUIRECT else np.nan
            bad["ivp"] = ivp
            ctx.set_camera(bad)
            assert ctx._lib.jpt_render(ctx.h, 1, 1) == E_STATE and b"not finite" in ctx._lib.jpt_last_error(ctx.h)
            ctx.set_camera_model(capi.CAMERA_PINHOLE)
            ctx.set_camera(scenes.camera_block(sc.camera, 32, 32))
            ctx.render(1, 2)   # (and the context renders on)
        finally:
            ctx.close()
    steps = []
    for m in (None,) + MODELS:
        ctx = make_ctx(sc, None, 32, 32, model=m)
        try:
            ctx.set_debug_steps(True)
            ctx.render(1, 1)
            steps.append(ctx.read_accum())
        finally:
            ctx.close()
    assert np.array_equal(steps[0], steps[1]) and np.array_equal(steps[0], steps[2]) and (steps[0][..., :3] > 0).any()
