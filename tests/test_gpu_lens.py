"""The thin-lens camera on the device (jpt_set_lens): the device's ray generation and whole paths against the numpy restatement
(tests/np_lens.py), the wavefront kernels against the audit kernel under every lighting, what radius 0 leaves unchanged, focus, the
set-aside route, queued renders, counters, ranks, refusals and the post passes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_lens as nl
import np_light_sampling as nls
import np_transmission as ntx
from test_gpu_transmission import glass_random_scene, host_ref, np_sum, sun_map
from test_lens_host import look_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
E_STATE = -4   # JPT_E_STATE
LENS = (0.25, 6.5)   # radius, focus of the whole-path tests
CORNELL_LENS = (0.25, 9.0)   # the box spans 6.8 to 12.8 units down the camera's axis: the focal plane lies inside it


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b)))


def make_ctx(scene, w, h, builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, bounces=4, kernel=capi.KERNEL_WAVEFRONT, lighting="sky", lens=None,
             flags=None, env=None):
    ctx = host.Context(0)
    try:
        ctx.build_scene(scene, builder)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_kernel(kernel)
        ctx.set_camera(scenes.camera_block(scene.camera, w, h))
        if lighting.startswith("map") or env is not None:
            ctx.set_environment(sun_map() if env is None else env)
            if "mis" in lighting:
                ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        if "emitters" in lighting:
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
        if flags is not None:
            ctx.set_material_extensions(flags)
        if lens is not None:
            ctx.set_lens(*lens)
    except Exception:
        ctx.close()
        raise
    return ctx


def soup_scene():
    """a small untextured soup seen from z = 7: triangles from about 4 to 10 units away (the focus of LENS lies among them), sky around"""
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=14, textured=False, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    return sc


# ---- 1. the device's ray generation ---------------------------------------------------------------------------------------------------------

CAMERAS = (look_at((0.3, 0.5, 7.0), (0.0, 0.0, 0.0), fov=70.0), look_at((-4.0, 3.0, -2.5), (1.0, 0.5, 0.0), fov=35.0),
           look_at((2.0, -1.0, 0.5), (2.5, 4.0, -3.0), fov=100.0))


@pytest.mark.parametrize("size", [(32, 32), (33, 17)])
def test_device_ray_generation_equals_numpy(hiplib, size):
    w, h = size
    for k, cd in enumerate(CAMERAS):
        for frame in (1, 77 + k):
            cam = scenes.camera_block(cd, w, h, frame)
            radius, focus = (0.01, 0.2, 0.5)[k], (0.5, 6.0, 20.0)[k]
            for r in (radius, 0.0):
                o, d = host.debug_lens_rays(0, cam, w, h, frame, r, focus)
                _, wo, wd = nl.lens_rays(cam, w, h, r, focus)
                assert np.array_equal(_u32(o).reshape(-1, 3), _u32(wo)) and np.array_equal(_u32(d).reshape(-1, 3), _u32(wd)), (k, frame, r)


# ---- 2. whole paths against numpy, sky lighting -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup_want(oracle):
    sc = soup_scene()
    w = h = 32
    ref = oracle.build_scene(sc)
    cam = scenes.camera_block(sc.camera, w, h).copy()
    frames, depth = [], None
    for f in range(2):
        cam["frame_index"] = 1 + f
        img, depth = nl.trace_frame(ref, cam, w, h, 4, *LENS)
        frames.append(img)
    return sc, frames, depth   # (the depth image is the render's last frame's)


def test_the_soup_shows_sky_and_both_sides_of_the_focus(soup_want):
    sc, frames, depth = soup_want
    cam = scenes.camera_block(sc.camera, 32, 32)
    far, near = F(cam["far"]), F(cam["near"])
    sky = depth == far / (far - near) * (F(1.0) - near / far)
    dist = near / (F(1.0) - depth * (far - near) / far)
    assert sky.mean() >= 0.25, sky.mean()
    assert (dist[~sky] < LENS[1] - 0.5).mean() > 0.05 and (dist[~sky] > LENS[1] + 0.5).mean() > 0.05


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT])
def test_whole_paths_equal_numpy(hiplib, soup_want, builder):
    sc, frames, want_depth = soup_want
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        want = np_sum(frames, accum == capi.ACCUM_REF_LDR8)
        for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
            ctx = make_ctx(sc, 32, 32, builder, accum, 4, kernel, lens=LENS)
            try:
                ctx.render(2, 1)
                got, depth = ctx.read_accum()[..., :3], ctx.read_depth()
            finally:
                ctx.close()
            bad = np.argwhere(~same(got, want).all(axis=-1))
            assert len(bad) == 0, "accum %d kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                accum, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            assert np.array_equal(_u32(depth), _u32(want_depth)), "depth: accum %d kernel %d builder %d" % (accum, kernel, builder)


# ---- 2b. whole paths against numpy under every other lighting, glass included ---------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ["map", "map_mis", "emitters", "map_mis_emitters"])
@pytest.mark.parametrize("which", ["cornell", "glass_random"])
def test_whole_paths_under_every_lighting_equal_numpy(oracle, hiplib, which, lighting):
    """np_transmission.trace_tx with the lens rays of np_lens (the lens does not advance the path's seed): a yardstick that shares no
    lens code with the kernels, where test_wavefront_equals_reference_layout_under_every_lighting compares two kernels that do.
    glass_random is textured and partly transmissive and renders with the flag on; one numpy render per distinct emitter order."""
    glass = which == "glass_random"
    sc = glass_random_scene() if glass else scenes.cornell_scene()
    lens = LENS if glass else CORNELL_LENS
    flags = capi.MATERIAL_EXT_TRANSMISSION if glass else None
    w = h = 32
    bounces, frames = 6, 2
    builders = (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH)
    ref = oracle.build_scene(sc)
    cam = scenes.camera_block(sc.camera, w, h).copy()

    def np_frames(tabs):
        out = []
        for f in range(frames):
            cam["frame_index"] = 1 + f
            out.append(ntx.trace_tx(ref, cam, w, h, bounces, capi.MATERIAL_EXT_TRANSMISSION if glass else 0,
                                    rgb=sun_map() if lighting.startswith("map") else None, env_mis="mis" in lighting,
                                    light_tabs=tabs, textures=sc.textures, lens=lens))
        return np_sum(out, False)

    def device(builder, kernel, ln):
        ctx = make_ctx(sc, w, h, builder, capi.ACCUM_HDR_F32, bounces, kernel, lighting, ln, flags=flags)
        try:
            ctx.render(frames, 1)
            return ctx.read_accum()[..., :3]
        finally:
            ctx.close()

    wants = []   # (emitter order, the sum of the frames)
    for builder in builders:
        tabs = nls.tables(host_ref(sc, builder)) if "emitters" in lighting else None
        key = None if tabs is None else tabs["pairs"].tobytes()
        want = next((x for k, x in wants if k == key), None)
        if want is None:
            want = np_frames(tabs)
            wants.append((key, want))
        for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
            got = device(builder, kernel, lens)
            bad = np.argwhere(~same(got, want).all(axis=-1))
            changed = (~same(got, device(builder, kernel, None))).any(axis=-1).mean()
            print("%s %s builder %d kernel %d: %d pixels differ from numpy; the lens changed %.1f %% of the pixels" % (
                which, lighting, builder, kernel, len(bad), 100.0 * changed))
            assert changed > 0.03, changed
            assert len(bad) == 0, "%s %s kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                which, lighting, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    print("%s %s: %d numpy render(s) for %d builders" % (which, lighting, len(wants), len(builders)))


# ---- 3. every family: the wavefront kernels against the audit kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ["sky", "map", "map_mis", "emitters", "map_mis_emitters", "glass"])
def test_wavefront_equals_reference_layout_under_every_lighting(hiplib, lighting):
    glass = lighting == "glass"
    sc = scenes.glass_cornell_scene() if glass else scenes.cornell_scene()
    w = h = 32
    lens = (0.12, 3.0)
    out = {}
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        for ln in (lens, None):
            ctx = make_ctx(sc, w, h, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, kernel, "map_mis_emitters" if glass else lighting, ln,
                           flags=capi.MATERIAL_EXT_TRANSMISSION if glass else None)
            try:
                ctx.render(2, 1)
                out[kernel, ln is not None] = (ctx.read_accum(), ctx.read_depth())
            finally:
                ctx.close()
    for with_lens in (True, False):
        a, b = out[capi.KERNEL_WAVEFRONT, with_lens], out[capi.KERNEL_REFERENCE_LAYOUT, with_lens]
        assert same(a[0], b[0]).all(), "%s lens %s: %d pixels differ" % (lighting, with_lens, int((~same(a[0], b[0])).any(axis=-1).sum()))
        assert np.array_equal(_u32(a[1]), _u32(b[1]))
    changed = (~same(out[capi.KERNEL_WAVEFRONT, True][0], out[capi.KERNEL_WAVEFRONT, False][0])).any(axis=-1).mean()
    assert changed > 0.03, changed


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_radius_zero_renders_are_unchanged(hiplib, kernel):
    sc = soup_scene()

    def render(steps):
        ctx = make_ctx(sc, 48, 32, accum=capi.ACCUM_REF_LDR8, kernel=kernel)
        try:
            for s in steps:
                ctx.set_lens(*s)
            ctx.render(3, 1)
            return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes()
        finally:
            ctx.close()
    want = render([])
    for steps in ([(0.0, 3.0)], [(0.3, 5.0), (0.0, 5.0)]):
        got = render(steps)
        assert all(np.array_equal(g, w_) for g, w_ in zip(got[:3], want[:3])) and got[3] == want[3], steps
    lens = render([(0.3, 5.0)])
    assert not np.array_equal(lens[0], want[0])
    assert lens[3] == want[3], "jpt_get_workspace_bytes: lens %d, pinhole %d" % (lens[3], want[3])


# ---- 5. focus is sharp, elsewhere is not --------------------------------------------------------------------------------------------------------

FOCUS, QUAD_HALF, APERTURE = 4.0, 0.8, 0.15


def quad_scene(distance):
    """an emissive quad facing the camera `distance` down its axis, the same size on screen whatever the distance, in front of a black
    backdrop that fills the view; the camera at the origin looks down -z"""
    facing = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # the plane's +y normal -> +z
    half = QUAD_HALF * distance / FOCUS
    mats = np.stack([scenes.material(albedo=(0.0, 0.0, 0.0)), scenes.material(albedo=(0.0, 0.0, 0.0), emission=(1.0, 0.75, 0.5))])
    inst = [scenes.Instance(0, scenes.transform12(facing * half, (0.0, 0.0, -distance)), [1]),
            scenes.Instance(0, scenes.transform12(facing * 40.0, (0.0, 0.0, -12.0)), [0])]
    return scenes.Scene("quad", [scenes.plane_mesh(2.0)], inst, mats, scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 0.0)), fov_deg=60.0))


def quad_images(distance):
    out = []
    for lens in (None, (APERTURE, FOCUS)):
        ctx = make_ctx(quad_scene(distance), 48, 48, bounces=0, lens=lens, env=np.zeros((4, 8, 3), F))
        try:
            ctx.set_environment_params(None, 0.0)
            ctx.render(16, 1)
            out.append(ctx.read_accum()[..., :3].astype(np.float64))
        finally:
            ctx.close()
    return out


def test_a_quad_on_the_focal_plane_stays_sharp(hiplib):
    pin, lens = quad_images(FOCUS)
    n = 48
    edge = QUAD_HALF / (FOCUS * np.tan(np.deg2rad(30.0)))            # the outline in NDC, square image
    lo, hi = (1.0 - edge) * n / 2.0, (1.0 + edge) * n / 2.0          # ... and in pixels: the square [lo, hi]^2
    ys, xs = np.mgrid[0:n, 0:n]
    cx, cy = xs + 0.5, ys + 0.5
    inside = (cx >= lo) & (cx <= hi) & (cy >= lo) & (cy <= hi)
    to_side = np.minimum(np.minimum(np.abs(cx - lo), np.abs(cx - hi)), np.minimum(np.abs(cy - lo), np.abs(cy - hi)))
    outside = np.hypot(np.maximum(np.maximum(lo - cx, cx - hi), 0.0), np.maximum(np.maximum(lo - cy, cy - hi), 0.0))
    dist = np.where(inside, to_side, outside)                           # of the pixel centre from the outline
    differ = (pin != lens).any(axis=-1)
    assert (pin > 0).any() and not (differ & (dist > 1.5)).any(), "pixels that differ away from the outline: %s" % np.argwhere(differ & (dist > 1.5))[:5].tolist()
    assert abs(lens.sum() - pin.sum()) <= 0.1 * pin.sum()


def test_a_quad_off_the_focal_plane_is_blurred_and_keeps_its_energy(hiplib):
    pin, lens = quad_images(FOCUS / 2.0)
    lit_pin, lit_lens = int((pin > 0).any(axis=-1).sum()), int((lens > 0).any(axis=-1).sum())
    print("lit pixels: pinhole %d, lens %d; sums %.3f, %.3f" % (lit_pin, lit_lens, pin.sum(), lens.sum()))
    assert lit_lens > lit_pin
    assert abs(lens.sum() - pin.sum()) <= 0.1 * pin.sum()


# ---- 6. the set-aside route ---------------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from gdpathtracing_amd import capi
import test_gpu_lens as t
ctx = t.make_ctx(t.tied_scene(), 96, 64, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, capi.KERNEL_WAVEFRONT, lens=t.TIED_LENS)
ctx.render(2, 1)
np.save(sys.argv[2], ctx.read_accum())
st = ctx.stats()
ctx.close()
print(json.dumps({"set_aside": st["set_aside"], "dropped": st["set_aside_dropped"]}))
"""
TIED_LENS = (0.2, 6.0)


def tied_scene():
    """the fuzz soup with coincident triangles (exact distance ties) and the cracks of its reference tree"""
    return scenes.random_scene(4, coincident=True, textured=False)


def test_set_aside_paths_of_a_lens_render_are_finished_exactly(hiplib, tmp_path):
    ctx = make_ctx(tied_scene(), 96, 64, capi.BUILD_REFERENCE_EXACT, capi.ACCUM_HDR_F32, 4, capi.KERNEL_WAVEFRONT, lens=TIED_LENS)
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


# ---- 7. queued renders, counters, ranks ---------------------------------------------------------------------------------------------------------

def test_queued_renders_keep_the_lens_of_their_call(hiplib):
    """four renders that alternate between a lens and the pinhole, the lens set between them: queued without a sync they give what
    the same four calls give blocking -- each render took the lens of its own call by value"""
    sc = soup_scene()
    w, h = 160, 100
    lenses = [(0.3, 6.0), (0.0, 1.0), (0.1, 9.0), (0.0, 1.0)]

    def run(asynchronous, which):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8)
        try:
            for k, ln in enumerate(which):
                ctx.set_lens(*ln)
                ctx.render(2, 5 + 2 * k, asynchronous=asynchronous)
            return ctx.read_accum(), ctx.read_ldr()
        finally:
            ctx.close()
    want, got = run(False, lenses), run(True, lenses)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for other in ([(0.0, 1.0)] * 4, [lenses[0]] * 4, lenses[::-1]):   # (and the lens of each call matters)
        assert not np.array_equal(run(True, other)[0], want[0])


def test_a_counted_lens_render_culls_nothing(hiplib):
    sc = soup_scene()
    culled = {}
    for ln in (None, LENS):
        ctx = make_ctx(sc, 64, 64, lens=ln)
        try:
            ctx.render(2, 1, counted=True)
            culled[ln is not None] = ctx.stats()["sky_culled"]
        finally:
            ctx.close()
    assert culled[False] > 0 and culled[True] == 0, culled


def test_multi_two_ranks_equals_one_context(hiplib):
    sc = soup_scene()
    w, h = 160, 104
    one = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, lens=LENS)
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc)
        m.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
        m.set_camera(scenes.camera_block(sc.camera, w, h))
        m.set_lens(*LENS)
        one.render(4, 1)
        m.render(4, 1)
        assert np.array_equal(m.read_accum(), one.read_accum())
        assert np.array_equal(m.read_ldr(), one.read_ldr())
    finally:
        m.close()
        one.close()


# ---- 8. refusals and the post passes --------------------------------------------------------------------------------------------------------------

def test_temporal_mode_refuses_a_lens_and_debug_steps_ignores_it(hiplib):
    sc = soup_scene()
    ctx = make_ctx(sc, 32, 32, lens=LENS)
    try:
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        rc = ctx._lib.jpt_render(ctx.h, 1, 1)
        assert rc == E_STATE and b"lens" in ctx._lib.jpt_last_error(ctx.h).lower()
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        bad = scenes.camera_block(sc.camera, 32, 32).copy()
        bad["ivp"] = 0.0
        ctx.set_camera(bad)
        assert ctx._lib.jpt_render(ctx.h, 1, 1) == E_STATE and b"not finite" in ctx._lib.jpt_last_error(ctx.h)
    finally:
        ctx.close()
    steps = []
    for ln in (None, LENS):
        ctx = make_ctx(sc, 32, 32, lens=ln)
        try:
            ctx.set_debug_steps(True)
            ctx.render(1, 1)
            steps.append(ctx.read_accum())
        finally:
            ctx.close()
    assert np.array_equal(steps[0], steps[1]) and (steps[0][..., :3] > 0).any()


def test_denoise_and_display_run_on_a_lens_render(hiplib):
    w, h = 96, 64
    ctx = make_ctx(scenes.cornell_scene(), w, h, lens=(0.1, 3.0))
    try:
        ctx.render(4, 1)
        ctx.denoise()
        den = ctx.read_denoised()
        assert den.shape[:2] == (h, w) and np.isfinite(den).all()
        ctx.display()
        assert ctx.read_display_ldr().shape[:2] == (h, w)
    finally:
        ctx.close()
