"""Transparent materials on the device (jpt_set_material_extensions, JPT_MATERIAL_EXT_TRANSMISSION): the dielectric event against
numpy, whole paths of the *_tx kernels against the numpy path tracer (tests/np_transmission.py) under every lighting, what the flag
leaves unchanged, a furnace, the set-aside route, and the flag across queued renders, ranks, a TLAS refit and the post passes."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_light_sampling as nls
import np_transmission as ntx
from test_transmission_host import corner_cases, random_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TX = capi.MATERIAL_EXT_TRANSMISSION
LIGHTINGS = ("sky", "map", "map_mis", "emitters", "map_mis_emitters")


def sun_map(h=32, w=64):
    v, u = np.mgrid[0:h, 0:w]
    rgb = np.stack([0.6 + 0.4 * u / w, 0.7 + 0.3 * (1.0 - v / h), 0.9 + 0.1 * np.cos(4.0 * u / w)], axis=-1) * 0.2
    rgb[h // 6:h // 6 + 3, w // 3:w // 3 + 4] = (20.0, 18.0, 15.0)
    return rgb.astype(F)


def make_ctx(scene, w, h, builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, bounces=6, kernel=capi.KERNEL_WAVEFRONT, lighting="sky",
             flags=TX, env=None):
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
    except Exception:
        ctx.close()
        raise
    return ctx


class _Ref:
    """the context's own reference-layout arrays, as np_path reads them"""
    def __init__(self, ctx):
        self.tri_geom = ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY)
        self.tri_data = ctx.reference_buffer(capi.BUF_TRI_DATA, wire.TRI_DATA)
        self.materials = ctx.reference_buffer(capi.BUF_MATERIALS, wire.MATERIAL)
        self.bvh_nodes = ctx.reference_buffer(capi.BUF_BVH_NODES, wire.BVH_NODE)
        self.instances = ctx.reference_buffer(capi.BUF_INSTANCES, wire.BLAS_INSTANCE)


def host_ref(scene, builder):
    ctx = host.Context(-1)
    try:
        ctx.build_scene(scene, builder)
        return _Ref(ctx)
    finally:
        ctx.close()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def glass_random_scene():
    """a small soup, three of its materials transmissive (one fully, one partly, one textured)"""
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=14, textured=True, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    used = sorted({m for i in sc.instances for m in i.material_ids})
    textured = [m for m in used if sc.materials["albedo_texture_index"][m] >= 0]
    assert textured, "the soup has no textured material in use"
    pick = [textured[0]] + [m for m in used if m != textured[0]][:2]
    return scenes.with_transmissive_materials(sc, pick, transmission=[0.8, 1.0, 0.45][:len(pick)], ior=[1.33, 1.5, 2.0][:len(pick)])


# ---- 1. the device function -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cases", ["random", "corners"])
def test_device_dielectric_event_equals_numpy(hiplib, cases):
    nrm, v, ior, front, xi = random_cases() if cases == "random" else corner_cases()
    d, fres, ev = host.debug_dielectric(0, nrm, v, ior, front, xi)
    wd, wf, we = ntx.dielectric_event(nrm, v, ior, front, xi)
    assert np.array_equal(ev, we) and np.array_equal(_u32(fres), _u32(wf)) and np.array_equal(_u32(d), _u32(wd))


# ---- 2. whole paths against numpy ---------------------------------------------------------------------------------------------------

def np_frames(ref, scene, w, h, frames, bounces, lighting, tabs):
    cam = scenes.camera_block(scene.camera, w, h).copy()
    out = []
    for f in range(frames):
        cam["frame_index"] = 1 + f
        out.append(ntx.trace_tx(ref, cam, w, h, bounces, TX, rgb=sun_map() if lighting.startswith("map") else None,
                                env_mis="mis" in lighting, light_tabs=tabs if "emitters" in lighting else None, textures=scene.textures))
    return out


def np_sum(frames, ldr8):
    acc = None
    for cur in frames:
        if ldr8:
            cur = (np.floor(np.clip(cur, F(0), F(1)) * F(255) + F(0.5)).astype(F) / F(255)).astype(F)
        acc = cur if acc is None else (cur + acc).astype(F)
    return acc


@pytest.mark.parametrize("lighting", LIGHTINGS)
@pytest.mark.parametrize("which", ["glass_cornell", "random"])
def test_whole_paths_equal_numpy(oracle, hiplib, which, lighting):
    sc = scenes.glass_cornell_scene() if which == "glass_cornell" else glass_random_scene()
    w = h = 32
    bounces, frames = 6, 2
    builders = (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT)
    ref = oracle.build_scene(sc)
    tabs = {b: nls.tables(host_ref(sc, b)) for b in builders} if "emitters" in lighting else {b: None for b in builders}
    wants = []   # (emitter order, the frames): one numpy render per distinct emitter order
    for builder in builders:
        t = tabs[builder]
        key = None if t is None else t["pairs"].tobytes()
        fr = next((f for k, f in wants if k == key), None)
        if fr is None:
            fr = np_frames(ref, sc, w, h, frames, bounces, lighting, t)
            wants.append((key, fr))
        for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
            want = np_sum(fr, accum == capi.ACCUM_REF_LDR8)
            for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
                ctx = make_ctx(sc, w, h, builder, accum, bounces, kernel, lighting)
                try:
                    ctx.render(frames, 1)
                    got = ctx.read_accum()[..., :3]
                finally:
                    ctx.close()
                bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=-1))
                assert len(bad) == 0, "%s %s accum %d kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                    which, lighting, accum, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_glass_changes_the_image(hiplib):
    sc = scenes.glass_cornell_scene()
    out = []
    for flags in (capi.MATERIAL_EXT_NONE, TX):
        ctx = make_ctx(sc, 48, 48, flags=flags)
        try:
            ctx.render(2, 1)
            out.append(ctx.read_accum())
        finally:
            ctx.close()
    assert (out[0] != out[1]).any(axis=-1).mean() > 0.03


# ---- 3. unchanged when off ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
@pytest.mark.parametrize("lighting", ["sky", "map_mis_emitters"])
def test_renders_without_a_transmissive_material_are_unchanged(hiplib, kernel, lighting):
    base = scenes.cornell_scene()
    rng = np.random.default_rng(5)
    garbage = copy.deepcopy(base)
    garbage.materials = garbage.materials.copy()
    garbage.materials["padding"] = rng.standard_normal(garbage.materials["padding"].shape).astype(F) * F(1e3)
    garbage.materials["padding"][0] = np.array([np.nan, np.inf, -np.inf, 1.0, 0.5], F)
    dull = copy.deepcopy(base)
    dull.materials = dull.materials.copy()
    dull.materials["padding"][:, 0] = np.resize(np.array([0.0, -0.0, -1.0, np.nan, -np.inf], F), len(dull.materials))
    dull.materials["padding"][:, 1] = rng.uniform(-2, 9, len(dull.materials)).astype(F)

    def render(scene, steps):
        ctx = make_ctx(scene, 64, 48, accum=capi.ACCUM_REF_LDR8, kernel=kernel, lighting=lighting, flags=None)
        try:
            for f in steps:
                ctx.set_material_extensions(f)
            ctx.render(3, 1)
            return ctx.read_accum(), ctx.read_ldr()
        finally:
            ctx.close()
    want = render(base, [])
    for what, scene, steps in (("flag off, garbage padding", garbage, []), ("flag off explicitly, garbage padding", garbage, [capi.MATERIAL_EXT_NONE]),
                               ("flag on, no transmission > 0", dull, [TX]), ("flag on then off", scenes.glass_cornell_scene(), [TX, capi.MATERIAL_EXT_NONE]),
                               ("flag on then off, garbage padding", garbage, [TX, capi.MATERIAL_EXT_NONE])):
        if "then off" in what and scene is not garbage:
            # (the glass scene's extra material does not change the flag-less render: the block is opaque white)
            ref_img = render(scene, [])
        else:
            ref_img = want
        got = render(scene, steps)
        assert np.array_equal(got[0], ref_img[0]) and np.array_equal(got[1], ref_img[1]), what


# ---- 4. the furnace -----------------------------------------------------------------------------------------------------------------------

def furnace_scene(ior):
    """one closed convex glass box (transmission 1, albedo 1) in front of the camera, nothing else"""
    mats = np.stack([scenes.material(), scenes.material(transmission=1.0, ior=ior)])
    inst = [scenes.Instance(0, scenes.transform12(scenes.rot_y(33.0) @ np.diag([1.0, 1.3, 0.8]), (0.1, 0.0, 0.0)), [1])]
    return scenes.Scene("furnace", [scenes.box_mesh(2.0, 2.0, 2.0)], inst, mats, scenes.CameraDesc(scenes.transform12(None, (0.0, 0.3, 5.0)), fov_deg=60.0))


GREY = np.full((4, 8, 3), 0.5, F)


@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_furnace_with_ior_one_is_exact(hiplib, kernel):
    """ior 1: F is 0 to rounding and the refracted direction is the ray's own; every path leaves the box after two vertices with
    throughput exactly 1 (tint 1) and finds the constant map: every pixel's sum is exactly 0.5 per frame."""
    frames = 4
    ctx = make_ctx(furnace_scene(1.0), 64, 64, bounces=4, kernel=kernel, lighting="map", env=GREY)
    try:
        ctx.render(frames, 1)
        acc = ctx.read_accum()[..., :3]
    finally:
        ctx.close()
    assert (acc == F(0.5 * frames)).all(), "pixels off 0.5 x frames: %d" % int((acc != F(0.5 * frames)).any(axis=-1).sum())


def test_furnace_with_glass_conserves_energy(hiplib):
    """ior 1.5, max_bounces 16, tint 1, no eta^2 scaling: a path's throughput is exactly 1 until it leaves the glass for the constant
    map, so a pixel's expectation is 0.5 (1 - q), q the probability that the bounce limit cuts the path while it is still inside.
    The truncation bound, from F: an axis-aligned 2 x 2 x 2 box seen face-on from (0, 0, 5).  A primary ray meets the front face at
    an angle of at most theta_max = atan(sqrt(2) / 4) (the face's corner); reflected there (vertex 1) it leaves for the map.  Inside,
    its angle to the z axis is theta_1 <= asin(sin(theta_max) / 1.5) = 12.9 degrees and stays so: the side faces, met beyond the
    critical angle, reflect totally and keep |d.z|.  Between two visits of a z face the ray advances 2 in z and at most
    2 tan(theta_1) = 0.46 < 2 sideways per axis, so it meets at most two side faces: every three consecutive inside vertices hold
    a z-face vertex, where the path is reflected back in with probability F(theta_1) <= F_max = F(theta_max) (F grows with the
    angle; reciprocity).  Vertices 2..17 are sixteen inside vertices, at least five of them on z faces: q <= F_max^5, and the
    block means must agree with 0.5 inside 5 standard errors + 0.5 F_max^5."""
    w = h = 64
    n_batches, frames = 16, 32
    sc = scenes.Scene("furnace", [scenes.box_mesh(2.0, 2.0, 2.0)], [scenes.Instance(0, scenes.transform12(None, (0.0, 0.0, 0.0)), [1])],
                      np.stack([scenes.material(), scenes.material(transmission=1.0, ior=1.5)]),
                      scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 5.0)), fov_deg=40.0))
    ti = np.arctan(np.sqrt(2.0) / 4.0)
    tt = np.arcsin(np.sin(ti) / 1.5)
    f_max = 0.5 * (((np.cos(ti) - 1.5 * np.cos(tt)) / (np.cos(ti) + 1.5 * np.cos(tt))) ** 2 +
                   ((np.cos(tt) - 1.5 * np.cos(ti)) / (np.cos(tt) + 1.5 * np.cos(ti))) ** 2)
    truncation = 0.5 * f_max ** 5
    ctx = make_ctx(sc, w, h, bounces=16, lighting="map", env=GREY)
    try:
        out = []
        for b in range(n_batches):
            ctx.accum_reset()
            ctx.render(frames, 1 + b * frames)
            out.append(ctx.read_accum()[..., :3].astype(np.float64) / frames)
        ctx.set_outputs(depth=True)
        ctx.render(1, 1)
        depth = ctx.read_depth()
    finally:
        ctx.close()
    assert 0.1 < (depth < depth.max()).mean() < 0.9, "the box should cover part of the image"
    blocks = np.array(out).reshape(n_batches, h // 8, 8, w // 8, 8, 3).mean(axis=(2, 4))
    mean, se = blocks.mean(axis=0), np.sqrt(blocks.var(axis=0, ddof=1) / n_batches)
    print("F_max %.5f, truncation bound %.3e; block means min %.7f max %.7f, largest se %.2e" % (f_max, truncation, mean.min(), mean.max(), se.max()))
    assert (np.abs(mean - 0.5) <= 5.0 * se + truncation).all(), "largest deviation %.3e" % np.abs(mean - 0.5).max()


# ---- 5. the set-aside route ---------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from gdpathtracing_amd import capi
import test_gpu_transmission as t
sc = t.tied_glass_scene()
ctx = t.make_ctx(sc, 96, 64, capi.BUILD_SAH, capi.ACCUM_HDR_F32, 4, capi.KERNEL_WAVEFRONT, sys.argv[3])
ctx.render(2, 1)
np.save(sys.argv[2], ctx.read_accum())
st = ctx.stats()
ctx.close()
print(json.dumps({"set_aside": st["set_aside"], "dropped": st["set_aside_dropped"]}))
"""


def tied_glass_scene():
    """the fuzz soup with coincident triangles (exact distance ties) and the cracks of its reference tree, half its materials glass"""
    sc = scenes.random_scene(4, coincident=True, textured=False)
    used = sorted({m for i in sc.instances for m in i.material_ids})
    return scenes.with_transmissive_materials(sc, used[::2], transmission=0.9, ior=1.5)


@pytest.mark.parametrize("lighting", ["sky", "map_mis", "map_mis_emitters"])
def test_set_aside_paths_are_finished_with_the_lobe(hiplib, tmp_path, lighting):
    """JPT_BUILD_SAH on the wavefront kernels, its set-aside capacity forced, against the audit kernel on the same tree and against
    JPT_BUILD_REFERENCE_EXACT.  The emitter sampler draws from a list in the scene's triangle order, which each builder numbers its
    own way (test_whole_paths_equal_numpy makes one numpy render per order): under emitter sampling the two builders' renders are
    different estimates, so the REFERENCE_EXACT comparison is made where the lighting does not depend on that order, and the
    emitter lighting is compared on the one tree."""
    sc = tied_glass_scene()
    routes = [("audit", capi.BUILD_SAH, capi.KERNEL_REFERENCE_LAYOUT)]
    if "emitters" in lighting:
        pairs = [nls.tables(host_ref(sc, b))["pairs"] for b in (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH)]
        assert not np.array_equal(pairs[0], pairs[1]), "the builders list the emitters alike: compare with REFERENCE_EXACT here too"
    else:
        routes.append(("exact", capi.BUILD_REFERENCE_EXACT, capi.KERNEL_WAVEFRONT))
    out = {}
    for name, builder, kernel in routes:
        ctx = make_ctx(sc, 96, 64, builder, capi.ACCUM_HDR_F32, 4, kernel, lighting)
        try:
            ctx.render(2, 1)
            out[name] = ctx.read_accum()
        finally:
            ctx.close()
    env = dict(os.environ)
    env["JPT_SET_ASIDE_CAP"] = "1000000"
    path = str(tmp_path / "sah.npy")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, lighting], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads(r.stdout.strip().splitlines()[-1])
    print("set aside / dropped:", st)
    assert st["set_aside"] >= 1 and st["dropped"] == 0, st
    got = np.load(path)
    for name, want in out.items():
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        assert same.all(), "%s: %d pixels differ" % (name, int((~same).any(axis=-1).sum()))


# ---- 6. queued renders ------------------------------------------------------------------------------------------------------------------

def test_queued_renders_keep_the_flag_of_their_call(hiplib):
    sc = scenes.glass_cornell_scene()
    w, h = 160, 100
    want = {}
    for flags in (capi.MATERIAL_EXT_NONE, TX):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, bounces=4, flags=flags)
        try:
            ctx.render(2, 5)
            want[flags] = ctx.read_accum()
        finally:
            ctx.close()
    assert not np.array_equal(want[0], want[TX])
    ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, bounces=4, flags=None)
    try:
        got = []
        for flags in (0, TX, 0, TX, TX, 0):
            ctx.set_material_extensions(flags)
            ctx.accum_reset()
            ctx.render(2, 5, asynchronous=True)
            got.append((flags, ctx.read_accum()))
        for flags, img in got:
            assert np.array_equal(img, want[flags]), flags
    finally:
        ctx.close()


# ---- 7. other routes ------------------------------------------------------------------------------------------------------------------------

def test_multi_two_ranks_equals_one_context(hiplib):
    sc = scenes.glass_cornell_scene()
    w, h = 320, 200
    one = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, bounces=4, lighting="emitters")
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc)
        m.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
        m.set_camera(scenes.camera_block(sc.camera, w, h))
        m.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
        m.set_material_extensions(TX)
        one.render(4, 1)
        m.render(4, 1)
        assert np.array_equal(m.read_accum(), one.read_accum())
        assert np.array_equal(m.read_ldr(), one.read_ldr())
    finally:
        m.close()
        one.close()


def test_refit_moving_the_glass_equals_a_fresh_commit(hiplib):
    sc = scenes.glass_cornell_scene()
    w = h = 48
    t = np.stack([i.transform for i in sc.instances]).astype(F)
    moved = t.copy()
    moved[2, 9:] += np.array([-0.7, 0.4, 0.5], F)
    sc2 = copy.deepcopy(sc)
    sc2.instances[2].transform = moved[2].copy()
    ctx = make_ctx(sc, w, h, builder=capi.BUILD_SAH_WATERTIGHT)
    fresh = make_ctx(sc2, w, h, builder=capi.BUILD_SAH_WATERTIGHT)
    try:
        def again(c):
            c.accum_reset()
            c.render(2, 1)
            return c.read_accum()
        first = again(ctx)
        ctx.refit_tlas(moved)
        after = again(ctx)
        assert (after != first).any()
        assert np.array_equal(after, again(fresh))
        ctx.refit_tlas(t)
        assert np.array_equal(again(ctx), first)
    finally:
        ctx.close()
        fresh.close()


def test_denoise_and_display_run_on_a_glass_render(hiplib):
    sc = scenes.glass_cornell_scene()
    w, h = 96, 64
    ctx = make_ctx(sc, w, h, bounces=4)
    try:
        ctx.render(4, 1)
        ctx.denoise()
        den = ctx.read_denoised()
        assert den.shape[:2] == (h, w) and np.isfinite(den).all()
        ctx.display()
        assert ctx.read_display_ldr().shape[:2] == (h, w)
    finally:
        ctx.close()
