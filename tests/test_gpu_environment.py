"""HDR environment maps on the device (jpt_set_environment): the lookup the kernels inline against its numpy restatement, whole
paths against an environment-aware numpy path tracer, both kernels against each other, the sky cull, the ordering of map and
parameter changes against queued renders, and the map across the context's other features."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_env
import np_path
import np_restatement as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def sky_map(h=64, w=128, seed=5):
    """a smooth HDR gradient with noise and one small bright patch (a 'sun')"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    rgb = np.stack([0.3 + 0.7 * u / w, 0.2 + 1.5 * (1.0 - v / h), 0.5 + 0.5 * np.sin(6.0 * u / w)], axis=-1)
    rgb = rgb + 0.2 * rng.random((h, w, 3))
    rgb[h // 5:h // 5 + 3, w // 3:w // 3 + 4] = (30.0, 25.0, 18.0)
    return rgb.astype(F)


def checker_map(h=256, w=512, cells=32):
    v, u = np.mgrid[0:h, 0:w]
    on = ((u * cells // w) + (v * cells // (2 * h))) % 2 == 1
    return np.where(on[..., None], np.array([0.9, 0.7, 0.2], F), np.array([0.05, 0.1, 0.6], F)).astype(F)


def rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], F)


ROT = (rot_y(37.0) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])).astype(F)


def make_ctx(scene, w, h, builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, bounces=4, kernel=capi.KERNEL_WAVEFRONT, env=None,
             rot=None, intensity=1.0):
    ctx = host.Context(0)
    ctx.build_scene(scene, builder)
    ctx.set_params(w, h, bounces, accum)
    ctx.set_kernel(kernel)
    ctx.set_camera(scenes.camera_block(scene.camera, w, h))
    if env is not None:
        ctx.set_environment(env)
        ctx.set_environment_params(rot, intensity)
    return ctx


def images(ctx):
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth()


def assert_same(got, want, what):
    for g, x, name in zip(got, want, ("accumulation", "display", "depth")):
        bad = ~((g == x) | (np.isnan(g) & np.isnan(x)))
        if bad.ndim == 3:
            bad = bad.any(axis=-1)
        idx = np.argwhere(bad)
        assert len(idx) == 0, "%s: %s differs at %d pixels, first %s" % (what, name, len(idx), idx[:3].tolist())


# ---- 1. the lookup ---------------------------------------------------------------------------------------------------------

def test_device_lookup_equals_host_mirror_and_numpy(hiplib):
    import ctypes as C
    rgb = sky_map(96, 160)
    d = np_env.directions(1_000_000, seed=11)
    out = {}
    for dev in (0, -1):
        o = np.zeros_like(d)
        rc = hiplib.jpt_debug_env_lookup(dev, rgb.ctypes.data, 160, 96, ROT.ctypes.data, C.c_float(2.5), d.ctypes.data, len(d), o.ctypes.data)
        assert rc == 0, hiplib.jpt_debug_last_error()
        out[dev] = o
    want = np_env.env_radiance(rgb, d, ROT, 2.5)
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[-1].view(np.uint32), want.view(np.uint32))


# ---- 2. whole paths against numpy --------------------------------------------------------------------------------------------

def np_trace_env(ref, cam, width, height, max_bounces, rgb, rot, intensity):
    """np_path.trace_frame's loop with the gradient replaced by the environment lookup: radiance [H, W, 3] float32"""
    P = np_path
    with np.errstate(all="ignore"):
        ys, xs = np.mgrid[0:height, 0:width]
        px, py = xs.reshape(-1), ys.reshape(-1)
        n = len(px)
        seed = npr.prng_seed(px, py, int(cam["frame_index"]))
        seed, r = npr.pcg2d(seed)
        js, jc = P._sincos(F(6.2831853) * (r[:, 1] * F(0.25)))
        sx = (px.astype(F) + jc) / F(width) * F(2.0) - F(1.0)
        sy = (py.astype(F) + js) / F(height) * F(2.0) - F(1.0)
        nx, ny = sx, -sy
        m = cam["ivp"].astype(F)
        wx = m[0] * nx + m[4] * ny + m[8] + m[12]
        wy = m[1] * nx + m[5] * ny + m[9] + m[13]
        wz = m[2] * nx + m[6] * ny + m[10] + m[14]
        ww = m[3] * nx + m[7] * ny + m[11] + m[15]
        world = np.stack([wx / ww, wy / ww, wz / ww], axis=-1)
        cpos = np.array([cam["position"][k] for k in range(3)], dtype=F)
        o = np.broadcast_to(cpos, (n, 3)).astype(F)
        d = P._normalize(world - cpos[None, :])
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = np.ones(n, dtype=bool)
        for i in range(max_bounces + 1):
            t, tri, blas, lpos, lout, u, v, front = P._closest_hit(ref, o, d)
            hit = t < F(1e9)
            sky = np_env.env_radiance(rgb, d, rot, intensity)
            s = P._shading(ref, tri, blas, lpos, lout, u, v, front)
            emission = np.where(hit[:, None], s["emission"], sky)
            radiance = np.where(alive[:, None], radiance + throughput * emission, radiance)
            alive = alive & hit
            new_o = s["position"] + s["normal"] * F(0.001)
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = P._sample_brdf(s, xi)
            dens = P._density(s, new_d)
            lambert_in = P._dot(s["normal"], new_d)
            o = np.where(alive[:, None], new_o, o)
            d = np.where(alive[:, None], new_d, d)
            alive = alive & ~(lambert_in <= 0)
            f = (P._brdf(s, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where(alive[:, None], throughput * f, throughput)
        return radiance.reshape(height, width, 3)


def _quantise(x):
    q = np.floor(np.clip(x, F(0), F(1)) * F(255) + F(0.5))
    return (q.astype(F) / F(255)).astype(F)


def np_accumulate(ref, scene, w, h, frames, bounces, rgb, rot, intensity, ldr8):
    cam = scenes.camera_block(scene.camera, w, h).copy()
    acc = None
    for f in range(frames):
        cam["frame_index"] = 1 + f
        cur = np_trace_env(ref, cam, w, h, bounces, rgb, rot, intensity)
        if ldr8:
            cur = _quantise(cur)
        acc = cur if acc is None else (cur + acc).astype(F)
    return acc


def _small_random_scene():
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=24, textured=False, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    return sc


@pytest.mark.parametrize("which", ["cornell", "random"])
@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_whole_path_equals_numpy_with_a_map(oracle, hiplib, which, kernel):
    sc = scenes.cornell_scene() if which == "cornell" else _small_random_scene()
    w = h = 64
    rgb = sky_map()
    ref = oracle.build_scene(sc)
    for accum, frames in ((capi.ACCUM_HDR_F32, 2), (capi.ACCUM_REF_LDR8, 2)):
        want = np_accumulate(ref, sc, w, h, frames, 4, rgb, ROT, 1.7, accum == capi.ACCUM_REF_LDR8)
        for builder in (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH):
            ctx = make_ctx(sc, w, h, builder, accum, 4, kernel, rgb, ROT, 1.7)
            try:
                ctx.render(frames, 1)
                got, ldr, _ = images(ctx)
            finally:
                ctx.close()
            bad = np.argwhere((got[..., :3] != want).any(axis=-1))
            assert len(bad) == 0, "%s accum %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                which, accum, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])][:3], want[tuple(bad[0])])
            if accum == capi.ACCUM_REF_LDR8:   # the display: ACES of the mean, rgba8 (progressive_rendering.glsl:39-45)
                disp = npr.aces(want.astype(np.float64) / frames)
                q = np.floor(np.clip(disp, 0, 1) * 255 + 0.5)
                assert np.abs(ldr[..., :3].astype(int) - q).max() <= 1


def test_the_map_changes_the_image(oracle, hiplib):
    sc = scenes.cornell_scene()
    a = make_ctx(sc, 64, 64)
    b = make_ctx(sc, 64, 64, env=sky_map(), rot=ROT, intensity=1.7)
    try:
        a.render(2, 1)
        b.render(2, 1)
        assert (a.read_accum() != b.read_accum()).any(axis=-1).mean() > 0.3
    finally:
        a.close()
        b.close()


# ---- 3. both kernels, full size ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH])
def test_wavefront_equals_reference_layout_full_size(hiplib, builder):
    sc = scenes.demo_scene()
    w, h = 1920, 1080
    rgb = sky_map(512, 1024)
    out = []
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        ctx = make_ctx(sc, w, h, builder, capi.ACCUM_REF_LDR8, 4, kernel, rgb, ROT, 3.0)
        try:
            ctx.render(8, 1)
            out.append(images(ctx))
        finally:
            ctx.close()
    assert_same(out[0], out[1], "builder %d" % builder)


# ---- 4. the sky cull -----------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from gdpathtracing_amd import capi, host, scenes
sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_environment import checker_map, wide_scene, ROT
accum, per_render, renders, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
sc = wide_scene()
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(640, 360, 3, accum)
ctx.set_camera(scenes.camera_block(sc.camera, 640, 360))
ctx.set_environment(checker_map())
ctx.set_environment_params(ROT, 1.0)
for k in range(renders):
    ctx.render(per_render, 1 + k * per_render)
np.savez(out, accum=ctx.read_accum(), ldr=ctx.read_ldr(), depth=ctx.read_depth())
ctx.close()
"""


def wide_scene():
    sc = scenes.demo_scene(n_tris=4096)
    sc.camera = copy.deepcopy(sc.camera)
    sc.camera.fov_deg = 150.0
    return sc


@pytest.mark.parametrize("accum,per_render,renders", [(capi.ACCUM_REF_LDR8, 2, 2), (capi.ACCUM_REF_LDR8, 16, 1),
                                                      (capi.ACCUM_REF_LDR8, 24, 1), (capi.ACCUM_HDR_F32, 4, 2)])
def test_sky_cull_changes_nothing(hiplib, tmp_path, accum, per_render, renders):
    got = {}
    for cull in ("1", "0"):
        out = str(tmp_path / ("cull%s.npz" % cull))
        env = dict(os.environ, JPT_SKY_CULL=cull)
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(accum), str(per_render), str(renders), out], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        z = np.load(out)
        got[cull] = (z["accum"], z["ldr"], z["depth"])
    assert_same(got["1"], got["0"], "JPT_SKY_CULL=1 vs 0")


# ---- 5. / 6. set, clear, params, ordering -------------------------------------------------------------------------------------

def test_set_then_clear_equals_never_set(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    a = make_ctx(sc, 320, 200, accum=capi.ACCUM_REF_LDR8)
    b = make_ctx(sc, 320, 200, accum=capi.ACCUM_REF_LDR8, env=sky_map(), rot=ROT)
    try:
        a.render(4, 1)
        b.render(4, 1)
        assert (a.read_accum() != b.read_accum()).any()
        b.set_environment(None)
        a.accum_reset()
        b.accum_reset()
        a.render(4, 1)
        b.render(4, 1)
        assert_same(images(b), images(a), "cleared map")
    finally:
        a.close()
        b.close()


def test_params_alone_change_the_image(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    ctx = make_ctx(sc, 320, 200, env=sky_map(), rot=None, intensity=1.0)
    try:
        ctx.render(2, 1)
        a = ctx.read_accum()
        ctx.accum_reset()
        ctx.set_environment_params(ROT, 1.0)
        ctx.render(2, 1)
        b = ctx.read_accum()
        ctx.accum_reset()
        ctx.set_environment_params(ROT, 0.0)
        ctx.render(2, 1)
        c = ctx.read_accum()
        ctx.accum_reset()
        ctx.set_environment_params(None, 1.0)
        ctx.render(2, 1)
        assert (a != b).any() and (b != c).any()
        assert np.array_equal(ctx.read_accum(), a)
    finally:
        ctx.close()


def test_queued_renders_see_the_map_and_params_of_their_call(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 480, 270
    maps = [sky_map(64, 128, 1), None, checker_map(128, 256, 8), sky_map(32, 64, 2)]
    params = [(ROT, 1.0), (None, 1.0), (rot_y(90.0), 2.0), (rot_y(-20.0), 0.5)]
    # blocking: each step alone, starting from an empty accumulation
    want = []
    for k, (m, (r, i)) in enumerate(zip(maps, params)):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8)
        try:
            if m is not None:
                ctx.set_environment(m)
            ctx.set_environment_params(r, i)
            ctx.render(2, 1 + 2 * k)
            want.append(ctx.read_accum())
        finally:
            ctx.close()
    # queued: one context, accumulation reset between the steps, no wait but the one jpt_set_environment makes
    ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8)
    got = []
    try:
        for k, (m, (r, i)) in enumerate(zip(maps, params)):
            ctx.set_environment(m)
            for rep in range(3):                       # params changed with renders in flight, then set back
                ctx.set_environment_params(rot_y(10.0 * rep), 1.0 + rep)
                ctx.render(1, 1000 + rep, asynchronous=True)
            ctx.accum_reset()
            ctx.set_environment_params(r, i)
            ctx.render(2, 1 + 2 * k, asynchronous=True)
            got.append(ctx.read_accum())
    finally:
        ctx.close()
    for k in range(len(maps)):
        assert np.array_equal(got[k], want[k]), "step %d" % k


# ---- 7. the map across the context's other features ------------------------------------------------------------------------

def test_multi_two_ranks_equals_one_context(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 320, 200
    rgb = sky_map()
    one = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, env=rgb, rot=ROT, intensity=2.0)
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc)
        m.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
        m.set_camera(scenes.camera_block(sc.camera, w, h))
        m.set_environment(rgb)
        m.set_environment_params(ROT, 2.0)
        one.render(4, 1)
        m.render(4, 1)
        assert np.array_equal(m.read_accum(), one.read_accum())
        assert np.array_equal(m.read_ldr(), one.read_ldr())
    finally:
        m.close()
        one.close()


@pytest.mark.parametrize("mode", [capi.DENOISE_TEMPORAL, capi.DENOISE_NONE])
def test_denoise_modes_with_a_map(hiplib, mode):
    """the temporal and NONE modes on both kernels: the same images, and not the gradient's"""
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 320, 200
    out = []
    for kernel, env in ((capi.KERNEL_WAVEFRONT, sky_map()), (capi.KERNEL_REFERENCE_LAYOUT, sky_map()), (capi.KERNEL_WAVEFRONT, None)):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, kernel=kernel, env=env, rot=ROT)
        try:
            ctx.set_denoising_mode(mode)
            t = host.TemporalReprojection(w, h)
            for f in range(3):
                if mode == capi.DENOISE_TEMPORAL:
                    ctx.set_temporal_params(t.render(scenes.view_projection(sc.camera, w, h)))
                ctx.render(1, 1 + f)
            out.append(ctx.read_ldr())
        finally:
            ctx.close()
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], out[2])


def test_refit_and_mesh_update_with_a_map(hiplib):
    """jpt_scene_refit_tlas and jpt_scene_update_mesh with a map set: moving an instance (or deforming a mesh) changes the image,
    moving it back (restoring the vertices) gives the first image back bit for bit"""
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 320, 200
    ctx = make_ctx(sc, w, h, builder=capi.BUILD_SAH_WATERTIGHT, env=sky_map(), rot=ROT)
    try:
        def again():
            ctx.accum_reset()
            ctx.render(2, 1)
            return images(ctx)
        first = again()
        t = np.stack([i.transform for i in sc.instances]).astype(F)
        moved = t.copy()
        moved[-1, 9:] += np.array([0.3, 0.1, -0.2], F)
        ctx.refit_tlas(moved)
        assert (again()[0] != first[0]).any()
        ctx.refit_tlas(t)
        assert_same(again(), first, "refit_tlas and back")
        m0 = copy.deepcopy(sc.meshes[0])
        for s in m0.surfaces:
            s.vertices = (s.vertices * F(1.05)).astype(F)
        ctx.update_mesh(0, m0)
        assert (again()[0] != first[0]).any()
        ctx.update_mesh(0, sc.meshes[0])
        assert_same(again(), first, "update_mesh and back")
    finally:
        ctx.close()
