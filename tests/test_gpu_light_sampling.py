"""Importance sampling of the emissive triangles on the device (jpt_set_light_sampling, JPT_LIGHT_SAMPLING_MIS): the emitter tables
and the sampler against numpy, whole paths against the NEE-aware numpy path tracer (tests/np_light_sampling.py), alone and with the
map's own MIS, what the mode leaves unchanged, unbiasedness and the variance it saves, and the mode across queued renders, ranks,
denoising modes, a TLAS refit and a mesh update."""
import copy

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_light_sampling as nls

pytestmark = pytest.mark.gpu

F = np.float32
LMIS, LBRDF = capi.LIGHT_SAMPLING_MIS, capi.LIGHT_SAMPLING_BRDF


def sun_map(h=32, w=64):
    v, u = np.mgrid[0:h, 0:w]
    rgb = np.stack([0.6 + 0.4 * u / w, 0.7 + 0.3 * (1.0 - v / h), 0.9 + 0.1 * np.cos(4.0 * u / w)], axis=-1) * 0.2
    rgb[h // 6:h // 6 + 3, w // 3:w // 3 + 4] = (20.0, 18.0, 15.0)
    return rgb.astype(F)


def make_ctx(scene, w, h, builder=capi.BUILD_SAH, accum=capi.ACCUM_HDR_F32, bounces=3, kernel=capi.KERNEL_WAVEFRONT, env=None,
             env_mis=False, mode=LMIS):
    ctx = host.Context(0)
    ctx.build_scene(scene, builder)
    ctx.set_params(w, h, bounces, accum)
    ctx.set_kernel(kernel)
    ctx.set_camera(scenes.camera_block(scene.camera, w, h))
    if env is not None:
        ctx.set_environment(env)
        if env_mis:
            ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
    if mode is not None:
        ctx.set_light_sampling(mode)
    return ctx


def small_light_cornell(scale=0.25):
    sc = scenes.cornell_scene()
    t = sc.instances[0].transform.copy()
    t[:9] = t[:9] * F(scale)
    sc.instances[0].transform = t
    return sc


def small_random_scene():
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=24, textured=False, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    return sc


class _Ref:
    """the context's own reference-layout arrays, as np_path reads them"""
    def __init__(self, ctx):
        self.tri_geom = ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY)
        self.tri_data = ctx.reference_buffer(capi.BUF_TRI_DATA, wire.TRI_DATA)
        self.materials = ctx.reference_buffer(capi.BUF_MATERIALS, wire.MATERIAL)
        self.bvh_nodes = ctx.reference_buffer(capi.BUF_BVH_NODES, wire.BVH_NODE)
        self.instances = ctx.reference_buffer(capi.BUF_INSTANCES, wire.BLAS_INSTANCE)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the tables and the sampler ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["cornell", "random", "demo"])
def test_device_tables_and_sampler_equal_numpy(hiplib, which):
    sc = {"cornell": scenes.cornell_scene, "random": lambda: scenes.random_scene(5, textured=False),
          "demo": lambda: scenes.demo_scene(n_tris=4096)}[which]()
    ctx = make_ctx(sc, 16, 16, builder=capi.BUILD_SAH)
    try:
        ref = _Ref(ctx)
        pairs, tri, cdf, marg = ctx.debug_light_tables()
        want = nls.tables(ref)
        assert len(pairs) > 0
        assert np.array_equal(pairs.astype(np.int64), want["pairs"])
        assert np.array_equal(_u32(tri), _u32(want["tri"]))
        assert np.array_equal(_u32(cdf), _u32(want["cdf"]))
        assert np.array_equal(_u32(marg), _u32(want["marg"]))
        rng = np.random.default_rng(7)
        n = 4096
        xi = rng.random((n, 4)).astype(F)
        xi[:8, :2] = [[0, 0], [1, 1], [0.99999994, 0.5], [0.5, 0.99999994], [0, 1], [1, 0], [0.5, 0.5], [0.25, 0.75]]
        orig = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
        pts, dirs, pdf = ctx.debug_light_sample(xi, orig)
        y, l, p = nls.sample_seen_from(want, xi, orig)
        assert np.array_equal(_u32(pts), _u32(y))
        assert np.array_equal(_u32(dirs), _u32(l))
        assert np.array_equal(_u32(pdf), _u32(p))
        # the density at hits, for every emitter and a few non-emitters (density 0)
        k = rng.integers(0, len(pairs), n)
        inst, tr = pairs[k, 0], pairs[k, 1]
        got = ctx.debug_light_pdf(inst, tr, y, orig, l)
        assert np.array_equal(_u32(got), _u32(nls.hit_pdf(ref, want, inst, tr, y, orig, l)))
        assert (got > 0).mean() > 0.5
    finally:
        ctx.close()


# ---- 2. whole paths against numpy ------------------------------------------------------------------------------------------------

def np_accumulate(ref, scene, w, h, frames, bounces, ldr8, tabs, rgb=None, env_mis=False):
    cam = scenes.camera_block(scene.camera, w, h).copy()
    acc = None
    for f in range(frames):
        cam["frame_index"] = 1 + f
        cur = nls.trace_lights(ref, cam, w, h, bounces, rgb=rgb, env_mis=env_mis, tabs=tabs)
        if ldr8:
            cur = (np.floor(np.clip(cur, F(0), F(1)) * F(255) + F(0.5)).astype(F) / F(255)).astype(F)
        acc = cur if acc is None else (cur + acc).astype(F)
    return acc


def builder_tables(scene, builder):
    """the emitter tables of the scene as `builder` lays it out: the native builders number the triangles their own way, and the
    emitter list follows the scene's triangle order"""
    ctx = host.Context(-1)
    try:
        ctx.build_scene(scene, builder)
        return nls.tables(_Ref(ctx))
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["cornell", "random"])
@pytest.mark.parametrize("env", ["sky", "map_mis"])
def test_whole_path_equals_numpy_with_light_sampling(oracle, hiplib, which, env):
    sc = {"cornell": small_light_cornell, "random": small_random_scene}[which]()
    w = h = 32
    rgb = sun_map() if env == "map_mis" else None
    ref = oracle.build_scene(sc)
    tabs = {b: builder_tables(sc, b) for b in (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT)}
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        wants = []   # (tables, image): one numpy render per distinct emitter order
        for builder in (capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT):
            t = tabs[builder]
            want = next((img for tt, img in wants if np.array_equal(tt["pairs"], t["pairs"])), None)
            if want is None:
                want = np_accumulate(ref, sc, w, h, 2, 3, accum == capi.ACCUM_REF_LDR8, t, rgb, env == "map_mis")
                wants.append((t, want))
            for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
                ctx = make_ctx(sc, w, h, builder, accum, 3, kernel, rgb, env == "map_mis")
                try:
                    ctx.render(2, 1)
                    got = ctx.read_accum()[..., :3]
                finally:
                    ctx.close()
                bad = np.argwhere((got != want).any(axis=-1))
                assert len(bad) == 0, "%s %s accum %d kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                    which, env, accum, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 3. what the mode leaves unchanged ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT])
def test_off_by_default_and_emitter_free_renders_are_unchanged(hiplib, kernel):
    sc = scenes.cornell_scene()
    dark = scenes.random_scene(5, textured=False)
    dark.materials = dark.materials.copy()
    dark.materials["emission"][:, 3] = 0.0
    for scene, env in ((sc, None), (dark, None), (dark, sun_map())):
        out = []
        for steps in ([], [LBRDF], [LMIS, LBRDF]) if scene is sc else ([], [LMIS]):
            ctx = make_ctx(scene, 64, 48, accum=capi.ACCUM_REF_LDR8, kernel=kernel, env=env, mode=None)
            try:
                for m in steps:
                    ctx.set_light_sampling(m)
                ctx.render(3, 1)
                out.append((ctx.read_accum(), ctx.read_ldr()))
            finally:
                ctx.close()
        for o in out[1:]:
            assert np.array_equal(o[0], out[0][0]) and np.array_equal(o[1], out[0][1])


BLACK = np.zeros((8, 16, 3), F)   # a black map: the scene's emitters are its only light


def test_light_sampling_changes_the_image(hiplib):
    sc = small_light_cornell()
    a = make_ctx(sc, 48, 48, mode=LBRDF, env=BLACK)
    b = make_ctx(sc, 48, 48, mode=LMIS, env=BLACK)
    try:
        a.render(2, 1)
        b.render(2, 1)
        assert (a.read_accum() != b.read_accum()).any(axis=-1).mean() > 0.2
    finally:
        a.close()
        b.close()


# ---- 4. unbiasedness and variance -------------------------------------------------------------------------------------------------

def _batches(ctx, n_batches, frames, first=1):
    out = []
    for b in range(n_batches):
        ctx.accum_reset()
        ctx.render(frames, first + b * frames)
        out.append(ctx.read_accum()[..., :3].astype(np.float64) / frames)
    return np.array(out)


@pytest.mark.parametrize("env", ["sky", "map_mis"])
def test_light_sampling_is_unbiased(hiplib, env):
    sc = scenes.cornell_scene()
    w = h = 64
    means = {}
    for mode in (LBRDF, LMIS):
        ctx = make_ctx(sc, w, h, mode=mode, bounces=3, env=sun_map() if env == "map_mis" else None, env_mis=env == "map_mis")
        try:
            b = _batches(ctx, 16, 64)
        finally:
            ctx.close()
        blocks = np.nanmean(b.reshape(16, h // 8, 8, w // 8, 8, 3), axis=(2, 4))
        means[mode] = (blocks.mean(axis=0), blocks.var(axis=0, ddof=1) / 16)
    diff = np.abs(means[LMIS][0] - means[LBRDF][0])
    se = np.sqrt(means[LMIS][1] + means[LBRDF][1])
    print("largest deviation %.2f sigma" % float((diff / (se + 1e-12)).max()))
    assert (diff <= 5.0 * se + 1e-3 * np.abs(means[LBRDF][0]) + 1e-6).all(), "largest deviation %.2f sigma" % float((diff / (se + 1e-12)).max())


def test_light_sampling_cuts_variance_under_a_small_light(hiplib):
    """the cornell box with its light scaled to 0.5 and a black map (the open box's sky would otherwise light it as much).
    Measured, 512 frames: the median per-pixel variance over lit pixels drops 279x (2 bounces; 5376x with 1).  With the light
    scaled to 0.25 BRDF sampling never finds it in 512 frames at most lit pixels, whose BRDF variance then reads 0: the median
    over the pixels that did see it drops 1559x.  The mean over lit pixels drops 4.0x (0.25: 2.3x): it is set by the ceiling just
    above the light's back face, where neither strategy does well."""
    sc = small_light_cornell(0.5)
    w = h = 64
    per = {}
    for mode in (LBRDF, LMIS):
        ctx = make_ctx(sc, w, h, mode=mode, bounces=2, env=BLACK)
        try:
            ctx.set_outputs(depth=True)
            b = _batches(ctx, 256, 1)
            depth = ctx.read_depth()
        finally:
            ctx.close()
        per[mode] = (b.mean(axis=0).sum(-1), b.var(axis=0, ddof=1).sum(-1), depth)
    mean_b, var_b, depth = per[LBRDF]
    mean_m, var_m, _ = per[LMIS]
    lit = (depth < depth.max()) & (mean_m > 0.05 * np.median(mean_m[mean_m > 0]))
    assert lit.sum() > 200, lit.sum()
    ratio = float(np.median(var_b[lit]) / max(np.median(var_m[lit]), 1e-30))
    print("median per-pixel variance BRDF / light MIS on %d lit pixels: %.1f (mean: %.2f)" % (
        lit.sum(), ratio, float(var_b[lit].mean() / var_m[lit].mean())))
    assert ratio >= 50.0, ratio


# ---- 5. the mode across the context's other features ---------------------------------------------------------------------------

def test_queued_renders_keep_the_mode_of_their_call(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 160, 100
    want = {}
    for mode in (LBRDF, LMIS):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, mode=mode)
        try:
            ctx.render(2, 5)
            want[mode] = ctx.read_accum()
        finally:
            ctx.close()
    assert not np.array_equal(want[LBRDF], want[LMIS])
    ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, mode=LBRDF)
    try:
        got = []
        for k, mode in enumerate((LBRDF, LMIS, LBRDF, LMIS, LMIS, LBRDF)):
            ctx.set_light_sampling(mode)
            ctx.accum_reset()
            ctx.render(2, 5, asynchronous=True)
            got.append((mode, ctx.read_accum()))
        for mode, img in got:
            assert np.array_equal(img, want[mode]), mode
    finally:
        ctx.close()


def test_multi_two_ranks_equals_one_context(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 320, 200
    one = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, bounces=4)
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc)
        m.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
        m.set_camera(scenes.camera_block(sc.camera, w, h))
        m.set_light_sampling(LMIS)
        one.render(4, 1)
        m.render(4, 1)
        assert np.array_equal(m.read_accum(), one.read_accum())
        assert np.array_equal(m.read_ldr(), one.read_ldr())
    finally:
        m.close()
        one.close()


@pytest.mark.parametrize("mode", [capi.DENOISE_PROGRESSIVE, capi.DENOISE_TEMPORAL, capi.DENOISE_NONE])
def test_denoise_modes_with_light_sampling(hiplib, mode):
    """every denoising mode on both kernels: the same images, and not BRDF mode's"""
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 320, 200
    out = []
    for kernel, samp in ((capi.KERNEL_WAVEFRONT, LMIS), (capi.KERNEL_REFERENCE_LAYOUT, LMIS), (capi.KERNEL_WAVEFRONT, LBRDF)):
        ctx = make_ctx(sc, w, h, accum=capi.ACCUM_REF_LDR8, kernel=kernel, mode=samp)
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


def test_refit_moving_the_light_equals_a_fresh_commit(hiplib):
    sc = small_light_cornell(0.5)
    w = h = 48
    t = np.stack([i.transform for i in sc.instances]).astype(F)
    moved = t.copy()
    moved[0, 9:] += np.array([0.6, -0.3, 0.4], F)
    sc2 = copy.deepcopy(sc)
    sc2.instances[0].transform = moved[0].copy()
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


def test_update_mesh_of_the_emitter_equals_a_fresh_commit(hiplib):
    sc = scenes.cornell_scene()
    w = h = 48
    sc2 = copy.deepcopy(sc)
    light_mesh = sc2.meshes[sc2.instances[0].mesh]
    for s in light_mesh.surfaces:
        s.vertices[:] = (s.vertices * F(0.5) + np.array([0.3, 0.0, -0.2], F)).astype(F)
    # the emitter's mesh must be its own: the plane mesh is shared by no other instance of the cornell box
    assert sum(1 for i in sc.instances if i.mesh == sc.instances[0].mesh) == 1
    ctx = make_ctx(sc, w, h, builder=capi.BUILD_SAH_WATERTIGHT)
    fresh = make_ctx(sc2, w, h, builder=capi.BUILD_SAH_WATERTIGHT)
    try:
        ctx.render(2, 1)
        first = ctx.read_accum()
        ctx.update_mesh(sc.instances[0].mesh, light_mesh, with_normals=False)
        ctx.accum_reset()
        ctx.render(2, 1)
        after = ctx.read_accum()
        fresh.render(2, 1)
        assert (after != first).any()
        assert np.array_equal(after, fresh.read_accum())
    finally:
        ctx.close()
        fresh.close()
