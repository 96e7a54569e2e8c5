"""Reflection probes on the device (jpt_set_reflection_probes, jpt_reflection_prefilter): the device's cube ray and prefilter and whole
paths against the numpy restatement (tests/np_reflection.py), the context's chain, a constant map end to end, ranks and queued renders,
what freeing the probes leaves unchanged, and the refusals.  Faces of 8 texels, three probes, two to a row (the fourth strip has no
probe): an image of 96 x 16; 2 frames, 4 bounces."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, partition, scenes

import np_reflection as nrf
from test_bake_host import atlas
from test_camera_host import soup_scene
from test_gpu_camera import make_ctx, same
from test_gpu_transmission import np_sum, sun_map
from test_reflection_host import N_PROBES, PER_ROW, PREFILTER_CASES, accum_image, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_STATE = -1, -4   # JPT_E_*
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)
S = 8
# inside Cornell's box ([-3, 3]^3 about the origin)
POSITIONS = np.array([(0.0, 0.25, 2.0), (1.25, 0.5, -0.5), (-1.5, -0.5, 0.25)], F)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def cube_ctx(scene, s=S, positions=POSITIONS, per_row=PER_ROW, **kw):
    """test_gpu_camera.make_ctx at the size the strips make, with the reflection probes set; the camera is the scene's (only near and
    far are read)"""
    w, h = nrf.image_size(len(positions), s, per_row)
    ctx = make_ctx(scene, None, w, h, **kw)
    try:
        ctx.set_reflection_probes(positions, s, per_row)
        assert ctx.reflection_image_size() == (w, h)
    except Exception:
        ctx.close()
        raise
    return ctx


def np_chain_level(accum, frames, n, s, per_row, n_levels, K, level):
    table, lvl = host.debug_reflection_samples(s, n_levels, K, level) if level else (None, None)
    return nrf.prefilter(accum, frames, n, s, per_row, n_levels, level, table, lvl)


# ---- 1. the device's functions ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", (4, 8))
def test_device_cube_rays_equal_numpy(hiplib, s):
    for frame in (0, 7):
        rays = host.debug_cube_rays(0, POSITIONS, s, PER_ROW, frame).reshape(-1, 6)
        _, wo, wd, wv = nrf.cube_rays(POSITIONS, s, PER_ROW, frame)
        assert same_bits(rays[:, :3], wo) and same_bits(rays[:, 3:], wd) and not wv.all(), frame
        assert same_bits(rays, host.debug_cube_rays(-1, POSITIONS, s, PER_ROW, frame).reshape(-1, 6))


@pytest.mark.parametrize("case", PREFILTER_CASES)
def test_device_prefilter_equals_numpy(hiplib, case):
    s, n_levels, K, n, per_row = case
    for frames in (1, 3):
        a = accum_image(s, n, per_row, frames)
        for level in range(n_levels):
            got = host.debug_reflection_prefilter(0, a, frames, n, s, per_row, level, n_levels=n_levels, samples=K)
            assert same_bits(got, np_chain_level(a, frames, n, s, per_row, n_levels, K, level)), (frames, level)


def test_a_larger_prefilter_equals_numpy(hiplib):
    """S = 64, seven levels, 256 samples, one probe: about two million gathers, and more than one block per level down to level 3"""
    s, n_levels, K = 64, 7, 256
    a = accum_image(s, 1, 1, 2, specials=False)
    for level in range(n_levels):
        got = host.debug_reflection_prefilter(0, a, 2, 1, s, 1, level, n_levels=n_levels, samples=K)
        assert same_bits(got, np_chain_level(a, 2, 1, s, 1, n_levels, K, level)), level


# ---- 2. whole paths against numpy -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cube_want(oracle):
    """(scene, the two frames under the sky, the last frame's depth, the two frames under sun_map())"""
    sc = scenes.cornell_scene()
    ref = oracle.build_scene(sc)
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    cam = scenes.camera_block(sc.camera, w, h).copy()
    sky, env, depth = [], [], None
    for f in range(2):
        cam["frame_index"] = 1 + f
        img, depth = nrf.trace_frame(ref, POSITIONS, S, PER_ROW, cam, 4)
        sky.append(img)
        env.append(nrf.trace_frame(ref, POSITIONS, S, PER_ROW, cam, 4, rgb=sun_map())[0])
    return sc, sky, depth, env


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH])
def test_whole_paths_equal_numpy(hiplib, cube_want, builder):
    sc, frames, want_depth, _ = cube_want
    assert (frames[0][S:, 6 * S:] == 0).all() and (frames[0][:S] > 0).any()
    want = np_sum(frames, False)
    for kernel in KERNELS:
        ctx = cube_ctx(sc, builder=builder, kernel=kernel)
        try:
            ctx.render(2, 1)
            got, depth = ctx.read_accum()[..., :3], ctx.read_depth()
        finally:
            ctx.close()
        bad = np.argwhere(~same(got, want).all(axis=-1))
        assert len(bad) == 0, "kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
            kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(_u32(depth), _u32(want_depth)), "depth: kernel %d builder %d" % (kernel, builder)


def test_whole_paths_under_a_map_equal_numpy(hiplib, cube_want):
    """wf2_primary_env_cube: every primary walk is queued, and the misses look the map up (np_env.env_radiance)"""
    sc, _, _, frames = cube_want
    want = np_sum(frames, False)
    for kernel in KERNELS:
        ctx = cube_ctx(sc, kernel=kernel, lighting="map")
        try:
            ctx.render(2, 1)
            got = ctx.read_accum()[..., :3]
        finally:
            ctx.close()
        bad = np.argwhere(~same(got, want).all(axis=-1))
        assert len(bad) == 0, "kernel %d: %d pixels differ, first %s: %s vs %s" % (kernel, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 3. through the context -------------------------------------------------------------------------------------------------------------------

def test_the_context_makes_the_chain_numpy_makes_and_leaves_the_accumulation_alone(hiplib):
    sc = scenes.cornell_scene()
    ctx = cube_ctx(sc)
    try:
        assert same_bits(ctx.read_reflection_probes(), POSITIONS)
        ctx.render(2, 1)
        for frames, n_levels, K in ((2, 0, 64), (4, 3, 16)):
            if frames == 4:
                ctx.render(2, 3)                                   # a second render continues the accumulation
                ctx.set_reflection_params(n_levels=n_levels, samples=K)
            before, depth = ctx.read_accum(), ctx.read_depth()
            ctx.reflection_prefilter()
            levels = n_levels or 4
            got = [ctx.read_reflection(level) for level in range(levels)]
            accum = ctx.read_accum()
            assert np.array_equal(_u32(before), _u32(accum)) and np.array_equal(_u32(depth), _u32(ctx.read_depth()))   # the call writes only its own images
            offset = 0
            for level in range(levels):
                want = np_chain_level(accum, frames, N_PROBES, S, PER_ROW, levels, K, level)
                assert got[level].shape == (N_PROBES, 6, S >> level, S >> level, 4) and same_bits(got[level], want), (frames, level)
                assert ctx.reflection_chain_size(level) == (S >> level, offset)
                offset += N_PROBES * 6 * (S >> level) ** 2
            assert (got[0][..., :3] > 0).any() and (got[levels - 1][..., :3] > 0).any()
            assert ctx._lib.jpt_read_reflection_f32(ctx.h, levels, host._ptr(np.zeros(96, F))) == E_INVALID
    finally:
        ctx.close()


# ---- 4. end to end: a constant map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_a_constant_map_gives_the_constant_at_every_level(hiplib, kernel):
    """a speck of a plane a thousand units away: no cube ray hits it, every path is one miss; level 0 is what a camera's misses
    accumulate, bit for bit, and every other level stays within the constant cube's bound (tests/test_reflection_host.py)"""
    base = scenes.cornell_scene()
    plane = scenes.plane_mesh(0.01)
    t12 = scenes.transform12(None, (0.0, -1000.0, 0.0))
    sc = scenes.Scene("speck", [plane], [scenes.Instance(0, t12, [0])], base.materials, base.camera)
    colour = np.array([0.375, 0.5, 0.25], F)
    env = np.broadcast_to(colour, (4, 8, 3)).astype(F)
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    cam_ctx = make_ctx(sc, None, w, h, kernel=kernel, env=env)
    try:
        cam_ctx.render(2, 1)
        miss = cam_ctx.read_accum()[..., :3]
    finally:
        cam_ctx.close()
    assert (_u32(miss) == _u32(miss[0, 0])).all()                 # every camera pixel misses, and a miss accumulates one value
    K = 64
    ctx = cube_ctx(sc, kernel=kernel, env=env)
    try:
        ctx.render(2, 1)
        accum = ctx.read_accum()[..., :3]
        ctx.reflection_prefilter()
        chain = [ctx.read_reflection(level) for level in range(4)]
    finally:
        ctx.close()
    assert (_u32(accum[:S]) == _u32(miss[0, 0])).all() and (_u32(accum[S:, :6 * S]) == _u32(miss[0, 0])).all() and (accum[S:, 6 * S:] == 0).all()
    assert (_u32(chain[0][..., :3]) == _u32((miss[0, 0] / F(2.0)).astype(F))).all()
    mean = (miss[0, 0] / F(2.0)).astype(np.float64)
    bound = (2 * K + 2) * 2.0 ** -24
    for level in range(1, 4):
        rel = np.abs(chain[level][..., :3].astype(np.float64) / mean - 1.0).max()
        print("kernel %d level %d: off by %.3g relative, bound %.3g" % (kernel, level, rel, bound))
        assert rel <= bound and (chain[level][..., 3] == 1).all()


# ---- 5. ranks and queued renders ----------------------------------------------------------------------------------------------------------------

def test_two_partitions_equal_one_context(hiplib):
    sc = scenes.cornell_scene()
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    one = cube_ctx(sc, accum=capi.ACCUM_REF_LDR8)
    try:
        one.render(2, 1)
        want = one.read_accum()
        got = np.zeros_like(want)
        for r in range(2):
            part = cube_ctx(sc, accum=capi.ACCUM_REF_LDR8, rank=r, world=2)
            try:
                part.render(2, 1)
                rows = partition.rows_of_rank(h, r, 2)
                got[rows] = part.read_accum()[rows]
                assert part._lib.jpt_reflection_prefilter(part.h) == E_STATE and b"jpt_reflection_prefilter" in part._lib.jpt_last_error(part.h)
            finally:
                part.close()
        assert np.array_equal(_u32(got), _u32(want)) and (want[..., :3] > 0).any()
    finally:
        one.close()


def test_two_queued_renders_equal_the_blocking_calls(hiplib):
    """two renders queued without a sync and the prefilter behind them give what the same calls give blocking"""
    sc = scenes.cornell_scene()

    def run(asynchronous):
        ctx = cube_ctx(sc, accum=capi.ACCUM_REF_LDR8)
        try:
            ctx.render(2, 5, asynchronous=asynchronous)
            ctx.render(2, 7, asynchronous=asynchronous)
            ctx.reflection_prefilter()
            return ctx.read_accum(), ctx.read_reflection(0), ctx.read_reflection(2)
        finally:
            ctx.close()
    want, got = run(False), run(True)
    assert np.array_equal(_u32(got[0]), _u32(want[0])) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])


# ---- 6. freeing the probes means a camera render ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_renders_after_freeing_the_probes_are_the_default_bits(hiplib, kernel):
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    sc = soup_scene()

    def render(probes_first):
        ctx = make_ctx(sc, None, w, h, accum=capi.ACCUM_REF_LDR8, kernel=kernel)
        try:
            cubed = culled = None
            if probes_first:
                ctx.set_reflection_probes(POSITIONS, S, PER_ROW)
                ctx.render(1, 1, counted=True)
                cubed, culled = ctx.read_accum(), ctx.stats()["sky_culled"]
                ctx.reflection_prefilter()
                ctx.accum_reset()
                ctx.set_reflection_probes(None)
                assert ctx._lib.jpt_read_reflection_probes(ctx.h, host._ptr(np.zeros((3, 3), F))) == E_STATE
                assert ctx._lib.jpt_read_reflection_f32(ctx.h, 0, host._ptr(np.zeros(4, F))) == E_STATE
            ctx.render(3, 1, counted=True)
            return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes(), ctx.stats()["sky_culled"], cubed, culled
        finally:
            ctx.close()
    want, got = render(False), render(True)
    assert all(np.array_equal(g, w_) for g, w_ in zip(got[:3], want[:3])) and got[3] == want[3]
    assert not np.array_equal(got[5], want[0])
    assert got[6] == 0 and got[4] == want[4]                      # a cube render culls nothing; the cull is back afterwards
    if kernel == capi.KERNEL_WAVEFRONT:
        assert want[4] > 0


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_what_a_cube_render_refuses_and_what_ignores_the_probes(hiplib):
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    sc, p4, n4 = atlas(w, h)
    ctx = cube_ctx(sc)
    L = ctx._lib

    def refused(word, what=b"reflection probes"):
        assert L.jpt_render(ctx.h, 1, 1) == E_STATE
        msg = L.jpt_last_error(ctx.h).lower()
        assert word in msg and what in msg, msg
        assert L.jpt_render_async(ctx.h, 1, 1) == E_STATE
    try:
        ctx.render(1, 1)
        ctx.set_params(33, 17, 4, capi.ACCUM_HDR_F32)      # another size than the strips make
        ctx.set_camera(scenes.camera_block(sc.camera, 33, 17))
        refused(b"96 x 16")
        ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.render(1, 1)
        ctx.set_lens(0.25, 6.5)
        refused(b"lens")
        ctx.set_lens(0.0, 1.0)
        for model in (capi.CAMERA_PROJECTIVE, capi.CAMERA_EQUIRECT):
            ctx.set_camera_model(model)
            refused(b"camera model")
        ctx.set_camera_model(capi.CAMERA_PINHOLE)
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        refused(b"temporal")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.render(1, 4)
        # beside bake images or light probes: refused, whatever their size
        ctx.set_bake_texels(p4, n4)
        refused(b"bake images")
        assert L.jpt_reflection_prefilter(ctx.h) == E_STATE and b"jpt_reflection_prefilter" in L.jpt_last_error(ctx.h)
        assert L.jpt_bake_finish(ctx.h) == E_STATE and b"jpt_bake_finish" in L.jpt_last_error(ctx.h) and b"reflection probes" in L.jpt_last_error(ctx.h)
        ctx.set_bake_texels(None, None)
        ctx.set_probes(POSITIONS, 8, 4, 2)
        refused(b"light probes")
        assert L.jpt_probe_project(ctx.h, 0) == E_STATE and b"jpt_probe_project" in L.jpt_last_error(ctx.h) and b"reflection probes" in L.jpt_last_error(ctx.h)
        assert L.jpt_reflection_prefilter(ctx.h) == E_STATE and b"jpt_reflection_prefilter" in L.jpt_last_error(ctx.h)
        ctx.set_probes(None)
        ctx.render(1, 5)
        # the guides and picking rays are camera rays
        assert L.jpt_denoise(ctx.h) == E_STATE and b"jpt_denoise" in L.jpt_last_error(ctx.h) and b"reflection probes" in L.jpt_last_error(ctx.h)
        xy = np.array([[3.5, 4.5]], F)
        hits = np.zeros(1, host.wire.RAY_HIT)
        assert L.jpt_query_pixels(ctx.h, host._ptr(xy), 1, host._ptr(hits)) == E_STATE and b"jpt_query_pixels" in L.jpt_last_error(ctx.h)
        ctx.set_reflection_probes(None)
        ctx.denoise()
        ctx.query_pixels(xy)
    finally:
        ctx.close()
    # DEBUG_STEPS ignores the probes, as it ignores the lens
    steps = []
    for probes in (False, True):
        c2 = make_ctx(sc, None, w, h)
        try:
            if probes:
                c2.set_reflection_probes(POSITIONS, S, PER_ROW)
            c2.set_debug_steps(True)
            c2.render(1, 1)
            steps.append(c2.read_accum())
        finally:
            c2.close()
    assert np.array_equal(steps[0], steps[1]) and (steps[0][..., :3] > 0).any()


def test_what_the_prefilter_refuses(hiplib):
    w, h = nrf.image_size(N_PROBES, S, PER_ROW)
    sc = scenes.cornell_scene()
    ctx = make_ctx(sc, None, w, h)
    L = ctx._lib
    out = np.zeros((N_PROBES, 6, S, S, 4), F)

    def refused(rc, word, call=b"jpt_reflection_prefilter", code=E_STATE):
        assert rc == code, rc
        msg = L.jpt_last_error(ctx.h)
        assert call in msg and word in msg, msg
    try:
        ctx.render(1, 1)
        refused(L.jpt_reflection_prefilter(ctx.h), b"no reflection probes")
        refused(L.jpt_read_reflection_f32(ctx.h, 0, host._ptr(out)), b"no jpt_reflection_prefilter", b"jpt_read_reflection_f32")
        ctx.set_reflection_params(n_levels=6, samples=32)          # no face size to check against yet
        ctx.set_reflection_probes(POSITIONS, S, PER_ROW)
        ctx.accum_reset()
        refused(L.jpt_reflection_prefilter(ctx.h), b"no frame")
        ctx.render(1, 1)
        refused(L.jpt_reflection_prefilter(ctx.h), b"n_levels is 6")
        refused(L.jpt_set_reflection_params(ctx.h, host.C.byref(capi.ReflectionParams(5, 32))), b"n_levels", b"jpt_set_reflection_params", E_INVALID)
        ctx.set_reflection_params()
        refused(L.jpt_read_reflection_f32(ctx.h, 0, host._ptr(out)), b"no jpt_reflection_prefilter", b"jpt_read_reflection_f32")
        ctx.set_denoising_mode(capi.DENOISE_NONE)
        refused(L.jpt_reflection_prefilter(ctx.h), b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_reflection_prefilter(ctx.h), b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.reflection_prefilter()
        first = ctx.read_reflection(1)
        assert (first[..., :3] > 0).any()
        # another size: the prefilter and the read-back both refuse
        ctx.set_params(33, 17, 4, capi.ACCUM_HDR_F32)
        refused(L.jpt_reflection_prefilter(ctx.h), b"96 x 16")
        refused(L.jpt_read_reflection_f32(ctx.h, 1, host._ptr(out)), b"no jpt_reflection_prefilter", b"jpt_read_reflection_f32")
        ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.reflection_prefilter()
        assert same_bits(ctx.read_reflection(1), first)
        # other parameters, other probes: no chain of them yet
        ctx.set_reflection_params(samples=16)
        refused(L.jpt_read_reflection_f32(ctx.h, 1, host._ptr(out)), b"no jpt_reflection_prefilter", b"jpt_read_reflection_f32")
        ctx.reflection_prefilter()
        assert not same_bits(ctx.read_reflection(1), first) and same_bits(ctx.read_reflection(0), np_chain_level(ctx.read_accum(), 1, N_PROBES, S, PER_ROW, 4, 16, 0))
        ctx.set_reflection_probes(POSITIONS[:2], 4, 1)
        refused(L.jpt_read_reflection_f32(ctx.h, 0, host._ptr(out)), b"no jpt_reflection_prefilter", b"jpt_read_reflection_f32")
        assert ctx.reflection_image_size() == (24, 8)
        assert not hasattr(L, "jpt_multi_reflection_prefilter")
        # kernel timing: the two steps' times, only of a call made under it
        refused(L.jpt_get_reflection_timing(ctx.h, host.C.byref(host.C.c_float()), host.C.byref(host.C.c_float())), b"jpt_set_kernel_timing", b"jpt_get_reflection_timing")
        ctx.set_params(24, 8, 4, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, 24, 8))
        ctx.render(1, 1)
        ctx.set_kernel_timing(True)
        ctx.reflection_prefilter()
        chain_ms, prefilter_ms = ctx.reflection_timing()
        ctx.set_kernel_timing(False)
        assert chain_ms > 0 and prefilter_ms > 0
    finally:
        ctx.close()
