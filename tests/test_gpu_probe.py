"""Light probes on the device (jpt_set_probes, jpt_probe_project): the device's probe ray and projection and whole paths against the
numpy restatement (tests/np_probe.py), the wavefront kernels against the audit kernel under every lighting, the context's projection,
a constant map end to end, ranks and queued renders, what freeing the probes leaves unchanged, and the refusals.  Images 24 x 8, 36 x
12 and 48 x 16: tiles 8 x 4, 12 x 6 and 16 x 8, five probes, three to a row (the sixth tile has no probe); 2 frames, 4 bounces."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, partition, scenes

import np_probe as npb
from test_bake_host import atlas, atlas_scene
from test_camera_host import soup_scene
from test_gpu_camera import make_ctx, same
from test_gpu_transmission import glass_random_scene, np_sum, sun_map
from test_probe_host import N_PROBES, PER_ROW, TILES, accum_image, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_STATE = -1, -4   # JPT_E_*
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)
# around the soup and over the floor of test_bake_host.atlas_scene (the floor lies at y = -2.2); the last one just above the floor
POSITIONS = np.array([(0.0, 0.5, 4.0), (2.5, 1.0, -1.0), (-3.0, -1.0, 0.5), (0.3, 3.5, 0.2), (0.4, -1.9, 0.3)], F)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def probe_ctx(scene, tile, positions=POSITIONS, per_row=PER_ROW, **kw):
    """test_gpu_camera.make_ctx at the size the probes make, with the probes set; the camera is the scene's (only near and far are read)"""
    tw, th = tile
    w, h = npb.image_size(len(positions), tw, th, per_row)
    ctx = make_ctx(scene, None, w, h, **kw)
    try:
        ctx.set_probes(positions, tw, th, per_row)
        assert ctx.probe_image_size() == (w, h)
    except Exception:
        ctx.close()
        raise
    return ctx


# ---- 1. the device's functions ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", TILES)
def test_device_probe_rays_and_projection_equal_numpy(hiplib, tile):
    tw, th = tile
    for frame in (1, 78):
        o, d, valid = host.debug_probe_rays(0, POSITIONS, tw, th, PER_ROW, frame)
        _, wo, wd, wv = npb.probe_rays(POSITIONS, tw, th, PER_ROW, frame)
        assert np.array_equal(valid.reshape(-1) != 0, wv) and not wv.all(), frame
        assert same_bits(o.reshape(-1, 3), wo) and same_bits(d.reshape(-1, 3), wd), frame
    for frames in (1, 3):
        a = accum_image(tw, th, frames)
        for flags in (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE):
            table = host.debug_probe_basis(tw, th, flags)
            got = host.debug_probe_project(0, a, frames, N_PROBES, tw, th, PER_ROW, table)
            assert same_bits(got, npb.project(a, frames, N_PROBES, tw, th, PER_ROW, table)), (frames, flags)
    # one probe more than a block of four, a lone probe, and a last row of tiles that is full
    for n, per_row in ((1, 1), (6, 3), (9, 2)):
        w, h = npb.image_size(n, tw, th, per_row)
        a = (np.random.default_rng(n).uniform(0.0, 2.0, (h, w, 4))).astype(F)
        got = host.debug_probe_project(0, a, 1, n, tw, th, per_row, table)
        assert same_bits(got, npb.project(a, 1, n, tw, th, per_row, table)), (n, per_row)


@pytest.mark.parametrize("tile", [(4, 2), (5, 3), (64, 16)])
def test_device_projection_at_the_limit_tiles_is_finite_and_equals_numpy(hiplib, tile):
    """the smallest tile (blind to coefficients 6 and 8: zeros, not NaN), the smallest that sees all nine, and the largest (36 KB of LDS)"""
    tw, th = tile
    n, per_row = 5, 3
    w, h = npb.image_size(n, tw, th, per_row)
    a = np.random.default_rng(tw).uniform(0.5, 2.0, (h, w, 4)).astype(F)
    table = host.debug_probe_basis(tw, th, capi.PROBE_IRRADIANCE)
    got = host.debug_probe_project(0, a, 2, n, tw, th, per_row, table)
    assert np.isfinite(got).all() and same_bits(got, npb.project(a, 2, n, tw, th, per_row, table))
    for k, blind in ((6, th == 2), (8, tw == 4)):
        assert (got[:, k, :3] == 0).all() == blind, k


# ---- 2. whole paths against numpy -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe_want(oracle):
    """per tile: (scene, the two frames under the sky, the last frame's depth, the two frames under sun_map())"""
    out = {}
    sc, _ = atlas_scene()
    ref = oracle.build_scene(sc)
    for tw, th in TILES:
        w, h = npb.image_size(N_PROBES, tw, th, PER_ROW)
        cam = scenes.camera_block(sc.camera, w, h).copy()
        sky, env, depth = [], [], None
        for f in range(2):
            cam["frame_index"] = 1 + f
            img, depth = npb.trace_frame(ref, POSITIONS, tw, th, PER_ROW, cam, 4)
            sky.append(img)
            env.append(npb.trace_frame(ref, POSITIONS, tw, th, PER_ROW, cam, 4, rgb=sun_map())[0])
        out[tw, th] = (sc, sky, depth, env)
    return out


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT])
@pytest.mark.parametrize("tile", TILES)
def test_whole_paths_equal_numpy(hiplib, probe_want, tile, builder):
    tw, th = tile
    sc, frames, want_depth, _ = probe_want[tile]
    assert (frames[0][th:, 2 * tw:] == 0).all() and (frames[0][:th] > 0).any()
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        want = np_sum(frames, accum == capi.ACCUM_REF_LDR8)
        for kernel in KERNELS:
            ctx = probe_ctx(sc, tile, builder=builder, accum=accum, kernel=kernel)
            try:
                ctx.render(2, 1)
                got, depth = ctx.read_accum()[..., :3], ctx.read_depth()
            finally:
                ctx.close()
            bad = np.argwhere(~same(got, want).all(axis=-1))
            assert len(bad) == 0, "accum %d kernel %d builder %d: %d pixels differ, first %s: %s vs %s" % (
                accum, kernel, builder, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            assert np.array_equal(_u32(depth), _u32(want_depth)), "depth: accum %d kernel %d builder %d" % (accum, kernel, builder)


@pytest.mark.parametrize("tile", TILES)
def test_whole_paths_under_a_map_equal_numpy(hiplib, probe_want, tile):
    """wf2_primary_env_probe: every primary walk is queued, and the misses look the map up (np_env.env_radiance)"""
    sc, _, _, frames = probe_want[tile]
    want = np_sum(frames, False)
    for kernel in KERNELS:
        ctx = probe_ctx(sc, tile, kernel=kernel, lighting="map")
        try:
            ctx.render(2, 1)
            got = ctx.read_accum()[..., :3]
        finally:
            ctx.close()
        bad = np.argwhere(~same(got, want).all(axis=-1))
        assert len(bad) == 0, "kernel %d: %d pixels differ, first %s: %s vs %s" % (kernel, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 3. every family: the wavefront kernels against the audit kernel ------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ["map_mis", "emitters", "map_mis_emitters", "glass"])
def test_wavefront_equals_reference_layout_under_every_lighting(hiplib, lighting):
    """probes inside Cornell's box; glass: inside the partly transmissive soup, under every light"""
    glass = lighting == "glass"
    sc = glass_random_scene() if glass else scenes.cornell_scene()
    pos = (POSITIONS * F(0.25 if glass else 0.5)).astype(F)   # (Cornell's box is [-3, 3]^3 about the origin)
    tile = (12, 6)
    out = {}
    for kernel in KERNELS:
        ctx = probe_ctx(sc, tile, positions=pos, builder=capi.BUILD_SAH, kernel=kernel, lighting="map_mis_emitters" if glass else lighting,
                        flags=capi.MATERIAL_EXT_TRANSMISSION if glass else None)
        try:
            ctx.render(2, 1)
            out[kernel] = (ctx.read_accum(), ctx.read_depth())
        finally:
            ctx.close()
    a, b = out[capi.KERNEL_WAVEFRONT], out[capi.KERNEL_REFERENCE_LAYOUT]
    assert same(a[0], b[0]).all(), "%s: %d pixels differ" % (lighting, int((~same(a[0], b[0])).any(axis=-1).sum()))
    assert np.array_equal(_u32(a[1]), _u32(b[1]))
    assert (a[0][:6, :, :3] > 0).any() and (a[0][6:, 24:, :3] == 0).all()


# ---- 4. through the context -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", TILES)
def test_the_context_projects_what_numpy_projects(hiplib, tile):
    tw, th = tile
    sc, _ = atlas_scene()
    ctx = probe_ctx(sc, tile)
    try:
        assert same_bits(ctx.read_probes(), POSITIONS)
        ctx.render(2, 1)
        for frames, flags in ((2, capi.PROBE_RADIANCE), (2, capi.PROBE_IRRADIANCE), (4, capi.PROBE_IRRADIANCE), (4, capi.PROBE_RADIANCE)):
            if frames == 4 and flags == capi.PROBE_IRRADIANCE:
                ctx.render(2, 3)                                   # a second render continues the accumulation
            before = ctx.read_accum()
            ctx.probe_project(flags)
            got = ctx.read_probe_sh()
            accum = ctx.read_accum()
            assert np.array_equal(_u32(before), _u32(accum))       # the call writes only its own buffer
            table = host.debug_probe_basis(tw, th, flags)
            want = npb.project(accum, frames, N_PROBES, tw, th, PER_ROW, table)
            assert got.shape == (N_PROBES, 9, 4) and same_bits(got, want), (frames, flags)
            assert (got[:, 0, :3] > 0).all()
    finally:
        ctx.close()


# ---- 5. end to end: a constant map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_a_constant_map_gives_the_constant_in_coefficient_zero(hiplib, kernel):
    """a speck of a plane a thousand units away: no probe ray hits it, every path is one miss, and every cell's mean is the map's colour"""
    base = scenes.cornell_scene()
    plane = scenes.plane_mesh(0.01)
    t12 = scenes.transform12(None, (0.0, -1000.0, 0.0))
    sc = scenes.Scene("speck", [plane], [scenes.Instance(0, t12, [0])], base.materials, base.camera)
    colour = np.array([0.375, 0.5, 0.25], F)
    env = np.broadcast_to(colour, (4, 8, 3)).astype(F)
    for tw, th in TILES:
        ctx = probe_ctx(sc, (tw, th), kernel=kernel, env=env)
        try:
            ctx.render(2, 1)
            accum = ctx.read_accum()[..., :3]
            ctx.probe_project(capi.PROBE_RADIANCE)
            rad = ctx.read_probe_sh().astype(np.float64)
            ctx.probe_project(capi.PROBE_IRRADIANCE)
            irr = ctx.read_probe_sh().astype(np.float64)
        finally:
            ctx.close()
        assert np.abs(accum[:th] / 2.0 - colour).max() < 1e-6 and (accum[th:, 2 * tw:] == 0).all()
        # the rounding bound of the table test (tests/test_probe_host.py), times the radiance
        bound = tw * th * 2.0 ** -23 * 4.0 * np.pi * float(colour.max())
        for sh, factor in ((rad, 1.0), (irr, np.pi)):
            print("tile %d x %d factor %.3g: coefficient 0 off by %.3g, the others at most %.3g, bound %.3g" % (
                tw, th, factor, np.abs(sh[:, 0, :3] - 2.0 * np.sqrt(np.pi) * factor * colour).max(), np.abs(sh[:, 1:, :3]).max(), bound * factor))
            assert (np.abs(sh[:, 0, :3] - 2.0 * np.sqrt(np.pi) * factor * colour) <= bound * factor).all()
            assert (np.abs(sh[:, 1:, :3]) <= bound * factor).all()
            assert (sh[..., 3] == 0).all()


# ---- 6. ranks and queued renders ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [(12, 6), (16, 8)])
def test_two_partitions_equal_one_context(hiplib, tile):
    """36 x 12: the border between the 8-row strips runs inside the second row of tiles"""
    tw, th = tile
    sc, _ = atlas_scene()
    w, h = npb.image_size(N_PROBES, tw, th, PER_ROW)
    one = probe_ctx(sc, tile, accum=capi.ACCUM_REF_LDR8)
    try:
        one.render(2, 1)
        want = one.read_accum()
        got = np.zeros_like(want)
        for r in range(2):
            part = probe_ctx(sc, tile, accum=capi.ACCUM_REF_LDR8, rank=r, world=2)
            try:
                part.render(2, 1)
                rows = partition.rows_of_rank(h, r, 2)
                got[rows] = part.read_accum()[rows]
                assert part._lib.jpt_probe_project(part.h, 0) == E_STATE and b"jpt_probe_project" in part._lib.jpt_last_error(part.h)
            finally:
                part.close()
        assert np.array_equal(_u32(got), _u32(want)) and (want[..., :3] > 0).any()
    finally:
        one.close()


def test_two_queued_renders_equal_the_blocking_calls(hiplib):
    """two renders queued without a sync and the projection behind them give what the same calls give blocking"""
    tile = (12, 6)
    sc, _ = atlas_scene()

    def run(asynchronous):
        ctx = probe_ctx(sc, tile, accum=capi.ACCUM_REF_LDR8)
        try:
            ctx.render(2, 5, asynchronous=asynchronous)
            ctx.render(2, 7, asynchronous=asynchronous)
            ctx.probe_project()
            return ctx.read_accum(), ctx.read_probe_sh()
        finally:
            ctx.close()
    want, got = run(False), run(True)
    assert np.array_equal(_u32(got[0]), _u32(want[0])) and same_bits(got[1], want[1])


# ---- 7. freeing the probes means a camera render ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_renders_after_freeing_the_probes_are_the_default_bits(hiplib, kernel):
    tile = (16, 8)
    w, h = npb.image_size(N_PROBES, 16, 8, PER_ROW)
    sc = soup_scene()

    def render(probes_first):
        ctx = make_ctx(sc, None, w, h, accum=capi.ACCUM_REF_LDR8, kernel=kernel)
        try:
            probed = culled = None
            if probes_first:
                ctx.set_probes(POSITIONS, tile[0], tile[1], PER_ROW)
                ctx.render(1, 1, counted=True)
                probed, culled = ctx.read_accum(), ctx.stats()["sky_culled"]
                ctx.accum_reset()
                ctx.set_probes(None)
                assert ctx._lib.jpt_read_probes(ctx.h, host._ptr(np.zeros((5, 3), F))) == E_STATE
            ctx.render(3, 1, counted=True)
            return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes(), ctx.stats()["sky_culled"], probed, culled
        finally:
            ctx.close()
    want, got = render(False), render(True)
    assert all(np.array_equal(g, w_) for g, w_ in zip(got[:3], want[:3])) and got[3] == want[3]
    assert not np.array_equal(got[5], want[0])
    assert got[6] == 0 and got[4] == want[4]                      # a probe render culls nothing; the cull is back afterwards
    if kernel == capi.KERNEL_WAVEFRONT:
        assert want[4] > 0


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_what_a_probe_render_refuses_and_what_ignores_the_probes(hiplib):
    tile = (8, 4)
    w, h = npb.image_size(N_PROBES, 8, 4, PER_ROW)
    sc, p4, n4 = atlas(w, h)
    ctx = probe_ctx(sc, tile)
    L = ctx._lib

    def refused(word, what=b"probe"):
        assert L.jpt_render(ctx.h, 1, 1) == E_STATE
        msg = L.jpt_last_error(ctx.h).lower()
        assert word in msg and what in msg, msg
        assert L.jpt_render_async(ctx.h, 1, 1) == E_STATE
    try:
        ctx.render(1, 1)
        ctx.set_params(33, 17, 4, capi.ACCUM_HDR_F32)      # another size than the tiles make
        ctx.set_camera(scenes.camera_block(sc.camera, 33, 17))
        refused(b"24 x 8")
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
        # probes beside bake images: a bake, refused as one
        ctx.set_bake_texels(np.zeros((4, 4, 4), F), np.zeros((4, 4, 4), F))
        refused(b"4 x 4", b"bake")
        ctx.set_bake_texels(p4, n4)
        ctx.render(1, 5)
        assert L.jpt_bake_finish(ctx.h) == E_STATE and b"jpt_bake_finish" in L.jpt_last_error(ctx.h) and b"probes" in L.jpt_last_error(ctx.h)
        ctx.set_bake_texels(None, None)
        assert L.jpt_bake_finish(ctx.h) == E_STATE and b"jpt_bake_finish" in L.jpt_last_error(ctx.h)
        # the guides and picking rays are camera rays
        assert L.jpt_denoise(ctx.h) == E_STATE and b"jpt_denoise" in L.jpt_last_error(ctx.h) and b"probes" in L.jpt_last_error(ctx.h)
        xy = np.array([[3.5, 4.5]], F)
        hits = np.zeros(1, host.wire.RAY_HIT)
        assert L.jpt_query_pixels(ctx.h, host._ptr(xy), 1, host._ptr(hits)) == E_STATE and b"jpt_query_pixels" in L.jpt_last_error(ctx.h)
        ctx.set_probes(None)
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
                c2.set_probes(POSITIONS, 8, 4, PER_ROW)
            c2.set_debug_steps(True)
            c2.render(1, 1)
            steps.append(c2.read_accum())
        finally:
            c2.close()
    assert np.array_equal(steps[0], steps[1]) and (steps[0][..., :3] > 0).any()


def test_what_the_projection_refuses(hiplib):
    tile = (8, 4)
    w, h = npb.image_size(N_PROBES, 8, 4, PER_ROW)
    sc, _ = atlas_scene()
    ctx = make_ctx(sc, None, w, h)
    L = ctx._lib
    out = np.zeros((N_PROBES, 9, 4), F)

    def refused(rc, word, call=b"jpt_probe_project", code=E_STATE):
        assert rc == code, rc
        msg = L.jpt_last_error(ctx.h)
        assert call in msg and word in msg, msg
    try:
        ctx.render(1, 1)
        refused(L.jpt_probe_project(ctx.h, 0), b"no probes")
        refused(L.jpt_read_probe_sh_f32(ctx.h, host._ptr(out)), b"no jpt_probe_project", b"jpt_read_probe_sh_f32")
        ctx.set_probes(POSITIONS, 8, 4, PER_ROW)
        ctx.accum_reset()
        refused(L.jpt_probe_project(ctx.h, 0), b"no frame")
        ctx.render(1, 1)
        refused(L.jpt_probe_project(ctx.h, 2), b"flags", code=E_INVALID)
        refused(L.jpt_read_probe_sh_f32(ctx.h, host._ptr(out)), b"no jpt_probe_project", b"jpt_read_probe_sh_f32")
        ctx.set_denoising_mode(capi.DENOISE_NONE)
        refused(L.jpt_probe_project(ctx.h, 0), b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_probe_project(ctx.h, 0), b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.probe_project()
        first = ctx.read_probe_sh()
        assert (first[:, 0, :3] > 0).all()
        # another size: the projection and the read-back both refuse, and the old coefficients are not the new size's
        ctx.set_params(33, 17, 4, capi.ACCUM_HDR_F32)
        refused(L.jpt_probe_project(ctx.h, 0), b"24 x 8")
        refused(L.jpt_read_probe_sh_f32(ctx.h, host._ptr(out)), b"no jpt_probe_project", b"jpt_read_probe_sh_f32")
        ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.probe_project()
        assert same_bits(ctx.read_probe_sh(), first)
        # other probes: no projection of them yet
        ctx.set_probes(POSITIONS[:4], 8, 4, 2)
        refused(L.jpt_read_probe_sh_f32(ctx.h, host._ptr(out)), b"no jpt_probe_project", b"jpt_read_probe_sh_f32")
        assert ctx.probe_image_size() == (16, 8)
        assert not hasattr(L, "jpt_multi_probe_project")
    finally:
        ctx.close()
