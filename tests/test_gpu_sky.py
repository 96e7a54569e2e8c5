"""The procedural sky on the device (jpt_set_sky): the kernel against the numpy restatement (tests/np_sky.py) and the host loop bit for
bit, the context's map read back, renders under a sky against renders under the same texels uploaded (every bit of accumulation,
display and depth; both kernels, both sampling modes in both orders, a bake and a probe render), a sky changed between queued renders,
replacing and clearing, and the multi form.  Renders: scenes.demo_scene(n_tris=4096) at 64 x 48, 2 frames, JPT_ACCUM_HDR_F32."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_probe as npb
import np_sky as ns
from test_bake_host import SIZES as BAKE_SIZES, ray_images
from test_gpu_environment import ROT, assert_same, images
from test_probe_host import PER_ROW, TILES
from test_sky_host import HOST_ONLY, SIZES, SUN_SETS, SUNS, hard_params

pytestmark = pytest.mark.gpu

F = np.float32
E_STATE = -4   # JPT_E_STATE
W, H = 64, 48
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)
INTENSITY = 2.5
# the skies of the render tests: Godot's defaults with a sun that lights the scene from the side, and a second one that differs everywhere
SKY_1 = ns.params(suns=[dict(direction=(0.5, 0.6, 0.4), angular_radius=0.08, color=(1.0, 0.9, 0.7), energy=30.0)])
SKY_2 = ns.params(sky_top_color=(0.9, 0.3, 0.1), ground_bottom_color=(0.0, 0.2, 0.4), sky_energy=1.5,
                  suns=[dict(direction=(-0.4, 0.3, 0.7), angular_radius=0.12, color=(0.6, 0.8, 1.0), energy=3.0, mode=ns.SUN_IRRADIANCE)])
MAP_W, MAP_H, MAP_N = 64, 32, 2
PROBE_POSITIONS = np.array([(0.0, 0.5, 4.0), (2.5, 1.0, -1.0), (-3.0, -1.0, 0.5), (0.3, 3.5, 0.2), (0.4, -1.9, 0.3)], F)


@pytest.fixture(scope="module")
def scene():
    return scenes.demo_scene(n_tris=4096)


def make_ctx(scene, kernel=capi.KERNEL_WAVEFRONT, w=W, h=H):
    ctx = host.Context(0)
    try:
        ctx.build_scene(scene, capi.BUILD_SAH)
        ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
        ctx.set_kernel(kernel)
        ctx.set_camera(scenes.camera_block(scene.camera, w, h))
        ctx.set_environment_params(ROT, INTENSITY)
    except Exception:
        ctx.close()
        raise
    return ctx


def set_sky(ctx, p, w=MAP_W, h=MAP_H, n=MAP_N):
    ctx.set_sky(ns.lib_params(p), w, h, n)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_suns", sorted(SUN_SETS))
def test_device_sky_equals_numpy_and_the_host_loop(hiplib, n_suns):
    p = ns.params(suns=SUN_SETS[n_suns])
    for w, h, n in SIZES + ((300, 2, 2), (1, 7, 3)):                 # (300 x 2, 1 x 7: a block's tail, a row of one texel)
        got = host.debug_sky(0, ns.lib_params(p), w, h, n)
        assert ns.same_bits(got, ns.sky_map(p, w, h, n)), (w, h, n)
        assert ns.same_bits(got, host.debug_sky(HOST_ONLY, ns.lib_params(p), w, h, n)), (w, h, n)
    assert ns.same_bits(host.debug_sky(0, ns.lib_params(hard_params()), 37, 19, 2), ns.sky_map(hard_params(), 37, 19, 2))
    assert ns.same_bits(host.debug_sky(0, None, 64, 32, 1), ns.sky_map(ns.params(), 64, 32, 1))


# ---- 2. through the context ----------------------------------------------------------------------------------------------------------------------

def test_the_context_holds_the_map_and_reads_it_back(hiplib):
    ctx = host.Context(0)
    try:
        w, h = host.C.c_int32(7), host.C.c_int32(7)
        assert ctx._lib.jpt_read_environment_f32(ctx.h, None, host.C.byref(w), host.C.byref(h)) == E_STATE
        assert "no environment map" in ctx.last_error()
        with pytest.raises(capi.JptError, match="jpt_read_environment_f32"):
            ctx.read_environment()
        p = ns.params(suns=SUNS)
        set_sky(ctx, p, 37, 19, 2)
        assert ns.same_bits(ctx.read_environment(), ns.sky_map(p, 37, 19, 2))
        set_sky(ctx, SKY_1, 37, 19, 3)                                 # the same size: written in place
        assert ns.same_bits(ctx.read_environment(), ns.sky_map(SKY_1, 37, 19, 3))
        ctx.set_sky()                                                   # the defaults, 2048 x 1024, samples 4
        got = ctx.read_environment()
        assert got.shape == (1024, 2048, 3)
        assert ns.same_bits(got, host.debug_sky(0, None, 2048, 1024, 4))
        rng = np.random.default_rng(4)
        rgb = rng.uniform(0.0, 4.0, (9, 21, 3)).astype(F)
        ctx.set_environment(rgb)
        assert ns.same_bits(ctx.read_environment(), rgb)
        assert ctx._lib.jpt_read_environment_f32(ctx.h, None, host.C.byref(w), host.C.byref(h)) == capi.OK and (w.value, h.value) == (21, 9)
        ctx.set_environment(None)
        with pytest.raises(capi.JptError, match="jpt_read_environment_f32"):
            ctx.read_environment()
    finally:
        ctx.close()


# ---- 3. a sky renders as its texels, uploaded, render ----------------------------------------------------------------------------------------------

def render_pair(a, b, what):
    a.render(2, 1)
    b.render(2, 1)
    ia, ib = images(a), images(b)
    assert_same(ia, ib, what)
    return ia


@pytest.mark.parametrize("mode", ("brdf", "mis, mode first", "mis, sky first"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_sky_renders_as_the_same_texels_uploaded(hiplib, scene, kernel, mode):
    a, b = make_ctx(scene, kernel), make_ctx(scene, kernel)
    try:
        if mode == "mis, mode first":
            a.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        set_sky(a, SKY_1)
        if mode == "mis, sky first":
            a.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        b.set_environment(a.read_environment())
        if mode != "brdf":
            b.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        lit = render_pair(a, b, mode)
        # and the sky is what lights the image: without it the accumulation differs
        c = make_ctx(scene, kernel)
        try:
            c.render(2, 1)
            assert (c.read_accum() != lit[0]).any()
        finally:
            c.close()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("form", ("bake", "probe"))
def test_a_sky_lights_bake_and_probe_renders_as_the_same_texels_uploaded(hiplib, scene, form):
    if form == "bake":
        w, h = BAKE_SIZES[-1]                                         # 33 x 17
    else:
        w, h = npb.image_size(len(PROBE_POSITIONS), TILES[0][0], TILES[0][1], PER_ROW)
    a, b = make_ctx(scene, w=w, h=h), make_ctx(scene, w=w, h=h)
    try:
        for ctx in (a, b):
            if form == "bake":
                ctx.set_bake_texels(*ray_images(w, h))
            else:
                ctx.set_probes(PROBE_POSITIONS, TILES[0][0], TILES[0][1], PER_ROW)
            ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        set_sky(a, SKY_1)
        b.set_environment(a.read_environment())
        a.render(2, 1)
        b.render(2, 1)
        got, want = a.read_accum(), b.read_accum()
        assert ns.same_bits(got, want) and got[..., :3].any()
    finally:
        a.close()
        b.close()


# ---- 4. ordering -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mis", (False, True))
def test_a_sky_changed_between_queued_renders(hiplib, scene, mis):
    """Sky 1, frames 1-2 queued, sky 2 at the same size (the kernel goes on the context's stream, no wait on the host in BRDF mode),
    frames 3-4 queued: the accumulation is the one blocking renders give with the two maps uploaded.  That the second jpt_set_sky returns
    with work still queued is not asserted: at this size a render is over in well under a millisecond, and nothing the library exposes
    tells reliably whether it was still in flight -- the images are what is checked (a sky written too early or too late changes them)."""
    maps = [host.debug_sky(0, ns.lib_params(p), MAP_W, MAP_H, MAP_N) for p in (SKY_1, SKY_2)]
    a, b = make_ctx(scene), make_ctx(scene)
    try:
        if mis:
            a.set_environment_sampling(capi.ENV_SAMPLING_MIS)
            b.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        set_sky(a, SKY_1)
        a.render(2, 1, asynchronous=True)
        set_sky(a, SKY_2)
        a.render(2, 3, asynchronous=True)
        a.sync()
        b.set_environment(maps[0])
        b.render(2, 1)
        b.set_environment(maps[1])
        b.render(2, 3)
        assert_same(images(a), images(b), "sky changed between queued renders")
        assert ns.same_bits(a.read_environment(), maps[1])
    finally:
        a.close()
        b.close()


# ---- 5. replace and clear ------------------------------------------------------------------------------------------------------------------------

def test_clearing_and_replacing_a_sky(hiplib, scene):
    a, b, fresh = make_ctx(scene), make_ctx(scene), make_ctx(scene)
    try:
        set_sky(a, SKY_1)
        a.render(2, 1)
        a.set_environment(None)
        a.accum_reset()
        a.render(2, 1)
        fresh.render(2, 1)
        assert_same(images(a), images(fresh), "set_sky, then cleared: the gradient")
        for size in ((MAP_W, MAP_H, 1), (96, 40, 3)):                  # back from no map, then another size: both allocate
            set_sky(a, SKY_2, *size)
            b.set_environment(a.read_environment())
            a.accum_reset()
            b.accum_reset()
            render_pair(a, b, "a sky of %r" % (size,))
        rng = np.random.default_rng(8)
        rgb = rng.uniform(0.0, 2.0, (16, 32, 3)).astype(F)
        a.set_environment(rgb)                                          # an uploaded map replaces the sky
        b.set_environment(rgb)
        a.accum_reset()
        b.accum_reset()
        render_pair(a, b, "replaced by an uploaded map")
    finally:
        a.close()
        b.close()
        fresh.close()


# ---- 6. the multi form ---------------------------------------------------------------------------------------------------------------------------

def test_multi_set_sky_on_one_device_equals_the_context(hiplib, scene):
    one = make_ctx(scene)
    m = host.MultiContext([0])
    try:
        m.build_scene(scene)
        m.set_params(W, H, 4, capi.ACCUM_HDR_F32)
        m.set_camera(scenes.camera_block(scene.camera, W, H))
        m.set_environment_params(ROT, INTENSITY)
        m.set_sky(ns.lib_params(SKY_1), MAP_W, MAP_H, MAP_N)
        set_sky(one, SKY_1)
        one.render(2, 1)
        m.render(2, 1)
        assert np.array_equal(m.read_accum(), one.read_accum())
        assert np.array_equal(m.read_ldr(), one.read_ldr())
        with pytest.raises(capi.JptError, match="samples"):
            m.set_sky(None, MAP_W, MAP_H, 9)
    finally:
        m.close()
        one.close()
