"""The transmission flag (JPT_MATERIAL_EXT_TRANSMISSION) across every way a scene changes under a context.  Whether a render takes
the *_tx kernels is decided by a scan of the context's materials (lights_stale), reached from jpt_scene_commit, jpt_scene_share,
jpt_scene_upload_reference_layout and the TLAS updates but not from the device refits: a second commit with and without glass,
sharing into a context whose flag was set before or after, moving and stretching the glass block (jpt_scene_update_tlas, a
non-rigid jpt_scene_refit_tlas), deforming it (jpt_scene_update_mesh, the glass emissive too), queues of refits / mesh updates
and renders with no read-back in between, and the multi-context upload with a lens.  The yardstick is a FRESH context committed
with the final scene: accumulation and display equal it bit for bit.  Every case runs under the gradient sky and under a map with
both kinds of MIS."""
import copy

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

from test_gpu_transmission import sun_map

pytestmark = pytest.mark.gpu

F = np.float32
TX = capi.MATERIAL_EXT_TRANSMISSION
W, H, BOUNCES, FRAMES = 64, 48, 4, 2
LIGHTINGS = ["sky", "map_mis_emitters"]
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)
BLOCK = 2          # glass_cornell_scene's glass block: its instance and its mesh
LENS = (0.12, 9.0)


def prepare(ctx, scene, lighting, flags=TX, accum=capi.ACCUM_REF_LDR8, lens=None):
    """the per-render state, on a context that got or will get its scene some way"""
    ctx.set_params(W, H, BOUNCES, accum)
    ctx.set_camera(scenes.camera_block(scene.camera, W, H))
    if lighting.startswith("map"):
        ctx.set_environment(sun_map())
        ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
    if "emitters" in lighting:
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
    if flags is not None:
        ctx.set_material_extensions(flags)
    if lens is not None:
        ctx.set_lens(*lens)


def ctx_for(scene, lighting, builder=capi.BUILD_SAH, flags=TX, accum=capi.ACCUM_REF_LDR8):
    ctx = host.Context(0)
    try:
        ctx.build_scene(scene, builder)
        prepare(ctx, scene, lighting, flags, accum)
    except Exception:
        ctx.close()
        raise
    return ctx


def state(ctx, kernel=capi.KERNEL_WAVEFRONT):
    ctx.set_kernel(kernel)
    ctx.accum_reset()
    ctx.render(FRAMES, 1)
    return ctx.read_accum(), ctx.read_ldr()


def fresh_state(scene, lighting, builder=capi.BUILD_SAH, kernel=capi.KERNEL_WAVEFRONT, flags=TX):
    ctx = ctx_for(scene, lighting, builder, flags)
    try:
        return state(ctx, kernel)
    finally:
        ctx.close()


def differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


def share(a, b):
    return 100.0 * differing(a[0], b[0]) / (W * H)


def assert_state(got, want, what):
    n = [differing(g, x) for g, x in zip(got, want)]
    print("%s: %d accumulation and %d display pixels differ from the yardstick" % (what, n[0], n[1]))
    assert n == [0, 0], "%s: accumulation differs at %d pixels, display at %d" % (what, n[0], n[1])


def with_transform(scene, i, t12):
    out = copy.deepcopy(scene)
    out.instances[i].transform = np.asarray(t12, F).copy()
    return out


def with_mesh(scene, mesh_id, mesh):
    out = copy.deepcopy(scene)
    out.meshes[mesh_id] = mesh
    return out


def all_transforms(scene):
    return np.stack([np.asarray(i.transform, F) for i in scene.instances])


def pose(scene, k):
    """the glass block moved about the box and stretched differently along its axes (k = 0: as committed)"""
    t = np.asarray(scene.instances[BLOCK].transform, F).copy()
    b = t[:9].reshape(3, 3).astype(np.float64) @ np.diag([1.0 + 0.08 * k, 1.0 + 0.05 * (k % 3), 1.0 - 0.04 * k])
    t[:9] = b.reshape(-1).astype(F)
    t[9:] += np.array([-0.12 * k, 0.03 * k, 0.1 * np.sin(k)], F)
    return t


def block_mesh(scene, k, uniform=False):
    """the block's mesh with vertices and normals scaled (k = 0: as committed); uniform: by the same power of two along every axis,
    which scales every area the builder compares by one exact factor -- the fresh commit's tree, so its emitter order, is the
    committed one's"""
    m = copy.deepcopy(scene.meshes[scene.instances[BLOCK].mesh])
    s = np.full(3, 0.5 if k % 2 else 1.0) if uniform else np.array([1.0 + 0.06 * k, 1.0 - 0.03 * k, 0.8 + 0.05 * (k % 4)])
    for surf in m.surfaces:
        surf.vertices[:] = (surf.vertices * s.astype(F)).astype(F)
        surf.normals[:] = (surf.normals / s.astype(F) * F(1.0 + 0.1 * k)).astype(F)
    return m


def glowing_glass_scene():
    """glass_cornell_scene with a block that transmits, reflects and emits: its twelve triangles are in the emitter tables"""
    sc = scenes.glass_cornell_scene()
    sc.materials = sc.materials.copy()
    sc.materials[-1] = scenes.material(albedo=(0.9, 0.95, 1.0), emission=(0.9, 0.6, 0.3), energy=3.0, transmission=0.6, ior=1.5)
    return sc


# ---- commits and sharing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", LIGHTINGS)
def test_commits_with_and_without_glass_on_one_context(hiplib, lighting):
    """glass, the plain box, glass again, the flag set once: the *_tx kernels, the plain family, the *_tx kernels"""
    glass, plain = scenes.glass_cornell_scene(), scenes.cornell_scene()
    ctx = host.Context(0)
    try:
        ctx.build_scene(glass, capi.BUILD_SAH)
        prepare(ctx, glass, lighting)
        first = state(ctx)
        assert_state(first, fresh_state(glass, lighting), "first commit, glass")
        ctx.build_scene(plain, capi.BUILD_SAH)
        middle = state(ctx)
        print("the flag over glass changed %.1f %% of the pixels" % share(first, middle))
        assert share(first, middle) > 0.0
        assert_state(middle, fresh_state(plain, lighting), "second commit, no glass")
        assert_state(middle, fresh_state(plain, lighting, flags=capi.MATERIAL_EXT_NONE), "second commit against a flag-off render")
        ctx.build_scene(glass, capi.BUILD_SAH)
        assert_state(state(ctx), first, "third commit, glass again")
    finally:
        ctx.close()


@pytest.mark.parametrize("lighting", LIGHTINGS)
def test_shared_glass_renders_the_source_and_ignores_its_later_commit(hiplib, lighting):
    sc = scenes.glass_cornell_scene()
    src = ctx_for(sc, lighting)
    before, after = host.Context(0), host.Context(0)
    try:
        want = state(src)
        off = fresh_state(sc, lighting, flags=capi.MATERIAL_EXT_NONE)
        print("the flag changed %.1f %% of the pixels" % share(want, off))
        assert share(want, off) > 0.0
        before.set_material_extensions(TX)
        before.share_scene_from(src)
        prepare(before, sc, lighting, flags=None)
        after.share_scene_from(src)
        prepare(after, sc, lighting)
        assert_state(state(before), want, "flag set before the share")
        assert_state(state(after), want, "flag set after the share")
        plain = scenes.cornell_scene()
        src.build_scene(plain, capi.BUILD_SAH)
        assert_state(state(src), fresh_state(plain, lighting), "the source after its commit of the plain box")
        assert_state(state(before), want, "flag set before the share, after the source's commit")
        assert_state(state(after), want, "flag set after the share, after the source's commit")
    finally:
        src.close()
        before.close()
        after.close()


# ---- moving and deforming the glass -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", LIGHTINGS)
@pytest.mark.parametrize("how", ["update_tlas", "refit_tlas"])
def test_moving_the_glass_block_equals_a_fresh_commit(hiplib, how, lighting):
    sc = scenes.glass_cornell_scene()
    sc2 = with_transform(sc, BLOCK, pose(sc, 4))
    builder = capi.BUILD_SAH if how == "update_tlas" else capi.BUILD_SAH_WATERTIGHT
    ctx = ctx_for(sc, lighting, builder)
    try:
        first = state(ctx)
        if how == "update_tlas":
            ctx.set_instance_transform(BLOCK, sc2.instances[BLOCK].transform)
            ctx.update_tlas()
        else:
            # (a device refit serves the default kernel only; the jpt_scene_update_tlas behind it brings the other records up to date)
            ctx.refit_tlas(all_transforms(sc2))
            assert_state(state(ctx), fresh_state(sc2, lighting, builder), "refit_tlas, before update_tlas")
            ctx.update_tlas()
        for kernel in KERNELS:
            got = state(ctx, kernel)
            assert_state(got, fresh_state(sc2, lighting, builder, kernel), "%s, kernel %d" % (how, kernel))
        print("the move changed %.1f %% of the pixels" % share(got, first))
        assert share(got, first) > 0.0
        off = fresh_state(sc2, lighting, builder, flags=capi.MATERIAL_EXT_NONE)
        print("the flag changed %.1f %% of the pixels" % share(got, off))
        assert share(got, off) > 0.0
    finally:
        ctx.close()


@pytest.mark.parametrize("lighting", LIGHTINGS)
@pytest.mark.parametrize("which", ["glass", "glowing_glass"])
def test_deforming_the_glass_block_equals_a_fresh_commit(hiplib, which, lighting):
    sc = scenes.glass_cornell_scene() if which == "glass" else glowing_glass_scene()
    mesh_id = sc.instances[BLOCK].mesh
    assert sum(1 for i in sc.instances if i.mesh == mesh_id) == 1
    new = block_mesh(sc, 3, uniform=which == "glowing_glass")
    sc2 = with_mesh(sc, mesh_id, new)
    ctx = ctx_for(sc, lighting, capi.BUILD_SAH_WATERTIGHT)
    try:
        first = state(ctx)
        ctx.update_mesh(mesh_id, new, with_normals=True)
        got = state(ctx)   # (a deformed mesh serves the default kernel only)
        assert_state(got, fresh_state(sc2, lighting, capi.BUILD_SAH_WATERTIGHT), "update_mesh of the %s block" % which)
        print("the deformation changed %.1f %% of the pixels" % share(got, first))
        assert share(got, first) > 0.0
        off = fresh_state(sc2, lighting, capi.BUILD_SAH_WATERTIGHT, flags=capi.MATERIAL_EXT_NONE)
        print("the flag changed %.1f %% of the pixels" % share(got, off))
        assert share(got, off) > 0.0
    finally:
        ctx.close()


N_STEPS = 10


@pytest.mark.parametrize("lighting", LIGHTINGS)
@pytest.mark.parametrize("step", ["refit_tlas", "update_mesh"])
def test_queued_steps_and_renders_of_glass_equal_the_blocking_sequence(hiplib, step, lighting):
    """Ten times `refit_tlas(pose_k)` (or `update_mesh(block, shape_k)`), `render(1, k, asynchronous=True)` with nothing in between,
    read once at the end: the HDR sum and the display equal the same sequence rendered blocking on another context, and differ from
    the sequence with the flag off"""
    sc = scenes.glass_cornell_scene()
    mesh_id = sc.instances[BLOCK].mesh

    def apply(ctx, k):
        if step == "refit_tlas":
            ctx.refit_tlas(all_transforms(with_transform(sc, BLOCK, pose(sc, k))))
        else:
            ctx.update_mesh(mesh_id, block_mesh(sc, k), with_normals=True)

    def run(asynchronous, flags=TX):
        ctx = ctx_for(sc, lighting, capi.BUILD_SAH_WATERTIGHT, flags, capi.ACCUM_HDR_F32)
        try:
            for k in range(1, N_STEPS + 1):
                apply(ctx, k)
                ctx.render(1, k, asynchronous=asynchronous)
            return ctx.read_accum(), ctx.read_ldr()
        finally:
            ctx.close()
    want, got = run(False), run(True)
    assert_state(got, want, "queued %s" % step)
    off = run(False, capi.MATERIAL_EXT_NONE)
    print("the flag changed %.1f %% of the pixels" % share(want, off))
    assert share(want, off) > 0.0


# ---- the multi-context upload -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", LIGHTINGS)
def test_multi_context_upload_of_glass_with_a_lens_equals_one_context(oracle, hiplib, lighting):
    sc = scenes.glass_cornell_scene()
    r = oracle.build_scene(sc)
    arrays = (r.tri_geom, r.tri_data, r.materials, r.bvh_nodes, r.instances, r.tlas_nodes, r.textures)
    one, m = host.Context(0), host.MultiContext([0, 0])
    try:
        for c in (one, m):
            c.upload_reference_layout(*arrays)
            prepare(c, sc, lighting, lens=LENS)
        one.render(FRAMES, 1)
        m.render(FRAMES, 1)
        got, want = (m.read_accum(), m.read_ldr()), (one.read_accum(), one.read_ldr())
        assert_state(got, want, "two ranks")
        for what, kw in (("flag", dict(flags=capi.MATERIAL_EXT_NONE, lens=LENS)), ("lens", dict(lens=(0.0, 1.0)))):
            prepare(one, sc, lighting, **kw)
            one.accum_reset()
            one.render(FRAMES, 1)
            other = (one.read_accum(), one.read_ldr())
            print("the %s changed %.1f %% of the pixels" % (what, share(want, other)))
            assert share(want, other) > 0.0
    finally:
        m.close()
        one.close()
