"""The emitter tables of JPT_LIGHT_SAMPLING_MIS across every way a scene changes under a context: jpt_scene_update_tlas,
jpt_scene_update_reference_tlas with more and fewer emitting instances, a second jpt_scene_commit whose emitter count crosses a block
boundary or drops to zero, jpt_scene_share, a non-rigid jpt_scene_refit_tlas, and queues of refits / mesh updates and renders with
no read-back in between (one copy of the tables, rewritten while earlier renders are in flight).  The reference is a FRESH context
committed in the final state: accumulators, display images and the tables (jpt_debug_light_tables) equal it bit for bit.  Every
case runs under the gradient sky and under a map with JPT_ENV_SAMPLING_MIS."""
import copy

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import light_stress as ls
from test_gpu_light_sampling import LBRDF, LMIS, make_ctx, small_light_cornell, sun_map

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
ENVS = ["sky", "map_mis"]
KERNELS = (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT)


def ctx_for(scene, env, builder=capi.BUILD_SAH, accum=capi.ACCUM_REF_LDR8, mode=LMIS, kernel=capi.KERNEL_WAVEFRONT):
    return make_ctx(scene, W, H, builder, accum, 3, kernel, sun_map() if env == "map_mis" else None, env == "map_mis", mode)


def prepare(ctx, scene, env, mode=LMIS, accum=capi.ACCUM_REF_LDR8):
    """the per-render state of make_ctx on a context that got its scene some other way"""
    ctx.set_params(W, H, 3, accum)
    ctx.set_camera(scenes.camera_block(scene.camera, W, H))
    if env == "map_mis":
        ctx.set_environment(sun_map())
        ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
    ctx.set_light_sampling(mode)


def state(ctx, kernel=capi.KERNEL_WAVEFRONT, tables=True):
    ctx.set_kernel(kernel)
    ctx.accum_reset()
    ctx.render(2, 3)
    return (ctx.read_accum(), ctx.read_ldr()) + (tuple(ctx.debug_light_tables()) if tables else ())


def assert_state(got, want, what, first=0):
    names = ("accumulation", "display", "pairs", "tri", "cdf", "marg")[first:]
    assert len(got) == len(want)
    for g, x, name in zip(got, want, names):
        assert g.shape == x.shape, "%s: %s has shape %s, the fresh context's %s" % (what, name, g.shape, x.shape)
        differing = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(x).view(np.uint8)).sum())
        assert differing == 0, "%s: %s differs from the fresh context's in %d bytes" % (what, name, differing)


def fresh_state(scene, env, builder=capi.BUILD_SAH, kernel=capi.KERNEL_WAVEFRONT, mode=LMIS, tables=True):
    ctx = ctx_for(scene, env, builder, mode=mode)
    try:
        return state(ctx, kernel, tables)
    finally:
        ctx.close()


def with_transform(scene, i, t12):
    out = copy.deepcopy(scene)
    out.instances[i].transform = np.asarray(t12, F).copy()
    return out


def pose(scene, k):
    """the light (instance 0) moved and scaled differently along its axes: its area, so its power, changes with k"""
    t = np.asarray(scene.instances[0].transform, F).copy()
    b = t[:9].reshape(3, 3).astype(np.float64) @ np.diag([1.0 + 0.15 * k, 1.0, 0.6 + 0.1 * (k % 4)])
    t[:9] = b.reshape(-1).astype(F)
    t[9:] += np.array([0.25 * np.cos(k), -0.1 * (k % 3), 0.3 * np.sin(k)], F)
    return t


def all_transforms(scene):
    return np.stack([np.asarray(i.transform, F) for i in scene.instances])


# ---- host updates -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", ENVS)
def test_update_tlas_moving_and_stretching_the_light(hiplib, env):
    sc = small_light_cornell(0.5)
    sc2 = with_transform(sc, 0, pose(sc, 3))
    ctx = ctx_for(sc, env)
    try:
        before = state(ctx)
        ctx.set_instance_transform(0, sc2.instances[0].transform)
        ctx.update_tlas()
        for kernel in KERNELS:
            got = state(ctx, kernel)
            assert_state(got, fresh_state(sc2, env, kernel=kernel), "update_tlas, kernel %d" % kernel)
        assert not np.array_equal(got[0], before[0]) and not np.array_equal(got[5], before[5])   # the image and the total power moved
    finally:
        ctx.close()


def lights_scene(n_emitting, n_lights=3):
    """the small-light cornell box with n_lights - 1 more instances of the light's mesh, the first n_emitting of all of them with
    the light's material, the others with a non-emitting one"""
    sc = small_light_cornell(0.5)
    for j in range(1, n_lights):
        t = scenes.transform12(np.diag([0.3 + 0.1 * j, 1.0, 0.2]) @ scenes.rot_y(25.0 * j), (-1.5 + 1.2 * j, 0.5 * j, 0.4 * j))
        sc.instances.append(scenes.Instance(0, t, [1]))
    lights = [i for i in sc.instances if i.mesh == 0]
    for j, i in enumerate(lights):
        i.material_ids = [1 if j < n_emitting else 2]
    return sc


@pytest.mark.parametrize("env", ENVS)
def test_update_reference_tlas_with_more_fewer_and_no_emitting_instances(oracle, hiplib, env):
    """jpt_scene_update_reference_tlas refuses another instance count (asserted), so the emitting instances come and go with the
    material words of the instance records: two emit, then three, then two, then none -- the last equals BRDF mode"""
    def upload(ctx, r):
        ctx.upload_reference_layout(r.tri_geom, r.tri_data, r.materials, r.bvh_nodes, r.instances, r.tlas_nodes, r.textures)

    def fresh(sc, mode=LMIS):
        c = host.Context(0)
        try:
            upload(c, oracle.build_scene(sc))
            prepare(c, sc, env, mode)
            return state(c, tables=mode == LMIS)
        finally:
            c.close()

    steps = [lights_scene(2), lights_scene(3), lights_scene(2), lights_scene(0)]
    ctx = host.Context(0)
    try:
        upload(ctx, oracle.build_scene(steps[0]))
        prepare(ctx, steps[0], env)
        first = state(ctx)
        assert len(first[2]) == 4
        other = oracle.build_scene(lights_scene(2, n_lights=4))
        with pytest.raises(capi.JptError, match="instance count changed"):
            ctx.update_reference_tlas(other.instances, other.tlas_nodes)
        assert_state(state(ctx), first, "after the refused update")
        for k, (sc, n_emitting) in enumerate(zip(steps[1:], (3, 2, 0))):
            r = oracle.build_scene(sc)
            ctx.update_reference_tlas(r.instances, r.tlas_nodes)
            got = state(ctx)
            assert len(got[2]) == 2 * n_emitting
            assert_state(got, fresh(sc), "update_reference_tlas step %d" % k)
        assert_state(got[:2], fresh(steps[-1], LBRDF), "no emitting instance: BRDF mode")
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ENVS)
def test_commits_on_one_context_across_block_boundaries_and_zero(hiplib, env):
    """300, 100, 0 and 300 emitters again on one context: the tables shrink below a block, vanish and come back"""
    ctx = host.Context(0)
    try:
        for n in (300, 100, 0, 300):
            sc = ls.edges_scene(n)
            ctx.build_scene(sc, capi.BUILD_SAH)
            prepare(ctx, sc, env)
            got = state(ctx)
            assert len(got[2]) == n
            assert_state(got, fresh_state(sc, env), "commit of %d emitters" % n)
            if n == 0:
                assert_state(got[:2], fresh_state(sc, env, mode=LBRDF, tables=False), "no emitter: BRDF mode")
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ENVS)
def test_shared_scene_renders_the_source_and_ignores_its_later_updates(hiplib, env):
    sc = small_light_cornell(0.5)
    src = ctx_for(sc, env)
    dst = host.Context(0)
    try:
        want = state(src)
        dst.share_scene_from(src)
        prepare(dst, sc, env)
        assert_state(state(dst), want, "shared scene")
        src.set_instance_transform(0, pose(sc, 2))
        src.update_tlas()
        moved = state(src)
        assert not np.array_equal(moved[0], want[0])
        assert_state(state(dst), want, "shared scene after the source's update_tlas")
        assert_state(moved, fresh_state(with_transform(sc, 0, pose(sc, 2)), env), "the source after its update_tlas")
    finally:
        src.close()
        dst.close()


# ---- device refits ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", ENVS)
def test_non_rigid_refit_equals_a_fresh_commit(hiplib, env):
    sc = small_light_cornell(0.5)
    sc2 = with_transform(sc, 0, pose(sc, 5))
    ctx = ctx_for(sc, env, capi.BUILD_SAH_WATERTIGHT)
    try:
        before = state(ctx)
        ctx.refit_tlas(all_transforms(sc2))
        got = state(ctx)
        assert_state(got, fresh_state(sc2, env, capi.BUILD_SAH_WATERTIGHT), "non-rigid refit")
        assert not np.array_equal(got[5], before[5])
    finally:
        ctx.close()


N_STEPS = 10


def light_mesh(scene, k):
    """the light's mesh with its vertices stretched and moved: another area with every k"""
    m = copy.deepcopy(scene.meshes[scene.instances[0].mesh])
    for s in m.surfaces:
        s.vertices[:] = (s.vertices * np.array([0.5 + 0.12 * k, 1.0, 1.4 - 0.09 * k], F) + np.array([0.1 * k, 0.0, -0.05 * k], F)).astype(F)
    return m


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("step", ["refit_tlas", "update_mesh"])
def test_queued_steps_and_renders_equal_the_blocking_sequence(hiplib, step, env):
    """Ten times `refit_tlas(pose_k)` (or `update_mesh(light, shape_k)`), `render(1, frame_k, asynchronous=True)` with nothing in
    between -- no reset, read-back or synchronisation: more steps than there are copies of the instance records (eight) or
    pipeline slots, every one of which rewrites the one copy of the emitter tables while earlier renders may be in flight.
    After ONE read at the end the HDR sum equals, bit for bit, the same sequence rendered blocking on another context, and the
    tables equal a fresh commit's at the last pose.
    Mutation tried (not committed): without the lights_stale call in queue_instance_refit the tables keep the first pose's power
    and geometry; these four tests and test_non_rigid_refit_equals_a_fresh_commit (both environments) then fail: six of this
    file's fourteen (and the two blocking cases of test_gpu_light_sampling.py).  Measured on an MI355X: 0 differing bytes."""
    sc = small_light_cornell(0.5)
    assert sum(1 for i in sc.instances if i.mesh == sc.instances[0].mesh) == 1

    def apply(ctx, k):
        if step == "refit_tlas":
            ctx.refit_tlas(all_transforms(with_transform(sc, 0, pose(sc, k))))
        else:
            ctx.update_mesh(sc.instances[0].mesh, light_mesh(sc, k), with_normals=False)

    queued = ctx_for(sc, env, capi.BUILD_SAH_WATERTIGHT, capi.ACCUM_HDR_F32)
    blocking = ctx_for(sc, env, capi.BUILD_SAH_WATERTIGHT, capi.ACCUM_HDR_F32)
    try:
        for k in range(1, N_STEPS + 1):
            apply(queued, k)
            queued.render(1, k, asynchronous=True)
        for k in range(1, N_STEPS + 1):
            apply(blocking, k)
            blocking.render(1, k)
        got = (queued.read_accum(), queued.read_ldr()) + tuple(queued.debug_light_tables())
        want = (blocking.read_accum(), blocking.read_ldr()) + tuple(blocking.debug_light_tables())
        assert_state(got, want, "queued %s" % step)
        if step == "refit_tlas":
            last = with_transform(sc, 0, pose(sc, N_STEPS))
        else:
            last = copy.deepcopy(sc)
            last.meshes[sc.instances[0].mesh] = light_mesh(sc, N_STEPS)
        fresh = ctx_for(last, env, capi.BUILD_SAH_WATERTIGHT, capi.ACCUM_HDR_F32)
        try:
            assert_state(got[2:], tuple(fresh.debug_light_tables()), "tables after the queue", first=2)
        finally:
            fresh.close()
    finally:
        queued.close()
        blocking.close()
