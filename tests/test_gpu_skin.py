"""jpt_scene_pose_mesh on the device: the skin kernel against the numpy restatement (tests/np_skin.py), bit for bit, and a posed mesh
against the two independent routes to the same scene -- jpt_scene_update_mesh with vertices np_skin computed, and a fresh
JPT_BUILD_SAH_WATERTIGHT commit of the posed mesh: records, images and counted rays are equal."""
import copy

import numpy as np
import pytest

import np_skin
from gdpathtracing_amd import capi, host, scenes

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_STATE = -1, -4
W, H, SPP, BOUNCES = 64, 48, 2, 2
TUBE, FLOOR, SPARE = 0, 1, 2
N_BONES = 6


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the kernel alone -------------------------------------------------------------------------------------------------------

def test_device_kernel_equals_numpy_bit_for_bit(hiplib):
    """every case of the host test, palettes of 1, 3 and MANY_BONES bones among them"""
    cases = np_skin.debug_cases()
    assert any(c["palette"] is not None and len(c["palette"]) == np_skin.MANY_BONES for _, c in cases)
    for label, c in cases:
        r = c["rig"]
        want_p, want_n = np_skin.np_skin(c["pos"], c["nrm"], r.bones, r.weights, c["K"], r.position_deltas, r.normal_deltas, c["palette"], c["blend"])
        got_p, got_n = host.debug_skin(0, c["pos"], c["nrm"], host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas), c["K"], c["S"],
                                       c["palette"], c["blend"])
        assert np.array_equal(bits(got_p), bits(want_p)), label
        if want_n is not None:
            assert np.array_equal(bits(got_n), bits(want_n)), label


# ---- the small scene --------------------------------------------------------------------------------------------------------

def _tube_surface(x0, x1, rings, sides, cap):
    t = np.linspace(x0, x1, rings)
    a = np.arange(sides) * (2 * np.pi / sides)
    cy = 0.3 * np.sin(1.5 * t)
    p = np.stack([np.repeat(t, sides), np.repeat(cy, sides) + 0.25 * np.tile(np.cos(a), rings), 0.25 * np.tile(np.sin(a), rings)], axis=1)
    n = np.stack([np.zeros(rings * sides), np.tile(np.cos(a), rings), np.tile(np.sin(a), rings)], axis=1)
    idx = []
    for r in range(rings - 1):
        for s in range(sides):
            i0, i1 = r * sides + s, r * sides + (s + 1) % sides
            idx += [i0, i1 + sides, i0 + sides, i0, i1, i1 + sides]
    if cap:   # one more vertex closing the first ring
        p = np.concatenate([p, [[x0, cy[0], 0.0]]])
        n = np.concatenate([n, [[-1.0, 0.0, 0.0]]])
        for s in range(sides):
            idx += [rings * sides, (s + 1) % sides, s]
    uv = np.stack([p[:, 0], p[:, 1]], axis=1)
    return scenes.Surface(p.astype(F), n.astype(F), uv.astype(F), np.array(idx, np.int32))


def small_scene():
    """a bent tube of two surfaces (193 and 70 vertices, 502 triangles) named by two instances, a floor, and a mesh no instance names"""
    tube = scenes.Mesh([_tube_surface(-1.2, 0.4, 24, 8, True), _tube_surface(0.4, 1.2, 10, 7, False)])
    assert [len(s.vertices) for s in tube.surfaces] == [193, 70]
    mats = np.stack([scenes.material(), scenes.material(albedo=(1.0, 0.2, 0.2)), scenes.material(albedo=(0.3, 1.0, 0.2), roughness=0.5),
                     scenes.material(albedo=(0.8, 0.8, 0.8)), scenes.material(emission=(1.0, 0.9, 0.7), energy=6.0)])
    inst = [scenes.Instance(TUBE, scenes.transform12(None, (0.0, 0.6, 0.0)), [1, 2]),
            scenes.Instance(TUBE, scenes.transform12(scenes.rot_y(70.0), (0.2, 1.4, -0.8)), [2, 4]),
            scenes.Instance(FLOOR, scenes.transform12(np.eye(3) * 3.0, (0.0, 0.0, 0.0)), [3])]
    return scenes.Scene("tube", [tube, scenes.plane_mesh(), scenes.box_mesh(1.0, 1.0, 1.0)], inst, mats,
                        scenes.CameraDesc(scenes.transform12(None, (0.0, 0.9, 3.2))))


def tube_rigs(mesh, K=4, S=2, normal_deltas=True, convex=False, seed=11):
    """bones spread along x, each vertex bound to the K nearest by random weights; convex: weights from {0, 0.25, 0.5, 1} summing to 1"""
    rng = np.random.RandomState(seed)
    out = []
    for s in mesh.surfaces:
        nv = len(s.vertices)
        r = np_skin.random_rig(rng, nv, K, S, N_BONES, normal_deltas=normal_deltas)
        if K:
            centre = np.clip(((s.vertices[:, 0] + 1.2) / 2.4 * (N_BONES - 1)).astype(int), 0, N_BONES - 1)
            r.bones = ((centre[:, None] + np.arange(K)[None, :]) % N_BONES).astype(np.int32)
            if convex:
                sets = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.5, 0.25, 0.25, 0], [0.25, 0.25, 0.25, 0.25], [0, 1, 0, 0], [0.25, 0, 0.5, 0.25]], F)
                r.weights = sets[rng.randint(0, len(sets), nv)]
        if S:
            r.position_deltas = (r.position_deltas * F(0.3)).astype(F)
        out.append(r)
    return out


def host_rigs(rigs):
    return [host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas) for r in rigs]


def pose(k, n_bones=N_BONES, amount=0.25):
    rng = np.random.RandomState(100 + k)
    pal = np_skin.random_palette(rng, n_bones, amount)
    return pal, np.array([[0.7, 0.0], [0.0, -0.5], [1.2, 0.4], [0.3, 0.9]], F)[k % 4]


IDENTITY = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(F), (N_BONES, 1))


def with_mesh(scene, mesh_id, mesh):
    sc = copy.copy(scene)
    sc.meshes = list(scene.meshes)
    sc.meshes[mesh_id] = mesh
    return sc


def make_ctx(scene, w=W, h=H, bounces=BOUNCES):
    ctx = host.Context(0)
    ctx.build_scene(scene, capi.BUILD_SAH_WATERTIGHT)
    ctx.set_params(w, h, bounces)
    ctx.set_camera(scenes.camera_block(scene.camera, w, h))
    return ctx


def counted_frame(ctx, spp=SPP):
    ctx.accum_reset()
    ctx.render(spp, 1, counted=True)
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.stats()["rays"]


def fresh(scene, w=W, h=H, spp=SPP, bounces=BOUNCES):
    ctx = make_ctx(scene, w, h, bounces)
    try:
        return counted_frame(ctx, spp)
    finally:
        ctx.close()


def assert_same(got, want, what):
    for g, x, name in zip(got[:3], want[:3], ("accumulation", "display", "depth")):
        bad = ~((g == x) | (np.isnan(g) & np.isnan(x)))
        assert not bad.any(), "%s: %s differs at %d elements" % (what, name, int(bad.sum()))
    if len(got) > 3 and len(want) > 3:
        assert got[3] == want[3], "%s: counted rays %s / %s" % (what, got[3], want[3])


def assert_records(a, b, what, keys=("nodes4", "nodesq", "tris", "shade")):
    for key in keys:
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)


@pytest.mark.parametrize("K,S,with_normals,deltas", [(4, 2, True, True), (8, 2, True, False), (0, 2, True, True), (4, 0, False, False)])
def test_pose_equals_update_mesh_of_numpy_and_a_fresh_commit(hiplib, K, S, with_normals, deltas):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE], K, S, normal_deltas=deltas)
    a, b = make_ctx(sc), make_ctx(sc)
    try:
        a.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), K, S, with_normals=with_normals)
        committed = a.debug_mesh_records(TUBE)
        assert committed["has_tree"] and committed["n_tris"] == 502
        for k in range(3):
            pal, bw = pose(k)
            a.pose_mesh(TUBE, pal if K else None, bw if S else None)
            mk = np_skin.skin_mesh(sc.meshes[TUBE], rigs, K, pal, bw if S else None, with_normals)
            b.update_mesh(TUBE, mk, with_normals=with_normals)
            ra, rb = a.debug_mesh_records(TUBE), b.debug_mesh_records(TUBE)
            assert_records(ra, rb, "pose %d" % k)
            assert not np.array_equal(ra["tris"], committed["tris"])
            fa, fb = counted_frame(a), counted_frame(b)
            assert_same(fa, fb, "pose %d against update_mesh" % k)
            assert_same(fa, fresh(with_mesh(sc, TUBE, mk)), "pose %d against a fresh commit" % k)
    finally:
        a.close()
        b.close()


def test_identity_palette_restores_the_commit(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE], 4, 0, convex=True)
    for r in rigs:
        assert np.array_equal(r.weights.sum(axis=1), np.ones(len(r.weights), F))
    ctx = make_ctx(sc)
    try:
        before = counted_frame(ctx)
        r0 = ctx.debug_mesh_records(TUBE)
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 0, with_normals=False)
        ctx.pose_mesh(TUBE, pose(2, amount=0.6)[0])
        assert not np.array_equal(ctx.debug_mesh_records(TUBE)["nodes4"], r0["nodes4"])
        ctx.pose_mesh(TUBE, IDENTITY)
        assert_records(ctx.debug_mesh_records(TUBE), r0, "identity", ("tris", "nodes4", "nodesq", "shade"))
        assert_same(counted_frame(ctx), before, "identity")
    finally:
        ctx.close()


def test_pose_is_ordered_between_queued_renders_and_read_backs(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE])
    pal0, bw0 = pose(0)
    pal1, bw1 = pose(1)
    old = fresh(with_mesh(sc, TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal0, bw0)))
    new = fresh(with_mesh(sc, TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal1, bw1)))
    assert not np.array_equal(old[1], new[1])
    ctx = make_ctx(sc)
    try:
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal0, bw0)
        ctx.render(SPP, 1, asynchronous=True)
        ctx.readback_ldr_begin()
        ctx.pose_mesh(TUBE, pal1, bw1)
        ctx.accum_reset()
        ctx.render(SPP, 1, asynchronous=True)
        first = ctx.readback_ldr_end()
        assert np.array_equal(first, old[1])
        ctx.sync()
        assert np.array_equal(ctx.read_ldr(), new[1]) and np.array_equal(ctx.read_accum(), new[0])
    finally:
        ctx.close()


def test_demo_blob_posed_equals_update_mesh_of_numpy(hiplib):
    """51 200 triangles, 25 600 vertices: a hundred blocks of the skin kernel, and the refit's per-level launches; 64 bones, two shapes"""
    sc = scenes.demo_scene()
    BLOB, n_bones = 2, 64
    rig = np_skin.ring_rig(sc.meshes[BLOB].surfaces[0], n_bones)
    rng = np.random.RandomState(22)
    pal, bw = np_skin.random_palette(rng, n_bones, 0.15), np.array([0.8, -0.3], F)
    w, h, spp, bounces = 160, 96, 4, 3
    a, b = make_ctx(sc, w, h, bounces), make_ctx(sc, w, h, bounces)
    try:
        a.set_mesh_rig(BLOB, sc.meshes[BLOB], host_rigs([rig]), 4, 2)
        a.pose_mesh(BLOB, pal, bw)
        b.update_mesh(BLOB, np_skin.skin_mesh(sc.meshes[BLOB], [rig], 4, pal, bw))
        assert_records(a.debug_mesh_records(BLOB), b.debug_mesh_records(BLOB), "blob")
        assert_same(counted_frame(a, spp), counted_frame(b, spp), "blob")
    finally:
        a.close()
        b.close()


def test_emissive_posed_mesh_under_light_sampling(hiplib):
    sc = small_scene()   # (the second tube instance's second surface is emissive)
    rigs = tube_rigs(sc.meshes[TUBE])
    pal, bw = pose(2)
    a, b = make_ctx(sc), make_ctx(sc)
    try:
        for c in (a, b):
            c.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
        first = counted_frame(a)
        a.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        a.pose_mesh(TUBE, pal, bw)
        b.update_mesh(TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal, bw))
        fa = counted_frame(a)
        assert_same(fa, counted_frame(b), "emissive")
        assert not np.array_equal(fa[0], first[0])
    finally:
        a.close()
        b.close()


def test_refit_tlas_after_a_pose_keeps_working(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE])
    pal, bw = pose(1)
    moved = np.stack([np.asarray(i.transform, F) for i in sc.instances])
    moved[1, 9:] += F(0.3)
    a, b = make_ctx(sc), make_ctx(sc)
    try:
        a.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        a.pose_mesh(TUBE, pal, bw)
        b.update_mesh(TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal, bw))
        a.refit_tlas(moved)
        b.refit_tlas(moved)
        assert_same(counted_frame(a), counted_frame(b), "refit after a pose")
        a.pose_mesh(TUBE, *pose(3))   # and a pose after the refit keeps the moved transforms
        b.update_mesh(TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, *pose(3)))
        assert_same(counted_frame(a), counted_frame(b), "pose after a refit")
    finally:
        a.close()
        b.close()


def test_unreferenced_mesh_and_pose_refusals(hiplib):
    sc = small_scene()
    ctx = make_ctx(sc)
    try:
        before = counted_frame(ctx)
        assert not ctx.debug_mesh_records(SPARE)["has_tree"]
        spare_rigs = [np_skin.random_rig(np.random.RandomState(4), len(s.vertices), 4, 1, N_BONES) for s in sc.meshes[SPARE].surfaces]
        ctx.set_mesh_rig(SPARE, sc.meshes[SPARE], host_rigs(spare_rigs), 4, 1)
        ctx.pose_mesh(SPARE, pose(0)[0], [0.5])
        assert_same(counted_frame(ctx), before, "unreferenced mesh")
        # nothing changed anywhere: the host's copy of the scene is still current
        ctx.update_tlas()
        other = host.Context(0)
        try:
            other.share_scene_from(ctx)
        finally:
            other.close()
        assert len(ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, np.dtype((np.uint8, 48)))) > 0
        # the pose's own checks, with a rig in place
        rigs = tube_rigs(sc.meshes[TUBE])
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        pal, bw = pose(0)
        L = ctx._lib
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES - 1, host._ptr(bw), 2) == E_INVALID
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, None, N_BONES, host._ptr(bw), 2) == E_INVALID
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES, host._ptr(bw), 1) == E_INVALID
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES, host._ptr(np.array([0.5, np.nan], F)), 2) == E_INVALID
        assert L.jpt_scene_pose_mesh(ctx.h, FLOOR, host._ptr(pal), N_BONES, host._ptr(bw), 2) == E_STATE
        assert_same(counted_frame(ctx), before, "refused poses")
        ctx.clear_mesh_rig(TUBE)
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES, host._ptr(bw), 2) == E_STATE
    finally:
        ctx.close()


def test_a_commit_drops_the_rig(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE])
    pal, bw = pose(0)
    ctx = make_ctx(sc)
    try:
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal, bw)
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        with pytest.raises(capi.JptError, match=r"jpt_scene_pose_mesh failed \(-4\).*no rig"):
            ctx.pose_mesh(TUBE, pal, bw)
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal, bw)
        assert_same(counted_frame(ctx), fresh(with_mesh(sc, TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal, bw))), "after a new commit")
    finally:
        ctx.close()


def test_multi_pose_on_one_rank_equals_the_single_context(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE])
    pal, bw = pose(2)
    ctx = make_ctx(sc)
    m = host.MultiContext([0])
    try:
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal, bw)
        want = counted_frame(ctx)
        m.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        m.set_params(W, H, BOUNCES)
        m.set_camera(scenes.camera_block(sc.camera, W, H))
        m.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        m.pose_mesh(TUBE, pal, bw)
        m.render(SPP, 1)
        m.sync()
        assert np.array_equal(m.read_ldr(), want[1]) and np.array_equal(m.read_accum(), want[0])
        m.clear_mesh_rig(TUBE)
    finally:
        m.close()
        ctx.close()


def test_a_large_palette_through_the_context(hiplib):
    """the rig names bones 294 .. 299 only: pose_mesh stages the 300 bones up to the largest index behind the bounds head"""
    sc = small_scene()
    n_bones = 300
    rigs = tube_rigs(sc.meshes[TUBE])
    for r in rigs:
        r.bones = (r.bones + (n_bones - N_BONES)).astype(np.int32)
    assert max(int(r.bones.max()) for r in rigs) == n_bones - 1
    pal, bw = pose(1, n_bones)
    a, b = make_ctx(sc), make_ctx(sc)
    try:
        a.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        a.pose_mesh(TUBE, pal, bw)
        b.update_mesh(TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal, bw))
        assert_records(a.debug_mesh_records(TUBE), b.debug_mesh_records(TUBE), "300 bones")
        assert_same(counted_frame(a), counted_frame(b), "300 bones")
    finally:
        a.close()
        b.close()


def test_a_refused_upload_drops_the_rig_and_a_pose_is_a_state_error(hiplib):
    sc = small_scene()
    rigs = tube_rigs(sc.meshes[TUBE])
    pal, bw = pose(0)
    ctx = make_ctx(sc)
    try:
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal, bw)
        L = ctx._lib
        # an upload that validation refuses (no material table): the scene is gone, and so is the rig
        assert L.jpt_scene_upload_reference_layout(ctx.h, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0) == E_INVALID
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES, host._ptr(bw), 2) == E_STATE
        assert b"jpt_scene_pose_mesh needs a scene made by jpt_scene_commit" in L.jpt_last_error(ctx.h)
        arr = host._update_surfaces(sc.meshes[TUBE])
        assert L.jpt_scene_update_mesh(ctx.h, TUBE, arr, 2) == E_STATE
        # a new commit starts without a rig
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        assert L.jpt_scene_pose_mesh(ctx.h, TUBE, host._ptr(pal), N_BONES, host._ptr(bw), 2) == E_STATE
        assert b"no rig" in L.jpt_last_error(ctx.h)
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)
        ctx.set_mesh_rig(TUBE, sc.meshes[TUBE], host_rigs(rigs), 4, 2)   # (replacing a rig a pose has used)
        ctx.pose_mesh(TUBE, pal, bw)
        assert_same(counted_frame(ctx), fresh(with_mesh(sc, TUBE, np_skin.skin_mesh(sc.meshes[TUBE], rigs, 4, pal, bw))), "after the refused upload")
    finally:
        ctx.close()
