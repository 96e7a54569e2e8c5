"""jpt_scene_update_mesh on the device: a deformed mesh's triangle records and BLAS boxes refitted over the committed topology.
Every image is compared with an independent result -- a fresh JPT_BUILD_SAH_WATERTIGHT commit of the deformed scene, or the
oracle's tree-independent answer -- and the refitted records are checked against a numpy restatement."""
import copy

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

pytestmark = pytest.mark.gpu

BLOB = 2   # the demo scene's character mesh, named by two instances
E_STATE = -4


def deform(mesh, k, amount=1.0):
    """a smooth wobble, plus the x > 0 half pushed outwards: part of the mesh leaves its committed boxes"""
    m = copy.deepcopy(mesh)
    for s in m.surfaces:
        v = s.vertices.astype(np.float64)
        d = np.zeros_like(v)
        d[:, 1] = 0.08 * np.sin(3.0 * v[:, 0] + 0.7 * k)
        d[:, 0] = np.where(v[:, 0] > 0.0, 0.25 * k, 0.0)
        d[:, 2] = 0.05 * k * np.cos(2.0 * v[:, 1])
        s.vertices = (v + amount * d).astype(np.float32)
        n = s.normals.astype(np.float64) + 0.1 * k * np.array([0.0, 1.0, 0.0])
        s.normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return m


def with_mesh(scene, mesh_id, mesh):
    sc = copy.copy(scene)
    sc.meshes = list(scene.meshes)
    sc.meshes[mesh_id] = mesh
    return sc


def frame(ctx):
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth()


def fresh(scene, w, h, spp, bounces):
    """the independent answer: a fresh watertight commit of `scene`, one counted render"""
    ctx = host.Context(0)
    try:
        ctx.build_scene(scene, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(scene.camera, w, h))
        ctx.render(spp, 1, counted=True)
        return frame(ctx) + (ctx.stats()["rays"],)
    finally:
        ctx.close()


def assert_same(got, want, what):
    for g, x, name in zip(got, want, ("accumulation", "display", "depth")):
        bad = ~((g == x) | (np.isnan(g) & np.isnan(x)))
        if bad.ndim == 3:
            bad = bad.any(axis=-1)
        assert not bad.any(), "%s: %s differs at %d pixels, first %s" % (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def counted_frame(ctx, spp):
    ctx.accum_reset()
    ctx.render(spp, 1, counted=True)
    return frame(ctx) + (ctx.stats()["rays"],)


@pytest.mark.parametrize("w,h,spp,bounces,steps", [(160, 96, 4, 3, 3), (1920, 1080, 8, 4, 2)])
def test_demo_blob_deformed_equals_a_fresh_commit(hiplib, w, h, spp, bounces, steps):
    sc = scenes.demo_scene()
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        for k in range(1, steps + 1):
            mk = deform(sc.meshes[BLOB], k)
            ctx.render(spp, 1, asynchronous=True)      # queued before the update: reads the previous vertices
            ctx.update_mesh(BLOB, mk)
            ctx.render(spp, 1, asynchronous=True)      # queued after it
            got = counted_frame(ctx, spp)
            want = fresh(with_mesh(sc, BLOB, mk), w, h, spp, bounces)
            assert_same(got[:3], want[:3], "step %d" % k)
            assert got[3] == want[3]
    finally:
        ctx.close()


def test_update_is_ordered_between_queued_renders_and_read_backs(hiplib):
    sc = scenes.demo_scene()
    w, h, spp, bounces = 128, 96, 2, 3
    mk = deform(sc.meshes[BLOB], 2)
    old = fresh(sc, w, h, spp, bounces)
    new = fresh(with_mesh(sc, BLOB, mk), w, h, spp, bounces)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.render(spp, 1, asynchronous=True)
        ctx.readback_ldr_begin()
        ctx.update_mesh(BLOB, mk)
        ctx.accum_reset()
        ctx.render(spp, 1, asynchronous=True)
        first = ctx.readback_ldr_end()
        assert np.array_equal(first, old[1])
        ctx.sync()
        assert np.array_equal(ctx.read_ldr(), new[1])
        assert np.array_equal(ctx.read_accum(), new[0])
    finally:
        ctx.close()


def test_restoring_the_vertices_restores_the_records_and_the_image(hiplib):
    sc = scenes.demo_scene()
    w, h, spp, bounces = 128, 96, 2, 3
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        before = counted_frame(ctx, spp)
        r0 = ctx.debug_mesh_records(BLOB)
        assert r0["has_tree"] and r0["n_tris"] == sc.meshes[BLOB].n_tris and r0["n_records"] > 100
        ctx.update_mesh(BLOB, deform(sc.meshes[BLOB], 3))
        r1 = ctx.debug_mesh_records(BLOB)
        assert not np.array_equal(r1["nodes4"], r0["nodes4"]) and not np.array_equal(r1["tris"], r0["tris"])
        ctx.update_mesh(BLOB, sc.meshes[BLOB])
        r2 = ctx.debug_mesh_records(BLOB)
        for key in ("nodes4", "nodesq", "tris", "shade"):
            assert np.array_equal(r2[key], r0[key]), key
        assert_same(counted_frame(ctx, spp)[:3], before[:3], "restored")
    finally:
        ctx.close()


# ---- conservativeness, from the records themselves ------------------------------------------------------------------------

K_PLANE_SLACK = 1.0 / 256.0   # jpt_nodeq.h
EMPTY = -(2 ** 31)


def wide_tris(v0, v1, v2):
    """make_wide_tri (jpt_mesh_math.h) in float32, one rounding per operation"""
    e1, e2 = v1 - v0, v2 - v0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    out = np.zeros((len(v0), 12), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7], out[:, 8:11], out[:, 11] = v0, n[:, 0], e1, n[:, 1], e2, n[:, 2]
    return out


def records(rec):
    f = rec["nodes4"].view(np.float32).reshape(-1, 32)
    child = rec["nodes4"].view(np.int32).reshape(-1, 32)[:, 12:16]
    lo, hi = f[:, 0:12].reshape(-1, 3, 4), f[:, 16:28].reshape(-1, 3, 4)
    q = rec["nodesq"]
    qf = q.view(np.float32).reshape(-1, 16)
    origin, scale = qf[:, 0:3].astype(np.float64), np.stack([qf[:, 3], qf[:, 4], qf[:, 5]], axis=1).astype(np.float64)
    planes = q.view(np.uint32).reshape(-1, 16)[:, 6:12]   # lo_x lo_y lo_z hi_x hi_y hi_z
    qlo = np.stack([(planes[:, a][:, None] >> (8 * np.arange(4))[None, :]) & 255 for a in range(3)], axis=1).astype(np.float64)
    qhi = np.stack([(planes[:, 3 + a][:, None] >> (8 * np.arange(4))[None, :]) & 255 for a in range(3)], axis=1).astype(np.float64)
    dlo = origin[:, :, None] + (qlo - K_PLANE_SLACK) * scale[:, :, None]
    dhi = origin[:, :, None] + (qhi + K_PLANE_SLACK) * scale[:, :, None]
    qchild = q.view(np.int32).reshape(-1, 16)[:, 12:16]
    assert np.array_equal(qchild, child)
    return child, lo, hi, dlo, dhi


def device_order(rec0, mesh):
    """which triangle of `mesh` (committed vertices) each device triangle is: matched by its WideTri bytes"""
    s = mesh.surfaces[0]
    tri = s.vertices[s.indices.reshape(-1, 3)]
    key = {wide_tris(tri[:, 0], tri[:, 1], tri[:, 2])[i].tobytes(): i for i in range(len(tri))}
    dev = rec0["tris"].view(np.float32).reshape(-1, 12)
    return np.array([key[dev[i].tobytes()] for i in range(len(dev))])


def check_conservative(rec, tri_vertices):
    """every triangle's vertices lie inside the float box and the dequantised box of every slot on its path from the root"""
    child, lo, hi, dlo, dhi = records(rec)
    first, first_tri = rec["first_record"], rec["first_tri"]
    stack = [(rec["root"] - first, [])]
    seen = 0
    while stack:
        r, path = stack.pop()
        for k in range(4):
            c = int(child[r, k])
            if c == EMPTY:
                continue
            p = path + [(r, k)]
            if c >= 0:
                stack.append((c - first, p))
                continue
            l = ~c
            t0, n = (l & ((1 << 25) - 1)) - first_tri, (l >> 25) + 1
            v = tri_vertices[t0:t0 + n].reshape(-1, 3).astype(np.float64)
            for (pr, pk) in p:
                assert (v >= lo[pr, :, pk]).all() and (v <= hi[pr, :, pk]).all(), "float box of record %d slot %d" % (pr + first, pk)
                assert (v >= dlo[pr, :, pk]).all() and (v <= dhi[pr, :, pk]).all(), "quantised box of record %d slot %d" % (pr + first, pk)
            seen += n
    assert seen == len(tri_vertices)


def hostile(mesh, kind):
    m = copy.deepcopy(mesh)
    v = m.surfaces[0].vertices.copy()
    if kind == "plane":
        v[:, 1] = 0.25
    elif kind == "far_vertex":
        v[17] = (1.0e4, -3.0e3, 2.0e4)
    elif kind == "degenerate":
        idx = m.surfaces[0].indices.reshape(-1, 3)
        v[idx[::3, 1]] = v[idx[::3, 0]]     # triangles with two equal vertices (and their neighbours stretched)
    elif kind == "tiny":
        v = v * np.float32(1e-3)
    m.surfaces[0].vertices = v.astype(np.float32)
    return m


def test_refitted_boxes_contain_the_triangles_under_hostile_deformations(hiplib):
    sc = scenes.demo_scene(n_tris=2048)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        rec0 = ctx.debug_mesh_records(BLOB)
        perm = device_order(rec0, sc.meshes[BLOB])
        s0 = sc.meshes[BLOB].surfaces[0]
        check_conservative(rec0, s0.vertices[s0.indices.reshape(-1, 3)][perm])
        for kind in ("plane", "far_vertex", "degenerate", "tiny"):
            m = hostile(sc.meshes[BLOB], kind)
            ctx.update_mesh(BLOB, m)
            rec = ctx.debug_mesh_records(BLOB)
            s = m.surfaces[0]
            tv = s.vertices[s.indices.reshape(-1, 3)][perm]
            assert np.array_equal(rec["tris"].view(np.float32).reshape(-1, 12).view(np.uint32),
                                  wide_tris(tv[:, 0], tv[:, 1], tv[:, 2]).view(np.uint32)), kind
            sh = rec["shade"].view(np.float32).reshape(-1, 16)
            assert np.array_equal(sh[:, 0:9].reshape(-1, 3, 3), s.normals[s.indices.reshape(-1, 3)][perm]), kind
            check_conservative(rec, tv)
    finally:
        ctx.close()


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


@pytest.mark.parametrize("seed", [3, 11])
def test_random_scenes_deformed_match_the_tree_independent_answer(oracle, hiplib, seed):
    sc = scenes.random_scene(seed, coincident=False)
    w, h, bounces, frames = 96, 64, 3, 2
    cam = scenes.camera_block(sc.camera, w, h)
    rng = np.random.RandomState(seed)
    moved = copy.deepcopy(sc)
    for m in moved.meshes:
        for s in m.surfaces:
            s.vertices = (s.vertices + rng.normal(0.0, 0.2, size=s.vertices.shape) + rng.normal(0.0, 0.3, size=3)).astype(np.float32)
    ref = oracle.build_scene(moved)
    want, _, _, _, _ = oracle.render(ref, cam, w, h, bounces, frames, 1, wire.ACCUM_HDR_F32, flags=1)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces, wire.ACCUM_HDR_F32)
        ctx.set_camera(cam)
        ctx.render(frames, 1)
        for i, m in enumerate(moved.meshes):
            ctx.update_mesh(i, m)
        ctx.accum_reset()
        ctx.render(frames, 1)
        got = ctx.read_accum()
    finally:
        ctx.close()
    nan_got, nan_want = np.isnan(got).any(axis=-1), np.isnan(want).any(axis=-1)
    ok = ~(nan_got | nan_want)
    assert np.array_equal(nan_got, nan_want)
    assert rel_l2(got[ok], want[ok]) <= 1e-4


def test_million_triangle_mesh_deformed_equals_a_fresh_commit(hiplib):
    sc = scenes.unique_scene()
    w, h, spp, bounces = 256, 192, 2, 3
    mk = deform(sc.meshes[BLOB], 1, amount=0.5)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.render(spp, 1, asynchronous=True)
        ctx.update_mesh(BLOB, mk)
        got = counted_frame(ctx, spp)
    finally:
        ctx.close()
    want = fresh(with_mesh(sc, BLOB, mk), w, h, spp, bounces)
    assert_same(got[:3], want[:3], "unique_scene")
    assert got[3] == want[3]


@pytest.mark.parametrize("mesh_first", [False, True])
def test_moving_instances_and_deforming_meshes_in_one_step(hiplib, mesh_first):
    sc = scenes.demo_scene()
    w, h, spp, bounces = 128, 96, 2, 3
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, bounces)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        cur = copy.deepcopy(sc)
        for k in (1, 2):
            mk = deform(sc.meshes[BLOB], k)
            t = [np.asarray(i.transform, np.float32).copy() for i in cur.instances]
            t[2][9] += np.float32(0.2 * k)     # the first character moves, the second turns
            t[3][:9] = (scenes.rot_y(10.0 * k) @ t[3][:9].reshape(3, 3).astype(np.float64)).astype(np.float32).reshape(-1)
            ctx.render(spp, 1, asynchronous=True)
            if mesh_first:
                ctx.update_mesh(BLOB, mk)
                ctx.refit_tlas(np.stack(t))
            else:
                ctx.refit_tlas(np.stack(t))
                ctx.update_mesh(BLOB, mk)
            cur = with_mesh(cur, BLOB, mk)
            cur.instances = [copy.copy(i) for i in cur.instances]
            for i, inst in enumerate(cur.instances):
                inst.transform = t[i]
            got = counted_frame(ctx, spp)
            want = fresh(cur, w, h, spp, bounces)
            assert_same(got[:3], want[:3], "step %d" % k)
            assert got[3] == want[3]
    finally:
        ctx.close()


def test_stale_host_mirrors_are_refused_until_the_next_commit(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    w, h = 64, 48
    ctx, other = host.Context(0), host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, 2)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.update_mesh(BLOB, deform(sc.meshes[BLOB], 1))
        ctx.render(1, 1)
        with pytest.raises(capi.JptError, match="jpt_scene_update_tlas failed \\(-4\\).*jpt_scene_commit"):
            ctx.update_tlas()
        with pytest.raises(capi.JptError, match="\\(-4\\).*jpt_scene_commit"):
            other.share_scene_from(ctx)
        with pytest.raises(capi.JptError, match="\\(-4\\).*jpt_scene_commit"):
            ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY)
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        with pytest.raises(capi.JptError, match="\\(-4\\).*jpt_scene_commit"):
            ctx.render(1, 1)
        ctx.set_kernel(capi.KERNEL_WAVEFRONT)
        ctx.set_debug_steps(True)
        with pytest.raises(capi.JptError, match="\\(-4\\).*jpt_scene_commit"):
            ctx.render(1, 1)
        ctx.set_debug_steps(False)
        ctx.refit_tlas(np.stack([np.asarray(i.transform, np.float32) for i in sc.instances]))   # keeps working
        ctx.render(1, 1)
        # a new commit brings everything back
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.update_tlas()
        assert len(ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY)) == sum(m.n_tris for m in sc.meshes)
        other.share_scene_from(ctx)
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        ctx.render(1, 1)
    finally:
        ctx.close()
        other.close()


def test_unnamed_mesh_update_changes_nothing_on_the_device(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    sc.meshes.append(scenes.blob_mesh(512, seed=9))   # no instance names it
    w, h, spp = 64, 48, 2
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        ctx.set_params(w, h, 2)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        before = counted_frame(ctx, spp)
        assert not ctx.debug_mesh_records(len(sc.meshes) - 1)["has_tree"]
        ctx.update_mesh(len(sc.meshes) - 1, deform(sc.meshes[-1], 2))
        assert_same(counted_frame(ctx, spp)[:3], before[:3], "unnamed mesh")
    finally:
        ctx.close()


def test_multi_device_update_equals_one_fresh_context(hiplib):
    sc = scenes.demo_scene()
    w, h, spp, bounces = 128, 96, 2, 3
    mk = deform(sc.meshes[BLOB], 2)
    want = fresh(with_mesh(sc, BLOB, mk), w, h, spp, bounces)
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        m.set_params(w, h, bounces)
        m.set_camera(scenes.camera_block(sc.camera, w, h))
        m.render(spp, 1)
        m.update_mesh(BLOB, mk)
        m.accum_reset()
        m.render(spp, 1)
        m.sync()
        assert np.array_equal(m.read_ldr(), want[1])
        assert np.array_equal(m.read_accum(), want[0])
    finally:
        m.close()
