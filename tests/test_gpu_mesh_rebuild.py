"""jpt_scene_rebuild_mesh on the device: the sort against its host form, the records against the numpy restatement
(tests/np_mesh_rebuild.py), the images against fresh commits, the calls around it, and what it is for -- fewer record steps than a
refit once a mesh's triangles have swapped places."""
import copy
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_mesh_rebuild as ref
import np_skin
from test_gpu_mesh_update import BLOB, assert_same, check_conservative, counted_frame, deform, device_order, fresh, hostile, with_mesh
from test_gpu_skin import SPARE, TUBE, host_rigs, pose as skin_pose, small_scene, tube_rigs
from test_gpu_tlas_rebuild import (_assert_frames_equal, _five_instances, _fresh_watertight, _jitter_all, _quantised, _small_ctx, _small_frame,
                                   _watertight_ctx, _watertight_frame, all_t12)
from test_mesh_rebuild_host import degenerate_cases, soup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BOUNCES = 160, 96, 2, 3


def _constant(name):
    text = open(os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_mesh_rebuild.h")).read()
    return int(re.search(r"%s = (\d+)" % name, text).group(1))


T = _constant("kMeshSortTile")             # the keys one block of the sort owns
SCAN_THREADS = _constant("kMeshScanThreads")
assert T == 2048 and SCAN_THREADS == 1024

# A slot (4 / 5), a wave (63 .. 65), a step of the block's 256 threads (255 .. 257), a tile (T - 1 .. T + 1), more than one tile with a
# ragged end (2 T + 17), the two sides of the one-block TLAS sort's limit (32 767 / 32 768), and 70 001: 35 tiles, so a pass's
# [digit][block] table has 256 x 35 = 8960 words, more than one sweep of the scanning block's 1024 threads (each of its sixteen waves
# owns 560 words: nine sweeps of its 64 lanes, the last ragged; from 5 tiles on, i.e. 32 767 and 32 768 too, at four sweeps).
ORDER_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 17, 32767, 32768, 70001]
assert 256 * ((70001 + T - 1) // T) > SCAN_THREADS


@pytest.mark.parametrize("n", ORDER_COUNTS)
def test_device_order_equals_the_host_form(hiplib, n):
    v, ix = soup(np.random.RandomState(n), n)
    if n > 64:
        ix[n // 2:n // 2 + 20] = ix[7]   # some equal codes: the index decides
    codes, order = host.debug_mesh_order(0, v, ix)
    want_codes, want_order = host.debug_mesh_order(-1, v, ix)
    assert np.array_equal(codes, want_codes)
    assert np.array_equal(order, want_order)
    _, order_only = host.debug_mesh_order(0, v, ix, with_codes=False)
    assert np.array_equal(order_only, want_order)


DEGENERATE = degenerate_cases(3 * T + 5)   # equal codes across block boundaries: where stability can fail


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_device_order_of_degenerate_meshes_equals_the_host_form(hiplib, name):
    v, ix = DEGENERATE[name]
    codes, order = host.debug_mesh_order(0, v, ix)
    want_codes, want_order = host.debug_mesh_order(-1, v, ix)
    assert np.array_equal(codes, want_codes)
    assert np.array_equal(order, want_order)
    if name == "one_centre":
        assert np.array_equal(order, np.arange(len(ix)))


# ---- the records ---------------------------------------------------------------------------------------------------------------

def soup_mesh(n_tris, seed):
    """n disjoint small triangles in the blob's place, one surface"""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-0.5, 0.5, (n_tris, 1, 3))
    v = (centre + rng.uniform(-0.15, 0.15, (n_tris, 3, 3))).reshape(-1, 3).astype(np.float32)
    n = np.tile(np.float32([0, 1, 0]), (len(v), 1))
    return scenes.Mesh([scenes.Surface(v, n, np.zeros((len(v), 2), np.float32), np.arange(len(v), dtype=np.int32))])


def jittered(mesh, seed):
    m = copy.deepcopy(mesh)
    rng = np.random.RandomState(seed)
    s = m.surfaces[0]
    s.vertices = (s.vertices + rng.normal(0.0, 0.2, s.vertices.shape)).astype(np.float32)
    return m


def assert_records_are_numpys(rec, tv, what):
    """rec: jpt_debug_mesh_records after a rebuild; tv: the mesh's triangles' vertices in device order, float32 [t, 3, 3]"""
    v, ix = tv.reshape(-1, 3), np.arange(3 * len(tv)).reshape(-1, 3)
    _, order = ref.order(v, ix)
    lo, hi = ref.tri_boxes(v, ix)
    want = ref.records(order, lo, hi, ref.box_pad(v, ix), rec["first_record"], rec["first_tri"])
    mine = rec["nodes4"].view(np.dtype(want.dtype)).reshape(-1)
    assert rec["root"] == rec["first_record"] and len(mine) == len(want), what
    assert np.array_equal(mine["child"], want["child"]), what
    assert np.array_equal(mine["lo"].view(np.uint32), want["lo"].view(np.uint32)), what
    assert np.array_equal(mine["hi"].view(np.uint32), want["hi"].view(np.uint32)), what
    assert np.array_equal(rec["nodes4"], want.view(np.uint8).reshape(-1, 128)), what
    assert np.array_equal(rec["nodesq"], _quantised(np.ascontiguousarray(rec["nodes4"]))), what
    check_conservative(rec, tv)


@pytest.mark.parametrize("which", ["five", "seventeen", "blob2048"])
def test_records_after_a_rebuild_are_numpys_template_over_the_devices_order(hiplib, which):
    sc = scenes.demo_scene(n_tris=2048)
    if which != "blob2048":
        sc = with_mesh(sc, BLOB, soup_mesh(5 if which == "five" else 17, 3))
    mesh = sc.meshes[BLOB]
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        rec0 = ctx.debug_mesh_records(BLOB)
        perm = device_order(rec0, mesh)

        def tris_of(m):
            s = m.surfaces[0]
            return s.vertices[s.indices.reshape(-1, 3)][perm]

        steps = [(kind, hostile(mesh, kind)) for kind in ("plane", "far_vertex", "degenerate", "tiny")] if which == "blob2048" else \
                [("jitter%d" % k, jittered(mesh, k)) for k in (1, 2)]
        for kind, m in steps:   # every rebuild after the first goes into the same region
            ctx.rebuild_mesh(BLOB, m)
            rec = ctx.debug_mesh_records(BLOB)
            assert rec["first_record"] >= rec0["first_record"] + rec0["n_records"] and rec["n_tris"] == mesh.n_tris, kind
            assert_records_are_numpys(rec, tris_of(m), kind)
        region = (rec["first_record"], rec["n_records"])
        # a refit keeps the rebuilt topology: the child words stay, the boxes follow
        back = jittered(mesh, 7)
        ctx.update_mesh(BLOB, back)
        after = ctx.debug_mesh_records(BLOB)
        assert (after["first_record"], after["n_records"]) == region
        child = lambda r: r["nodes4"].view(np.int32).reshape(-1, 32)[:, 12:16]
        assert np.array_equal(child(after), child(rec))
        check_conservative(after, tris_of(back))
    finally:
        ctx.close()


# ---- the images ----------------------------------------------------------------------------------------------------------------

def _demo_ctx(sc):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
    ctx.set_params(W, H, BOUNCES)
    ctx.set_camera(scenes.camera_block(sc.camera, W, H))
    return ctx


def _assert_fresh(ctx, scene, what):
    got = counted_frame(ctx, SPP)
    want = fresh(scene, W, H, SPP, BOUNCES)
    assert_same(got[:3], want[:3], what)
    assert got[3] == want[3], what


def test_rebuilt_blob_equals_a_fresh_commit_blocking_queued_and_restored(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    blob = sc.meshes[BLOB]
    ctx = _demo_ctx(sc)
    try:
        r0 = ctx.debug_mesh_records(BLOB)
        m1 = deform(blob, 1)
        ctx.rebuild_mesh(BLOB, m1)                      # blocking renders around it
        _assert_fresh(ctx, with_mesh(sc, BLOB, m1), "rebuild, blocking")
        m2 = deform(blob, 2)
        ctx.render(SPP, 1, asynchronous=True)            # queued before the rebuild: reads the previous vertices and topology
        ctx.rebuild_mesh(BLOB, m2)                       # a second rebuild, into the same region, between queued renders
        ctx.render(SPP, 1, asynchronous=True)
        _assert_fresh(ctx, with_mesh(sc, BLOB, m2), "second rebuild, queued")
        m3 = deform(blob, 3)
        ctx.update_mesh(BLOB, m3)                        # a refit over the rebuilt topology
        _assert_fresh(ctx, with_mesh(sc, BLOB, m3), "update_mesh after a rebuild")
        ctx.rebuild_mesh(BLOB, blob)                     # the committed vertices again: the fresh commit's image, not its records
        _assert_fresh(ctx, sc, "restored")
        r1 = ctx.debug_mesh_records(BLOB)
        assert r1["first_record"] >= r0["first_record"] + r0["n_records"]
        assert np.array_equal(r1["tris"], r0["tris"]) and np.array_equal(r1["shade"], r0["shade"])
    finally:
        ctx.close()


def test_rebuild_is_ordered_between_queued_renders_and_read_backs(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    m1, m2 = deform(sc.meshes[BLOB], 1), deform(sc.meshes[BLOB], 2)
    old = fresh(with_mesh(sc, BLOB, m1), W, H, SPP, BOUNCES)
    new = fresh(with_mesh(sc, BLOB, m2), W, H, SPP, BOUNCES)
    ctx = _demo_ctx(sc)
    try:
        ctx.rebuild_mesh(BLOB, m1)                       # the region exists from here on: the next rebuild waits for nothing
        ctx.render(SPP, 1, asynchronous=True)
        ctx.readback_ldr_begin()
        ctx.rebuild_mesh(BLOB, m2)
        ctx.accum_reset()
        ctx.render(SPP, 1, asynchronous=True)
        first = ctx.readback_ldr_end()
        assert np.array_equal(first, old[1])
        ctx.sync()
        assert np.array_equal(ctx.read_ldr(), new[1])
        assert np.array_equal(ctx.read_accum(), new[0])
    finally:
        ctx.close()


def test_poses_after_and_with_a_rebuild_equal_a_fresh_commit(hiplib):
    sc = small_scene()
    bind, rigs = sc.meshes[TUBE], tube_rigs(sc.meshes[TUBE])
    ctx = _watertight_ctx(sc, W, H)
    try:
        ctx.render(1, 1)
        bent = deform(bind, 1)
        ctx.rebuild_mesh(TUBE, bent)                     # two surfaces, 502 triangles
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(sc, TUBE, bent)), "rebuild")
        ctx.set_mesh_rig(TUBE, bind, host_rigs(rigs), 4, 2)
        pal, bw = skin_pose(1)
        ctx.pose_mesh(TUBE, pal, bw)                     # a refit over the rebuilt topology
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(sc, TUBE, np_skin.skin_mesh(bind, rigs, 4, pal, bw))), "pose after a rebuild")
        pal, bw = skin_pose(2)
        ctx.render(1, 1, asynchronous=True)
        ctx.pose_mesh(TUBE, pal, bw, rebuild=True)       # jpt_scene_pose_mesh_rebuild, into the same region
        ctx.render(1, 1, asynchronous=True)
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(sc, TUBE, np_skin.skin_mesh(bind, rigs, 4, pal, bw))), "pose with a rebuild")
    finally:
        ctx.close()
    # ... and a pose's rebuild as the mesh's first
    ctx = _watertight_ctx(sc, W, H)
    try:
        ctx.set_mesh_rig(TUBE, bind, host_rigs(rigs), 4, 2)
        ctx.pose_mesh(TUBE, pal, bw, rebuild=True)
        assert ctx.debug_mesh_records(TUBE)["first_record"] > 0
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(sc, TUBE, np_skin.skin_mesh(bind, rigs, 4, pal, bw))), "a pose's first rebuild")
    finally:
        ctx.close()


def test_two_meshes_rebuilt_in_one_context(hiplib):
    sc = _five_instances()
    bent_tube, bent_box = deform(sc.meshes[TUBE], 2), deform(sc.meshes[SPARE], 1)
    ctx = _watertight_ctx(sc, W, H)
    try:
        ctx.rebuild_mesh(TUBE, bent_tube)
        ctx.render(1, 1, asynchronous=True)
        ctx.rebuild_mesh(SPARE, bent_box)                # the second region: the record arrays grow again
        want = with_mesh(with_mesh(sc, TUBE, bent_tube), SPARE, bent_box)
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(want), "two regions")
        a, b = ctx.debug_mesh_records(TUBE), ctx.debug_mesh_records(SPARE)
        assert b["first_record"] == a["first_record"] + a["n_records"]
        ctx.rebuild_mesh(TUBE, sc.meshes[TUBE])          # the first region again, the second untouched
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(sc, SPARE, bent_box)), "first region again")
    finally:
        ctx.close()


def test_mesh_and_tlas_rebuilds_in_both_orders_queued_equal_synced_and_fresh_commits(hiplib):
    sc = _five_instances()
    bent_tube, bent_box = deform(sc.meshes[TUBE], 1), deform(sc.meshes[SPARE], 2)
    m1 = _jitter_all(sc, 3)
    m2 = _jitter_all(m1, 4)

    def run(synced):
        ctx = _small_ctx(sc)
        after = ctx.sync if synced else (lambda: None)
        try:
            ctx.render(2, 1, asynchronous=True)
            after()
            ctx.rebuild_mesh(TUBE, bent_tube)            # the mesh, then the instance level
            after()
            ctx.rebuild_tlas(all_t12(m1))
            after()
            first = _small_frame(ctx, True)
            ctx.render(2, 1, asynchronous=True)
            after()
            ctx.rebuild_tlas(all_t12(m2))                # the instance level, then a mesh
            after()
            ctx.rebuild_mesh(SPARE, bent_box)
            after()
            return first, _small_frame(ctx, True)
        finally:
            ctx.close()

    def fresh_small(scene):
        ctx = _small_ctx(scene)
        try:
            return _small_frame(ctx, True)
        finally:
            ctx.close()

    queued, synced = run(False), run(True)
    for k in (0, 1):
        _assert_frames_equal(queued[k], synced[k], "image %d, queued against synced" % (k + 1))
    _assert_frames_equal(queued[0], fresh_small(with_mesh(m1, TUBE, bent_tube)), "mesh then TLAS against a fresh commit")
    _assert_frames_equal(queued[1], fresh_small(with_mesh(with_mesh(m2, TUBE, bent_tube), SPARE, bent_box)), "TLAS then mesh against a fresh commit")


def test_light_sampling_follows_a_rebuilt_emitter(hiplib):
    sc = scenes.demo_scene(n_tris=2048)
    light = copy.deepcopy(sc.meshes[0])   # the emissive plane: two triangles, the smallest tree the rebuild makes
    s = light.surfaces[0]
    s.vertices = (s.vertices * np.float32([0.6, 1.0, 1.3]) + np.float32([0.3, -0.2, 0.1])).astype(np.float32)
    moved = with_mesh(sc, 0, light)
    frames = {}
    for route in ("rebuild", "fresh"):
        ctx = host.Context(0)
        try:
            ctx.build_scene(sc if route == "rebuild" else moved, capi.BUILD_SAH_WATERTIGHT)
            ctx.set_params(W, H, BOUNCES, wire.ACCUM_HDR_F32)
            ctx.set_camera(scenes.camera_block(sc.camera, W, H))
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
            if route == "rebuild":
                ctx.render(2, 1)
                before = ctx.read_accum()
                ctx.rebuild_mesh(0, light)
                ctx.accum_reset()
            ctx.render(2, 1)
            frames[route] = (ctx.read_accum(), ctx.read_depth())
        finally:
            ctx.close()
    assert not np.array_equal(frames["rebuild"][0], before)
    assert np.array_equal(frames["rebuild"][0].view(np.uint32), frames["fresh"][0].view(np.uint32))
    assert np.array_equal(frames["rebuild"][1].view(np.uint32), frames["fresh"][1].view(np.uint32))


def test_queries_and_guides_follow_a_rebuild(hiplib):
    sc = scenes.demo_scene(n_tris=2048)
    bent = deform(sc.meshes[BLOB], 2)
    moved = with_mesh(sc, BLOB, bent)
    w, h = 96, 64
    cam = scenes.camera_block(sc.camera, w, h)
    xy = np.stack(np.meshgrid(np.arange(0, w, 3) + 0.5, np.arange(0, h, 3) + 0.5), axis=-1).reshape(-1, 2).astype(np.float32)

    def answers(ctx):
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.denoise()
        return [ctx.query_pixels(xy)] + list(ctx.read_guides())

    got_ctx, refit_ctx, want_ctx = host.Context(0), host.Context(0), host.Context(0)
    try:
        for c, scene in ((got_ctx, sc), (refit_ctx, sc), (want_ctx, moved)):
            c.build_scene(scene, capi.BUILD_SAH_WATERTIGHT)
            c.set_params(w, h, 2, wire.ACCUM_HDR_F32)
            c.set_camera(cam)
        before = answers(got_ctx)
        got_ctx.rebuild_mesh(BLOB, bent)
        refit_ctx.update_mesh(BLOB, bent)
        got, refit, want = answers(got_ctx), answers(refit_ctx), answers(want_ctx)
        assert got[0].tobytes() != before[0].tobytes()
        # a hit's `triangle` counts in device order, which is the commit's: the rebuild does not reorder triangles, so against a refit
        # of the same commit every byte is equal; a fresh commit of the deformed mesh numbers its triangles anew, every other field is equal
        assert got[0].tobytes() == refit[0].tobytes()
        hits_got, hits_want = got[0].view(wire.RAY_HIT).reshape(-1), want[0].view(wire.RAY_HIT).reshape(-1)
        for name in wire.RAY_HIT.names:
            if name != "triangle":
                assert hits_got[name].tobytes() == hits_want[name].tobytes(), name
        for g, x in zip(got[1:], want[1:]):
            assert np.array_equal(g.view(np.uint32), x.view(np.uint32))
    finally:
        got_ctx.close()
        refit_ctx.close()
        want_ctx.close()


def test_multi_device_rebuild_equals_one_fresh_context(hiplib):
    sc = scenes.demo_scene(n_tris=4096)
    mk = deform(sc.meshes[BLOB], 2)
    want = fresh(with_mesh(sc, BLOB, mk), W, H, SPP, BOUNCES)
    m = host.MultiContext([0, 0])
    try:
        m.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        m.set_params(W, H, BOUNCES)
        m.set_camera(scenes.camera_block(sc.camera, W, H))
        m.render(SPP, 1)
        m.rebuild_mesh(BLOB, mk)
        m.accum_reset()
        m.render(SPP, 1)
        m.sync()
        assert np.array_equal(m.read_ldr(), want[1])
        assert np.array_equal(m.read_accum(), want[0])
    finally:
        m.close()


def test_unnamed_mesh_rebuild_changes_nothing_on_the_device(hiplib):
    sc = scenes.demo_scene(n_tris=2048)
    sc.meshes.append(scenes.blob_mesh(512, seed=9))   # no instance names it
    ctx = _demo_ctx(sc)
    try:
        before = counted_frame(ctx, SPP)
        blob0 = ctx.debug_mesh_records(BLOB)
        assert not ctx.debug_mesh_records(len(sc.meshes) - 1)["has_tree"]
        ctx.rebuild_mesh(len(sc.meshes) - 1, deform(sc.meshes[-1], 2))
        assert not ctx.debug_mesh_records(len(sc.meshes) - 1)["has_tree"]
        assert_same(counted_frame(ctx, SPP)[:3], before[:3], "unnamed mesh")
        blob1 = ctx.debug_mesh_records(BLOB)
        assert all(np.array_equal(blob0[k], blob1[k]) for k in blob0)
    finally:
        ctx.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------

def quad_grid(n_side=32, span=12.0):
    """n_side x n_side disjoint quads on a grid in the plane y = 0, facing up: (mesh, cell size)"""
    cell = 2 * span / n_side
    h = 0.4 * cell
    quads = []
    for iz in range(n_side):
        for ix in range(n_side):
            x, z = -span + (ix + 0.5) * cell, -span + (iz + 0.5) * cell
            quads.append(scenes._quad((x - h, 0, z - h), (x - h, 0, z + h), (x + h, 0, z + h), (x + h, 0, z - h), (0, 1, 0)))
    return scenes.Mesh([scenes._merge(quads)])


def test_rebuild_expands_fewer_records_than_a_refit_of_a_shuffled_quad_grid(hiplib):
    """What the call is for.  One mesh of 32 x 32 disjoint quads whose quads move to cells permuted by a seeded shuffle, the index
    arrays as committed: a refit keeps the commit's topology, whose leaves now each span random cells of the grid; a rebuild sorts the
    triangles again.  Deterministic counters of one counted render per route; the images are equal.  Nothing is asserted against the
    fresh SAH commit's counters (the Morton tree with one-triangle leaves is not a SAH tree; DESIGN.md section 5 has the figures)."""
    base = scenes.instanced_scene(n_side=2, n_unique=1, tris_per_mesh=64)
    grid = quad_grid()
    sc = scenes.Scene("quads", [scenes.plane_mesh(), grid], [base.instances[0], scenes.Instance(1, scenes.transform12(None, (0.0, -0.5, 0.0)), [3])],
                      base.materials, base.camera)
    perm = np.random.RandomState(2024).permutation(32 * 32)
    moved_mesh = copy.deepcopy(grid)
    s = moved_mesh.surfaces[0]
    s.vertices = np.ascontiguousarray(grid.surfaces[0].vertices.reshape(-1, 4, 3)[perm].reshape(-1, 3))
    shuffled = with_mesh(sc, 1, moved_mesh)
    w, h = 256, 144
    got = {}
    for route in ("refit", "rebuild", "fresh"):
        ctx = host.Context(0)
        try:
            ctx.build_scene(shuffled if route == "fresh" else sc, capi.BUILD_SAH_WATERTIGHT)
            ctx.set_params(w, h, 3, wire.ACCUM_REF_LDR8)
            ctx.set_camera(scenes.camera_block(sc.camera, w, h))
            if route != "fresh":
                ctx.render(1, 1)
                (ctx.update_mesh if route == "refit" else ctx.rebuild_mesh)(1, moved_mesh)
            ctx.accum_reset()
            ctx.render(2, 1, counted=True)
            st = ctx.stats()
            got[route] = (ctx.read_accum(), ctx.read_depth(), {k: int(st[k]) for k in ("rays", "blas_expand", "tri_tests")})
        finally:
            ctx.close()
    for route in ("refit", "rebuild", "fresh"):
        print("shuffled 32 x 32 quad grid, %s: %s" % (route, got[route][2]))
    print("rebuild / refit: blas_expand %.3f, tri_tests %.3f; rebuild / fresh commit: blas_expand %.3f, tri_tests %.3f" % (
        got["rebuild"][2]["blas_expand"] / got["refit"][2]["blas_expand"], got["rebuild"][2]["tri_tests"] / max(got["refit"][2]["tri_tests"], 1),
        got["rebuild"][2]["blas_expand"] / got["fresh"][2]["blas_expand"], got["rebuild"][2]["tri_tests"] / max(got["fresh"][2]["tri_tests"], 1)))
    for route in ("refit", "rebuild"):
        assert np.array_equal(got[route][0], got["fresh"][0]) and np.array_equal(got[route][1], got["fresh"][1]), route
        assert got[route][2]["rays"] == got["fresh"][2]["rays"]
    assert got["rebuild"][2]["blas_expand"] < got["refit"][2]["blas_expand"]
