"""jpt_scene_rebuild_tlas on the device: the sort against its host form, the records against the numpy restatement
(tests/np_tlas_rebuild.py), the images against fresh commits, the calls around it, and what it is for -- fewer instance visits than
a refit once instances have swapped places."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_skin
import np_tlas_rebuild as ref
from test_gpu_mesh_update import deform
from test_gpu_parity import _moved, _moves_for, _render_hip, rel_l2
from test_gpu_skin import SPARE, TUBE, host_rigs, pose as skin_pose, small_scene, tube_rigs, with_mesh
from test_tlas_rebuild_host import ORDER_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The sort keeps both key buffers in LDS up to 2048 instances (kTlasLdsKeys, jpt_tlas_rebuild.h) and in device memory beyond: 2048 and
# 2049 are the two sides of that boundary.  The others: a slot (4 / 5), a level (17, 65, 257, 1025, 4097), a wave (65), a tile of the
# block's 1024 threads (1025) and the largest count there is.
ORDER_COUNTS = [2, 4, 5, 17, 65, 257, 1025, 2048, 2049, 4097, 32767]


def all_t12(scene):
    return np.stack([np.asarray(i.transform, dtype=np.float32) for i in scene.instances])


@pytest.mark.parametrize("n", ORDER_COUNTS)
def test_device_order_equals_the_host_form(hiplib, n):
    rng = np.random.RandomState(n)
    lo = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    hi = lo + rng.uniform(0, 2, (n, 3)).astype(np.float32)
    if n > 64:
        lo[n // 2:n // 2 + 20] = lo[7]   # some equal centres: the index decides
        hi[n // 2:n // 2 + 20] = hi[7]
    keys, order = host.debug_tlas_order(0, lo, hi)
    want_keys, want_order = host.debug_tlas_order(-1, lo, hi)
    assert np.array_equal(keys, want_keys)
    assert np.array_equal(order, want_order)
    _, order_only = host.debug_tlas_order(0, lo, hi, with_keys=False)
    assert np.array_equal(order_only, want_order)


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_device_order_of_degenerate_boxes_equals_the_host_form(hiplib, name):
    lo, hi = ORDER_CASES[name]
    keys, order = host.debug_tlas_order(0, lo, hi)
    want_keys, want_order = host.debug_tlas_order(-1, lo, hi)
    assert np.array_equal(keys, want_keys)
    assert np.array_equal(order, want_order)


def _jitter_all(scene, seed):
    """every instance moved: a turn, a scale and a shift"""
    rng = np.random.RandomState(seed)
    moves = {}
    for i, inst in enumerate(scene.instances):
        t = np.asarray(inst.transform, np.float32)
        basis = t[:9].reshape(3, 3).astype(np.float64) @ scenes.rot_y(rng.uniform(-30, 30)) * rng.uniform(0.9, 1.1)
        moves[i] = scenes.transform12(basis, t[9:12] + rng.uniform(-0.4, 0.4, 3))
    return _moved(scene, moves)


def _quantised(nodes4):
    L = capi.lib()
    q = np.zeros((len(nodes4), 64), np.uint8)
    assert L.jpt_debug_quantize_nodes4(nodes4.ctypes.data_as(C.c_void_p), len(nodes4), q.ctypes.data_as(C.c_void_p)) == 0
    return q


@pytest.mark.parametrize("which", ["grid38", "seventeen"])
def test_records_after_a_rebuild_are_numpys_template_over_the_devices_boxes(hiplib, which):
    if which == "grid38":
        sc = scenes.instanced_scene(n_side=6, n_unique=3, tris_per_mesh=128)
    else:
        sc = scenes.instanced_scene(n_side=4, n_unique=2, tris_per_mesh=64)
        sc.instances = sc.instances[:17]
    n = len(sc.instances)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(64, 48, 2, wire.ACCUM_REF_LDR8)
        ctx.set_camera(scenes.camera_block(sc.camera, 64, 48))
        for step in range(2):   # the second rebuild replaces a rebuilt topology
            moved = _jitter_all(sc, 5 + step)
            ctx.rebuild_tlas(all_t12(moved))
            got = ctx.debug_tlas_records(n)
            assert got["root"] == 0
            _, order = ref.order(got["lo"], got["hi"])
            want = ref.records(n, order, got["lo"], got["hi"])
            mine = got["nodes4"].view(ref.NODE4).reshape(-1)
            assert len(mine) == len(want)
            assert np.array_equal(mine["child"], want["child"]), step
            assert np.array_equal(mine["lo"].view(np.uint32), want["lo"].view(np.uint32)), step
            assert np.array_equal(mine["hi"].view(np.uint32), want["hi"].view(np.uint32)), step
            assert np.array_equal(got["nodes4"], want.view(np.uint8).reshape(-1, 128)), step
            assert np.array_equal(got["nodesq"], _quantised(want.view(np.uint8).reshape(-1, 128))), step
        # a refit keeps the rebuilt topology, in another copy of the instance level
        moved = _jitter_all(sc, 9)
        ctx.refit_tlas(all_t12(moved))
        after = ctx.debug_tlas_records(n)
        want = ref.records(n, order, after["lo"], after["hi"])
        assert after["root"] == 0 and np.array_equal(after["nodes4"], want.view(np.uint8).reshape(-1, 128))
        assert np.array_equal(after["nodesq"], _quantised(want.view(np.uint8).reshape(-1, 128)))
    finally:
        ctx.close()


@pytest.mark.parametrize("asynchronous", [False, True])
def test_device_rebuild_renders_like_a_fresh_build(oracle, hiplib, asynchronous):
    """test_device_refit_renders_like_a_fresh_build's three steps with jpt_scene_rebuild_tlas"""
    sc = scenes.instanced_scene(n_side=6, n_unique=3, tris_per_mesh=128)
    w, h, bounces, frames = 160, 96, 3, 2
    cam = scenes.camera_block(sc.camera, w, h)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(w, h, bounces, wire.ACCUM_REF_LDR8)
        ctx.set_camera(cam)
        cur = sc
        for step in range(3):
            ctx.accum_reset()
            ctx.render(frames, 1, asynchronous=asynchronous)      # still reads the records of the previous step
            moves = _moves_for(cur, 11 + 7 * step, 5 + step)
            cur = _moved(cur, moves)
            ctx.rebuild_tlas(all_t12(cur))
            ctx.accum_reset()
            ctx.render(frames, 1, asynchronous=asynchronous)
            if asynchronous:
                ctx.render(1, 3, asynchronous=True)               # a second render in flight behind the rebuild
                ctx.accum_reset()
                ctx.render(frames, 1, asynchronous=True)
            after, after_depth = ctx.read_accum(), ctx.read_depth()
            fresh, _, fresh_depth = _render_hip(cur, cam, w, h, bounces, frames, wire.ACCUM_REF_LDR8, builder=capi.BUILD_SAH)
            assert np.array_equal(after, fresh) and np.array_equal(after_depth, fresh_depth), step
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        with pytest.raises(capi.JptError, match="jpt_scene_update_tlas"):
            ctx.render(1, 1)
        ctx.update_tlas()
        ctx.accum_reset()
        ctx.render(frames, 1)
        audit = ctx.read_accum()
        want, _, _, _, _ = oracle.render(oracle.build_scene(cur), cam, w, h, bounces, frames, 1, wire.ACCUM_REF_LDR8)
        assert rel_l2(audit, want) <= 1e-4
    finally:
        ctx.close()


def test_rebuild_of_sheared_instances_equals_a_fresh_commit_bit_for_bit(hiplib):
    sc = scenes.random_scene(5, coincident=False)
    w, h = 128, 96
    cam = scenes.camera_block(sc.camera, w, h)
    rng = np.random.default_rng(3)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(w, h, 2, wire.ACCUM_HDR_F32)
        ctx.set_camera(cam)
        moved = sc
        for step in range(2):
            ts = []
            for inst in moved.instances:
                t = np.array(inst.transform, dtype=np.float32).copy()
                t[:9] += rng.normal(0.0, 0.05, 9).astype(np.float32)
                t[9:12] += rng.normal(0.0, 0.1, 3).astype(np.float32)
                ts.append(t)
            moved = _moved(moved, {i: t for i, t in enumerate(ts)})
            ctx.rebuild_tlas(np.stack(ts))
            ctx.accum_reset()
            ctx.render(2, 1)
            got, got_depth = ctx.read_accum(), ctx.read_depth()
            fresh, _, fresh_depth = _render_hip(moved, cam, w, h, 2, 2, wire.ACCUM_HDR_F32, builder=capi.BUILD_SAH)
            bad = int(np.count_nonzero(got.view(np.uint32) != fresh.view(np.uint32)))
            bad_depth = int(np.count_nonzero(got_depth.view(np.uint32) != fresh_depth.view(np.uint32)))
            assert bad == 0 and bad_depth == 0, (step, bad, bad_depth)
    finally:
        ctx.close()


def test_queue_of_rebuilds_and_refits_stays_correct(oracle, hiplib):
    """Ten steps queued without ever waiting -- rebuild, refit, refit, rebuild, ... -- with a render and a device-side snapshot behind
    each.  More steps than copies of the instance level, so every copy is refitted while it still holds an older topology."""
    import torch
    sc = scenes.instanced_scene(n_side=6, n_unique=3, tris_per_mesh=128)
    w, h, bounces, frames = 480, 270, 3, 3
    cam = scenes.camera_block(sc.camera, w, h)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(w, h, bounces, wire.ACCUM_HDR_F32)
        ctx.set_camera(cam)
        stream = torch.cuda.ExternalStream(ctx.get_stream(), device=torch.device("cuda", 0))
        ptr, nbytes = ctx.device_accum()

        class _View:
            __cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<f4", "data": (ptr, False), "version": 2}

        accum = torch.as_tensor(_View(), device=torch.device("cuda", 0))
        cur, steps, snaps = sc, [], []
        with torch.cuda.stream(stream):
            for k in range(10):
                cur = _moved(cur, _moves_for(cur, 100 + k, 6))
                steps.append(cur)
                (ctx.rebuild_tlas if k % 3 == 0 else ctx.refit_tlas)(all_t12(cur))
                ctx.accum_reset()
                ctx.render(frames, 1 + k, asynchronous=True)
                snaps.append(accum.clone())
            stream.synchronize()
        ctx.sync()
        snaps = [s.cpu().numpy().reshape(h, w, 4) for s in snaps]
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        ctx.set_params(160, 90, bounces, wire.ACCUM_REF_LDR8)
        small_cam = scenes.camera_block(sc.camera, 160, 90)
        ctx.set_camera(small_cam)
        ctx.update_tlas()
        ctx.render(2, 1)
        audit = ctx.read_accum()
    finally:
        ctx.close()
    for k, scene_k in enumerate(steps):
        fresh = host.Context(0)
        fresh.build_scene(scene_k, capi.BUILD_SAH)
        fresh.set_params(w, h, bounces, wire.ACCUM_HDR_F32)
        fresh.set_camera(cam)
        fresh.render(frames, 1 + k)
        want = fresh.read_accum()
        fresh.close()
        assert np.array_equal(snaps[k], want), k
    want, _, _, _, _ = oracle.render(oracle.build_scene(cur), small_cam, 160, 90, bounces, 2, 1, wire.ACCUM_REF_LDR8)
    assert rel_l2(audit, want) <= 1e-4


def _watertight_frame(ctx, spp=2):
    ctx.accum_reset()
    ctx.render(spp, 1, counted=True)
    return ctx.read_accum(), ctx.read_depth(), ctx.stats()["rays"]


def _watertight_ctx(scene, w=160, h=96):
    ctx = host.Context(0)
    ctx.build_scene(scene, capi.BUILD_SAH_WATERTIGHT)
    ctx.set_params(w, h, 3)
    ctx.set_camera(scenes.camera_block(scene.camera, w, h))
    return ctx


def _assert_frames_equal(got, want, what):
    for g, x in zip(got[:2], want[:2]):
        assert not (~((g == x) | (np.isnan(g) & np.isnan(x)))).any(), what
    assert got[2] == want[2], what


@pytest.mark.parametrize("route", ["update_mesh", "pose_mesh"])
def test_mesh_updates_after_a_rebuild_equal_a_fresh_commit(hiplib, route):
    sc = small_scene()
    moved = _jitter_all(sc, 3)
    bind = sc.meshes[TUBE]
    if route == "update_mesh":
        new_mesh = deform(bind, 1)
    else:
        rigs = tube_rigs(bind)
        pal, bw = skin_pose(1)
        new_mesh = np_skin.skin_mesh(bind, rigs, 4, pal, bw)
    ctx = _watertight_ctx(sc)
    try:
        ctx.render(1, 1)
        ctx.rebuild_tlas(all_t12(moved))
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(moved), "rebuild")
        if route == "update_mesh":
            ctx.update_mesh(TUBE, new_mesh)
        else:
            ctx.set_mesh_rig(TUBE, bind, host_rigs(rigs), 4, 2)
            ctx.pose_mesh(TUBE, pal, bw)
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(moved, TUBE, new_mesh)), route)
        # and a rebuild over the deformed mesh's root boxes
        again = _jitter_all(moved, 4)
        ctx.rebuild_tlas(all_t12(again))
        _assert_frames_equal(_watertight_frame(ctx), _fresh_watertight(with_mesh(again, TUBE, new_mesh)), route + ", rebuild")
    finally:
        ctx.close()


def _fresh_watertight(scene):
    ctx = _watertight_ctx(scene)
    try:
        return _watertight_frame(ctx)
    finally:
        ctx.close()


STALE_HOST_COPY = "a mesh was deformed on the device (jpt_scene_update_mesh): the host's copy of the scene is stale until the next jpt_scene_commit"


def _five_instances():
    """small_scene with its spare box named by two more instances: three meshes, five instances"""
    sc = small_scene()
    sc.instances = sc.instances + [scenes.Instance(SPARE, scenes.transform12(scenes.rot_y(25.0), (-1.1, 0.5, 0.4)), [1]),
                                   scenes.Instance(SPARE, scenes.transform12(np.eye(3) * 0.6, (1.2, 0.3, 0.9)), [4])]
    return sc


def _small_ctx(scene):
    ctx = host.Context(0)
    ctx.build_scene(scene, capi.BUILD_SAH_WATERTIGHT)
    ctx.set_params(64, 48, 2)
    ctx.set_camera(scenes.camera_block(scene.camera, 64, 48))
    return ctx


def _small_frame(ctx, asynchronous):
    """2 frames; (accum, depth, rays) as _watertight_frame gives them -- a queued render is not counted: its ray count is what the statistics hold"""
    ctx.accum_reset()
    ctx.render(2, 1, counted=not asynchronous, asynchronous=asynchronous)
    return ctx.read_accum(), ctx.read_depth(), ctx.stats()["rays"]


def test_every_scene_update_in_one_context_queued_equals_synced_and_fresh_commits(hiplib):
    """Every way the device's scene moves ahead of the host and is put back, in one context: refit, render, rebuild, render, jpt_scene_update_mesh,
    pose, a refit into a copy whose tail is a topology behind, render, the host route refused for the deformed mesh, a whole commit, a refit
    that makes the copies again, render.  Queued without a wait up to the third image, every image equals, bit for bit, the one of the same
    calls with jpt_sync after each; the third and the fourth equal a fresh commit of the same vertices and transforms."""
    import torch
    sc = _five_instances()
    bind, rigs = sc.meshes[TUBE], tube_rigs(sc.meshes[TUBE])
    pal, bw = skin_pose(1)
    posed, bent = np_skin.skin_mesh(bind, rigs, 4, pal, bw), deform(sc.meshes[SPARE], 1)
    m1 = _jitter_all(sc, 3)
    m2 = _jitter_all(m1, 4)
    m3 = _jitter_all(m2, 5)
    m4 = _jitter_all(m3, 6)
    at8, at12 = (with_mesh(with_mesh(m, SPARE, bent), TUBE, posed) for m in (m3, m4))

    def run(synced):
        ctx = _small_ctx(sc)
        after = ctx.sync if synced else (lambda: None)
        try:
            ctx.set_mesh_rig(TUBE, bind, host_rigs(rigs), 4, 2)
            stream = torch.cuda.ExternalStream(ctx.get_stream(), device=torch.device("cuda", 0))
            ptr, nbytes = ctx.device_accum()

            class _View:
                __cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<f4", "data": (ptr, False), "version": 2}

            accum, snaps = torch.as_tensor(_View(), device=torch.device("cuda", 0)), []

            def queued_frame():
                ctx.accum_reset()
                ctx.render(2, 1, asynchronous=True)
                after()
                snaps.append(accum.clone())

            with torch.cuda.stream(stream):
                ctx.refit_tlas(all_t12(m1))                    # 1
                after()
                queued_frame()                                 # 2
                ctx.rebuild_tlas(all_t12(m2))                  # 3
                after()
                queued_frame()                                 # 4
                ctx.update_mesh(SPARE, bent)                   # 5
                after()
                ctx.pose_mesh(TUBE, pal, bw)                   # 6
                after()
                ctx.refit_tlas(all_t12(m3))                    # 7: copy 5's tail still holds the committed topology
                after()
                third = _small_frame(ctx, True)                # 8
            first, second = (s.cpu().numpy().reshape(48, 64, 4) for s in snaps)
            assert ctx._lib.jpt_scene_update_tlas(ctx.h) == -4 and ctx.last_error() == STALE_HOST_COPY   # 9
            ctx.build_scene(at8, capi.BUILD_SAH_WATERTIGHT)    # 10
            after()
            ctx.refit_tlas(all_t12(m4))                        # 11
            after()
            return first, second, third, _small_frame(ctx, False)   # 12
        finally:
            ctx.close()

    def fresh(scene, asynchronous):
        ctx = _small_ctx(scene)
        try:
            return _small_frame(ctx, asynchronous)
        finally:
            ctx.close()

    queued, synced = run(False), run(True)
    for k in (0, 1):
        assert np.array_equal(queued[k].view(np.uint32), synced[k].view(np.uint32)), "image %d" % (k + 1)
    _assert_frames_equal(queued[2], synced[2], "image 3, queued against synced")
    _assert_frames_equal(queued[3], synced[3], "image 4, queued against synced")
    _assert_frames_equal(queued[2], fresh(at8, True), "image 3 against a fresh commit")
    _assert_frames_equal(queued[3], fresh(at12, False), "image 4 against a fresh commit")


def test_queries_and_guides_follow_a_rebuild(hiplib):
    sc = scenes.instanced_scene(n_side=6, n_unique=3, tris_per_mesh=128)
    moved = _jitter_all(sc, 8)
    w, h = 96, 64
    cam = scenes.camera_block(sc.camera, w, h)
    xy = np.stack(np.meshgrid(np.arange(0, w, 3) + 0.5, np.arange(0, h, 3) + 0.5), axis=-1).reshape(-1, 2).astype(np.float32)

    def answers(ctx):
        ctx.accum_reset()
        ctx.render(1, 1)
        ctx.denoise()
        return [ctx.query_pixels(xy)] + list(ctx.read_guides())

    got_ctx, want_ctx = host.Context(0), host.Context(0)
    try:
        for c, scene in ((got_ctx, sc), (want_ctx, moved)):
            c.build_scene(scene, capi.BUILD_SAH)
            c.set_params(w, h, 2, wire.ACCUM_HDR_F32)
            c.set_camera(cam)
        before = answers(got_ctx)
        got_ctx.rebuild_tlas(all_t12(moved))
        got, want = answers(got_ctx), answers(want_ctx)
        assert got[0].tobytes() == want[0].tobytes()
        assert got[0].tobytes() != before[0].tobytes()
        for g, x in zip(got[1:], want[1:]):
            assert np.array_equal(g.view(np.uint32), x.view(np.uint32))
    finally:
        got_ctx.close()
        want_ctx.close()


_CULL_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from gdpathtracing_amd import capi, host, scenes, wire
from test_gpu_tlas_rebuild import cull_scene_steps, all_t12
sc, steps = cull_scene_steps()
w, h = 320, 180
ctx = host.Context(0)
ctx.build_scene(sc if sys.argv[2] == "rebuild" else steps[-1], capi.BUILD_SAH)
ctx.set_params(w, h, 3, wire.ACCUM_REF_LDR8)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
if sys.argv[2] == "rebuild":
    ctx.render(1, 1)
    for s in steps:
        ctx.rebuild_tlas(all_t12(s))
ctx.accum_reset()
ctx.render(2, 1, counted=True)
st = ctx.stats()
np.savez(sys.argv[3], accum=ctx.read_accum(), depth=ctx.read_depth(), rays=st["rays"], culled=st["sky_culled"])
ctx.close()
"""


def cull_scene_steps():
    sc = scenes.demo_scene(2500)
    cur, steps = sc, []
    for step in range(2):
        moves = {2: scenes.transform12(scenes.rot_y(40.0 * (step + 1)) * 1.2, np.asarray(sc.instances[2].transform[9:12]) + np.array([0.6 * (step + 1), 0.2, 0.0])),
                 3: scenes.transform12(scenes.rot_y(-25.0 * (step + 1)) * 0.8, np.asarray(sc.instances[3].transform[9:12]) + np.array([-0.9 * (step + 1), 0.0, 0.3]))}
        cur = _moved(cur, moves)
        steps.append(cur)
    return sc, steps


def test_rebuild_keeps_the_sky_cull_exact(hiplib, tmp_path):
    """The demo scene leaves most of the frame to the sky: after rebuilds the primary launch culls by the host mirror's root boxes.
    Sums, depth and the counted rays equal the same run with the cull off and a fresh commit's."""
    got = {}
    for route, cull in (("rebuild", "1"), ("rebuild", "0"), ("fresh", "1")):
        out = str(tmp_path / ("%s%s.npz" % (route, cull)))
        r = subprocess.run([sys.executable, "-c", _CULL_CHILD, ROOT, route, out], env=dict(os.environ, JPT_SKY_CULL=cull),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        got[route, cull] = np.load(out)
    a, b, f = got["rebuild", "1"], got["rebuild", "0"], got["fresh", "1"]
    assert int(a["culled"]) > 0 and int(b["culled"]) == 0
    for other in (b, f):
        assert np.array_equal(a["accum"], other["accum"]) and np.array_equal(a["depth"], other["depth"])
        assert int(a["rays"]) == int(other["rays"])


def test_light_sampling_follows_a_rebuilt_emitter(hiplib):
    sc = scenes.instanced_scene(n_side=6, n_unique=3, tris_per_mesh=128)
    moved = _jitter_all(sc, 12)   # the emissive plane (instance 0) moves with the rest
    w, h = 128, 80
    cam = scenes.camera_block(sc.camera, w, h)
    frames = {}
    for route in ("rebuild", "fresh"):
        ctx = host.Context(0)
        try:
            ctx.build_scene(sc if route == "rebuild" else moved, capi.BUILD_SAH)
            ctx.set_params(w, h, 3, wire.ACCUM_HDR_F32)
            ctx.set_camera(cam)
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
            if route == "rebuild":
                ctx.render(1, 1)
                ctx.rebuild_tlas(all_t12(moved))
                ctx.accum_reset()
            ctx.render(2, 1)
            frames[route] = (ctx.read_accum(), ctx.read_depth())
        finally:
            ctx.close()
    assert np.array_equal(frames["rebuild"][0].view(np.uint32), frames["fresh"][0].view(np.uint32))
    assert np.array_equal(frames["rebuild"][1].view(np.uint32), frames["fresh"][1].view(np.uint32))


def _shuffled_grid_counters(with_planes):
    """the counters and images of one counted render of the shuffled grid after a refit, after a rebuild and of a fresh commit"""
    sc = scenes.instanced_scene(n_side=16, n_unique=1, tris_per_mesh=64)
    first = 2   # (instanced_scene puts a light plane and a ground plane, both as wide as the grid, before the grid's instances)
    if not with_planes:
        sc.instances = sc.instances[first:]
        first = 0
    assert len(sc.instances) == first + 256
    perm = np.random.RandomState(2024).permutation(256)
    shuffled = _moved(sc, {first + i: sc.instances[first + int(perm[i])].transform for i in range(256)})
    w, h = 256, 144
    cam = scenes.camera_block(sc.camera, w, h)
    got = {}
    for route in ("refit", "rebuild", "fresh"):
        ctx = host.Context(0)
        try:
            ctx.build_scene(shuffled if route == "fresh" else sc, capi.BUILD_SAH)
            ctx.set_params(w, h, 3, wire.ACCUM_REF_LDR8)
            ctx.set_camera(cam)
            if route != "fresh":
                ctx.render(1, 1)
                (ctx.refit_tlas if route == "refit" else ctx.rebuild_tlas)(all_t12(shuffled))
            ctx.accum_reset()
            ctx.render(2, 1, counted=True)
            st = ctx.stats()
            got[route] = (ctx.read_accum(), ctx.read_depth(), {k: int(st[k]) for k in ("rays", "inst_visits", "tlas_expand")})
        finally:
            ctx.close()
    what = "shuffled 16 x 16 grid" + (" between a light and a ground plane" if with_planes else "")
    for route in ("refit", "rebuild", "fresh"):
        print("%s, %s: %s" % (what, route, got[route][2]))
    print("rebuild / refit: inst_visits %.3f, tlas_expand %.3f; rebuild / fresh commit: inst_visits %.3f, tlas_expand %.3f" % (
        got["rebuild"][2]["inst_visits"] / got["refit"][2]["inst_visits"], got["rebuild"][2]["tlas_expand"] / got["refit"][2]["tlas_expand"],
        got["rebuild"][2]["inst_visits"] / got["fresh"][2]["inst_visits"], got["rebuild"][2]["tlas_expand"] / got["fresh"][2]["tlas_expand"]))
    for route in ("refit", "rebuild"):
        assert np.array_equal(got[route][0], got["fresh"][0]) and np.array_equal(got[route][1], got["fresh"][1]), route
        assert got[route][2]["rays"] == got["fresh"][2]["rays"]
    return {route: got[route][2] for route in got}


def test_rebuild_visits_fewer_instances_than_a_refit_of_a_shuffled_grid(hiplib):
    """What the call is for.  A 16 x 16 grid of instances of one mesh whose transforms are permuted by a seeded shuffle: a refit keeps
    the commit's topology, whose records now each span the grid; a rebuild sorts the instances again.  Deterministic counters of one
    counted render; the images are equal.  (Measured figures: DESIGN.md section 5.)"""
    c = _shuffled_grid_counters(with_planes=False)
    assert c["rebuild"]["inst_visits"] < c["refit"]["inst_visits"]
    assert c["rebuild"]["tlas_expand"] < c["refit"]["tlas_expand"]


def test_rebuild_of_a_grid_between_two_scene_wide_planes(hiplib):
    """The same grid as instanced_scene makes it, between a light plane and a ground plane as wide as the grid -- two instances whose
    centres fall in the middle of the Morton order while their boxes span the scene.  The rebuilt tree still expands far fewer records
    than the refitted one (measured 777 403 against 2 819 489; a fresh SAH commit: 420 655), but it enters MORE instances (112 090
    against the refit's 99 326 and the commit's 95 826): the commit's topology keeps the planes near the root, where a near-first walk
    finds the ground early and prunes the instances behind it, and the refit inherits that.  Only the images and the record count are
    asserted here; the figure is why INTEGRATION.md says to keep scene-wide instances in mind when choosing between the calls."""
    c = _shuffled_grid_counters(with_planes=True)
    assert c["rebuild"]["tlas_expand"] < c["refit"]["tlas_expand"]
