"""The tracing launches carry the walk's flags `have` and `in_blas` as two wave-uniform lane masks and the stack position as the LDS
address of the lane's next entry (walk_round_masked, trace_queue: jpt_kernels_wf2.hip; Traversal::Masked, push_at / pop_at:
jpt_trace_core.h).  No ray's steps change, so every render here equals the CPU oracle's pixel for pixel -- accumulation and rgba8, both
accumulation modes, once blocking and three times queued -- on the native tree (four-child records: the form those kernels run in):

 (a) a walk deeper than the LDS part of the stack: the spill region and the clamped read at its boundary, under the address form;
 (b) 18 instances: lanes leave an instance into a TLAS record, and the sentinel comes off as the LAST entry (sp == 0 right after it);
 (c) no instance at all, and an instance of a mesh without triangles: `have` false from the start;
 (d) one partly filled wave that drains, and a frame count that divides nothing;
 (e) a counting render of (b): the per-ray event counters equal those of the same render with JPT_PIPELINE=0 (another process: the
     switch is read once) and the oracle's ray count."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [wire.ACCUM_REF_LDR8, wire.ACCUM_HDR_F32]
K_STACK_LDS, K_STACK_SPILL = 20, 76   # jpt_trace_core.h: kStackLds, kStackSpill
EMPTY_CHILD = -(2 ** 31)


def fan_mesh(n, seed=5):
    """n large triangles, nearly coincident (0.2 deep in all, jittered by 1e-4): every ray through the fan crosses all of them, every
    box of their tree overlaps every other, and a walk that descends nearest-first leaves the siblings of every level on its stack"""
    rng = np.random.RandomState(seed)
    z = (np.arange(n, dtype=np.float64) / n) * 0.2 - 0.1
    base = np.array([[-6.0, -5.0, 0.0], [6.0, -5.0, 0.0], [0.0, 7.0, 0.0]])
    v = np.repeat(base[None], n, axis=0) + rng.uniform(-0.02, 0.02, (n, 3, 3))
    v[:, :, 2] = z[:, None] + rng.uniform(-1e-4, 1e-4, (n, 3))
    idx = np.arange(3 * n).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return scenes.Mesh([scenes.Surface(v.reshape(-1, 3), np.tile([0.0, 0.0, 1.0], (3 * n, 1)), np.tile([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], (n, 1)), idx)])


def deep_scene():
    sc = scenes.cornell_scene()
    sc.name = "cornell_fan"
    sc.meshes.append(fan_mesh(4000))
    sc.instances.append(scenes.Instance(len(sc.meshes) - 1, scenes.transform12(None, (0, 0, 2.0)), [3]))
    return sc


def empty_scene():
    base = scenes.cornell_scene()
    return scenes.Scene("empty", [], [], base.materials, base.camera)


def empty_mesh_scene():
    from tests.test_oracle_builder import with_empty_mesh
    sc = with_empty_mesh(scenes.cornell_scene(), "last")
    sc.name = "cornell_empty_mesh"
    return sc


SCENES = {
    "deep": (deep_scene, 64, 64, 2, 3),
    "instances": (lambda: scenes.instanced_scene(n_side=4, n_unique=2, tris_per_mesh=96), 64, 64, 2, 3),
    "no_instance": (empty_scene, 32, 16, 2, 3),
    "empty_mesh": (empty_mesh_scene, 48, 40, 2, 3),
    "one_wave": (scenes.cornell_scene, 8, 8, 1, 3),
    "three_frames": (scenes.cornell_scene, 40, 24, 3, 3),
}
_made, _wanted = {}, {}


def scene_of(name):
    if name not in _made:
        _made[name] = SCENES[name][0]()
    return _made[name]


def wanted(oracle, name, mode):
    """the oracle's render of a case, made once"""
    if (name, mode) not in _wanted:
        _, w, h, frames, bounces = SCENES[name]
        sc = scene_of(name)
        cam = scenes.camera_block(sc.camera, w, h)
        want, want_ldr, _, cnt, _ = oracle.render(oracle.build_scene(sc), cam, w, h, bounces, frames, 1, mode)
        _wanted[(name, mode)] = (want, want_ldr, cnt)
    return _wanted[(name, mode)]


def context(name, mode, builder=capi.BUILD_SAH):
    _, w, h, _, bounces = SCENES[name]
    sc = scene_of(name)
    ctx = host.Context(0)
    ctx.build_scene(sc, builder)
    ctx.set_params(w, h, bounces, mode)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    return ctx


def check(oracle, name, mode):
    """one blocking render and three queued ones (each from a cleared accumulation), each against the oracle: 0 differing pixels"""
    frames = SCENES[name][3]
    want, want_ldr, _ = wanted(oracle, name, mode)
    ctx = context(name, mode)
    try:
        ctx.render(frames, 1)
        got, got_ldr = ctx.read_accum(), ctx.read_ldr()
        for _ in range(3):
            ctx.accum_reset()
            ctx.render(frames, 1, asynchronous=True)
        ctx.sync()
        queued, queued_ldr = ctx.read_accum(), ctx.read_ldr()
    finally:
        ctx.close()
    for how, a, l in (("blocking", got, got_ldr), ("queued", queued, queued_ldr)):
        print(name, SCENES[name][1:], mode, how, "differing pixels: accumulation", int((a != want).any(axis=-1).sum()), "rgba8",
              int((l != want_ldr).any(axis=-1).sum()))
    assert np.array_equal(got, want) and np.array_equal(got_ldr, want_ldr)
    assert np.array_equal(queued, want) and np.array_equal(queued_ldr, want_ldr)


def need4(child, first, root):
    """need4 of jpt_builder.cpp (compute_stack_need) on one mesh's four-child records: the most entries a walk below `root` can hold"""
    memo = {}
    order = [root - first]
    for r in order:   # parents before children
        order.extend(int(c) - first for c in child[r] if c >= 0)
    for r in reversed(order):
        kids = [int(c) for c in child[r] if c != EMPTY_CHILD]
        deepest = max([memo[c - first] for c in kids if c >= 0], default=0)
        memo[r] = len(kids) - 1 + deepest if kids else 0
    return memo[root - first]


def test_the_deep_scene_needs_more_than_the_lds_part_of_the_stack(hiplib):
    """compute_stack_need's figure for the fan, restated on the mesh's records as the device holds them.  (jpt_debug_mesh_records reads
    them from a JPT_BUILD_SAH_WATERTIGHT commit: the same native tree, without reach records.)  A scene's need is the instance level's
    + 1 (the sentinel) + the deepest mesh's; an upload that needs more than the kernels hold is refused, so both commits of this
    module also show that it stays within capacity."""
    ctx = context("deep", wire.ACCUM_REF_LDR8, capi.BUILD_SAH_WATERTIGHT)
    try:
        rec = ctx.debug_mesh_records(len(scene_of("deep").meshes) - 1)
    finally:
        ctx.close()
    child = rec["nodes4"].view(np.int32).reshape(-1, 32)[:, 12:16]
    need = need4(child, rec["first_record"], rec["root"]) + 1
    print("fan of 4000 triangles:", rec["n_records"], "records, stack need of a walk inside it (with the sentinel)", need)
    assert K_STACK_LDS < need <= K_STACK_LDS + K_STACK_SPILL


@pytest.mark.parametrize("mode", MODES)
def test_a_walk_deeper_than_the_lds_part_of_the_stack(oracle, hiplib, mode):
    check(oracle, "deep", mode)


@pytest.mark.parametrize("mode", MODES)
def test_many_instances_and_the_sentinel_as_the_last_entry(oracle, hiplib, mode):
    assert len(scene_of("instances").instances) == 18
    check(oracle, "instances", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["no_instance", "empty_mesh"])
def test_scenes_whose_walks_hold_no_record_from_the_start(oracle, hiplib, name, mode):
    check(oracle, name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["one_wave", "three_frames"])
def test_a_partly_filled_wave_that_drains(oracle, hiplib, name, mode):
    check(oracle, name, mode)


# what one ray's walk and one path's vertices count, whatever the schedule (Stats.phase counts the waves' rounds: it depends on which
# wave's refill took which rays, so it is not compared)
EVENTS = ("rays", "blas_expand", "tri_tests", "tlas_expand", "inst_visits", "shaded_hits", "sky_culled", "set_aside", "set_aside_dropped",
          "walk_steps_max", "walk_steps_hist", "zero_throughput")

CHILD = """
import json, sys
sys.path.insert(0, %r)
from tests import test_gpu_round_masks as t
from gdpathtracing_amd import wire
ctx = t.context("instances", wire.ACCUM_REF_LDR8)
ctx.render(t.SCENES["instances"][3], 1, counted=True)
print("EVENTS " + json.dumps({k: ctx.stats()[k] for k in t.EVENTS}))
ctx.close()
"""


def test_counters_of_a_counting_render_with_and_without_pipelining(oracle, hiplib):
    frames = SCENES["instances"][3]
    _, _, cnt = wanted(oracle, "instances", wire.ACCUM_REF_LDR8)
    ctx = context("instances", wire.ACCUM_REF_LDR8)
    try:
        ctx.render(frames, 1, counted=True)
        here = {k: ctx.stats()[k] for k in EVENTS}
    finally:
        ctx.close()
    env = dict(os.environ, JPT_PIPELINE="0")
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    serial = json.loads([l for l in p.stdout.splitlines() if l.startswith("EVENTS ")][0][len("EVENTS "):])
    print("counting render, 18 instances:", here)
    assert here == serial
    # every walked ray takes the instance level's root record; more TLAS record steps than walks: lanes do go on into further ones
    assert here["rays"] == cnt["rays"] and here["inst_visits"] > 0 and here["tlas_expand"] > sum(here["walk_steps_hist"]) > 0
