"""Every kernel that walks the tree, on trees deeper than the LDS part of its stack.  Traversal's stack (jpt_trace_core.h) comes in
four forms -- 20 rows in LDS and 76 in scratch under the address form (wf2_trace, every wf2_primary* variant), 18 + 78 with two rows
lent to the pool (coop_walk's tail phase), all 96 rows in LDS without a spill pointer (wf2_occlude, wf2_occlude_lt, query_kernel, the
guide kernel) and all 96 in scratch (wf2_finish) -- and test_gpu_round_masks.py's "deep" render holds more than 20 entries in the
first of them only.  Here shadow rays of both kinds of MIS, jpt_query_rays in both modes, the guide pass, the set-aside / tie route,
the cooperative tail and the primary-ray families other than the pinhole walk that deep too.

The scenes.  shutter_mesh(n): fan_mesh's stack of n near-coincident layers (same z spacing and jitter), each layer one of two right
triangles that halve the rectangle, B with probability 1/3.  Every layer's box spans the rectangle, a ray is covered by a third or
two thirds of the layers: its closest hit usually lies in a sibling of the first leaf reached -- one of the entries at the top of
the stack -- so a lost or misread entry shows as a farther hit or a missing occluder.  (With fan_mesh every layer covers every ray,
the first leaf wins and a lost entry changes nothing.)  shutter_stack: N_STACK instances of one shutter, one behind the other along
z, nothing else.  deep_cornell: Cornell's box with such a stack, a quarter the size, standing between the camera and the blocks with
its lower edge near the floor: the strip of floor in front of it sees the light only through it.

The regime is asserted.  guaranteed_depth: the fewest entries a near-first walk holds at its first leaf when the ray enters every
child box, whatever order the kernel picks (hit.t culls nothing before the first hit): the minimum over root-to-leaf paths of the
sum of (children - 1).  It is evaluated on the device's records (jpt_debug_tlas_records, jpt_debug_mesh_records; a JPT_BUILD_SAH
commit's mesh records are read from the JPT_BUILD_SAH_WATERTIGHT commit of the same scene -- the same native tree without reach
records, as in test_gpu_round_masks.py; a native upload's records cannot be read back: its walk is held to the same brute force),
with 1 for the instance sentinel, and the rays the bound is claimed for are shown in float64 to enter every child box of every
record (the float boxes, grown by nothing: the quantised ones are larger).  GUARANTEED = 24: rows 20 .. 23 lie beyond both LDS
parts.  The instance count is what makes it hold: the SAH tree of 4000 layers has a leaf four records below its root (12 entries;
the balanced Morton tree of a rebuild: 17), and sixteen instances add 6 + 1, so N_STACK is 256: four more levels of the instance
tree.  In deep_cornell the first instance a ray reaches may be one of Cornell's own, so only the shutters count there: an entered
child that holds a shutter is still on the stack when the walk reaches its FIRST shutter (had the walk been below it, it would have
reached a shutter there), provided nothing was hit in front of the stack; deep_cornell_regime checks that too.

All comparisons are exact bits, NaN matching NaN.  Measured depths and needs: LAB_NOTEBOOK.md, "Deep walks"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_path as npp
import np_query as nq
import np_tlas_rebuild as ntr
import test_gpu_family_scene_changes as fam
from test_gpu_environment import assert_same, images
from test_gpu_light_sampling import sun_map
from test_gpu_round_masks import EMPTY_CHILD, K_STACK_LDS, K_STACK_SPILL, fan_mesh, need4

pytestmark = pytest.mark.gpu

F = np.float32
MODES = [wire.ACCUM_REF_LDR8, wire.ACCUM_HDR_F32]
SAH, WATERTIGHT = capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT
WF, AUDIT = capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT
GUARANTEED = 24        # rows 20 .. 23: beyond the LDS part of the tracing kernels (20) and of the tail phase (18)
CAPACITY = K_STACK_LDS + K_STACK_SPILL
N_LAYERS = 4000
TRI_A = np.array([[-6.0, -5.0], [6.0, -5.0], [-6.0, 7.0]])
TRI_B = np.array([[6.0, 7.0], [-6.0, 7.0], [6.0, -5.0]])
FAN_BASE = np.array([[-6.0, -5.0], [6.0, -5.0], [0.0, 7.0]])   # fan_mesh's triangle


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------

def shutter_mesh(n, seed=5, duplicated=0):
    """fan_mesh(n, seed) with every layer's triangle replaced by A or B (B with probability 1/3, seeded): the layer keeps the fan's z
    and its jitter.  duplicated: that many layers once more with exactly the same vertices (exact ties) -- half of them the last
    layers of the stack (the first in the way of a ray towards -z), half spread over it"""
    fan = fan_mesh(n, seed).surfaces[0]
    v = fan.vertices.reshape(n, 3, 3).astype(np.float64)
    is_b = np.random.RandomState(seed + 1000).random_sample(n) < 1.0 / 3.0
    v[:, :, :2] += np.where(is_b[:, None, None], TRI_B[None], TRI_A[None]) - FAN_BASE[None]
    if duplicated:
        half = duplicated // 2
        v = np.concatenate([v, v[n - half:], v[np.arange(duplicated - half) * (n // (duplicated - half))]])
    m = len(v)
    idx = np.arange(3 * m).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return scenes.Mesh([scenes.Surface(v.reshape(-1, 3), np.tile([0.0, 0.0, 1.0], (3 * m, 1)), np.tile([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], (m, 1)), idx)])


N_STACK, STACK_STEP = 256, 0.01     # (sixteen instances guarantee 6 + 1 + 12 = 19 entries on the SAH trees: see the module's docstring)


def shutter_stack():
    base = scenes.cornell_scene()
    inst = [scenes.Instance(0, scenes.transform12(None, (0.0, 0.0, STACK_STEP * k)), [3]) for k in range(N_STACK)]
    return scenes.Scene("shutter_stack", [shutter_mesh(N_LAYERS)], inst, base.materials, base.camera)


SHUTTER_SCALE, SHUTTER_AT, SHUTTER_STEP = 0.25, (0.0, -1.5, 2.2), 0.002
SHUTTER_MESH, FIRST_SHUTTER = 4, 4       # deep_cornell: the shutter is mesh 4, its instances follow Cornell's four


def deep_cornell(shutter=True, duplicated=0, material=3):
    """test_gpu_round_masks.deep_scene with a stack of shutters in place of the fan, a quarter the size: it spans x -1.5 .. 1.5 and
    y -2.75 .. 0.25 from z = 2.2 to 2.71, facing the camera, in front of the blocks.  A segment from the floor in front of it
    (z = 2.95) to the light (y = 2.96, z -1 .. 1) passes z = 2.74 at y = -2.6 and z = 2.2 at y = -1.5: that strip of the floor sees
    the light only through the whole stack.  shutter=False: the mesh stays, no instance names it."""
    sc = scenes.cornell_scene()
    sc.name = "deep_cornell"
    sc.meshes.append(shutter_mesh(N_LAYERS, duplicated=duplicated))
    if shutter:
        x, y, z = SHUTTER_AT
        sc.instances += [scenes.Instance(SHUTTER_MESH, scenes.transform12(np.eye(3) * SHUTTER_SCALE, (x, y, z + SHUTTER_STEP * k)), [material])
                         for k in range(N_STACK)]
    return sc


_scene_cache = {}


def scene_of(name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _scene_cache:
        _scene_cache[key] = {"shutter_stack": shutter_stack, "deep_cornell": deep_cornell}[name](**kw)
    return _scene_cache[key]


def all_transforms(sc):
    return np.stack([np.asarray(i.transform, F) for i in sc.instances])


# ---- the regime -------------------------------------------------------------------------------------------------------------------------

def guaranteed_depth(child_words, root, counts=None):
    """child_words: int32 [R, 4] (>= 0 a record of this array, < 0 a leaf, EMPTY_CHILD none).  The minimum over root-to-leaf paths of
    the sum of (children - 1): what a near-first walk below `root` holds when it reaches its first leaf, if the ray enters every
    child box -- the walk descends into ONE child of every record on the way and leaves the others on the stack, whichever it picks.
    counts(leaf word) -> bool: the leaves that count (None: all); with it, the paths end at such leaves and only children that hold
    one are counted.  Returns (the minimum, the records below root parents first, per record and slot: does the child hold a leaf
    that counts)."""
    order = [int(root)]
    for r in order:   # parents before children
        order.extend(int(c) for c in child_words[r] if c >= 0)
    memo, holds = {}, np.zeros(child_words.shape, bool)
    for r in reversed(order):
        best = None
        for k, c in enumerate(int(c) for c in child_words[r]):
            if c == EMPTY_CHILD:
                continue
            if c >= 0:
                holds[r, k] = memo[c] is not None
                below = memo[c]
            else:
                holds[r, k] = counts is None or bool(counts(c))
                below = 0 if holds[r, k] else None
            if below is not None:
                best = below if best is None else min(best, below)
        memo[r] = None if best is None else int(holds[r].sum()) - 1 + best
    assert memo[int(root)] is not None, "no leaf that counts"
    return memo[int(root)], order, holds


def boxes_of(nodes4, records, slots=None):
    """the float boxes (lo, hi: float64 [M, 3]) of the non-empty children of the records listed; slots: bool [R, 4], only those"""
    rec = np.ascontiguousarray(nodes4).view(ntr.NODE4).reshape(-1)
    used = rec["child"] != EMPTY_CHILD
    if slots is not None:
        used &= slots
    used = used[np.asarray(records)]
    rec = rec[np.asarray(records)]
    return rec["lo"].astype(np.float64).transpose(0, 2, 1)[used], rec["hi"].astype(np.float64).transpose(0, 2, 1)[used]


def rays_enter_every_box(lo, hi, o, d):
    """float64: does every ray (o, d [n, 3]) enter every box (lo, hi [M, 3])?  (bool [n], the largest exit distance [n]).  The slab
    test with exact quotients on the boxes as they are; a ray has to pass through the box in front of its origin."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ok, leaves_at = np.ones(len(o), bool), np.zeros(len(o))
    with np.errstate(all="ignore"):
        for first in range(0, len(lo), 4096):
            a = (lo[None, first:first + 4096] - o[:, None]) / d[:, None]  # [n, m, 3]
            b = (hi[None, first:first + 4096] - o[:, None]) / d[:, None]
            t_in, t_out = np.minimum(a, b).max(axis=2), np.maximum(a, b).min(axis=2)
            ok &= ((t_in <= t_out) & (t_out > 0)).all(axis=1)
            leaves_at = np.maximum(leaves_at, t_out.max(axis=1))
    return ok, leaves_at


def rays_cross_every_layer_box(lo, hi, o, d):
    """float64, for boxes that all hold one thin slab of z: the rectangle X x Y common to all boxes and the z range Z of them all; a
    ray that starts in front of Z, has d.z != 0 and is inside X x Y where it enters and where it leaves Z (so all the way between)
    passes, for every box, the box's own z range at points inside the box's rectangle: it enters every box.  Sufficient, not
    necessary; one pass over the boxes instead of rays x boxes tests.  bool [n]"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    assert (lo <= hi).all()
    x0, y0, x1, y1 = lo[:, 0].max(), lo[:, 1].max(), hi[:, 0].min(), hi[:, 1].min()
    z0, z1 = lo[:, 2].min(), hi[:, 2].max()
    ok = d[:, 2] != 0
    with np.errstate(all="ignore"):
        for z in (z0, z1):
            t = (z - o[:, 2]) / d[:, 2]
            p = o + t[:, None] * d
            ok &= (t > 0) & (p[:, 0] >= x0) & (p[:, 0] <= x1) & (p[:, 1] >= y0) & (p[:, 1] <= y1)
    return ok


def local_rays(inverse_transform, o, d):
    """the instance-local ray of np_path (column-major mat4), in float64 over the float32 matrix the device holds"""
    m = np.asarray(inverse_transform, np.float64).reshape(-1)
    return npp._mat_point(m, np.asarray(o, np.float64)), npp._mat_dir(m, np.asarray(d, np.float64))


def mesh_children(rec):
    """(child words counted from the mesh's first record, root) of jpt_debug_mesh_records"""
    child = rec["nodes4"].view(np.int32).reshape(-1, 32)[:, 12:16].copy()
    child[child >= 0] -= rec["first_record"]
    return child, rec["root"] - rec["first_record"]


def tlas_children(rec):
    return rec["nodes4"].view(np.int32).reshape(-1, 32)[:, 12:16].copy(), rec["root"]


def mesh_regime(rec, what):
    """(guaranteed, need, the boxes of every child) of one mesh's tree, printed"""
    child, root = mesh_children(rec)
    g, order, _ = guaranteed_depth(child, root)
    need = need4(child, 0, root)
    print("%s: %d records, %d triangles: a walk inside it holds at least %d entries at its first leaf and at most %d" % (
        what, rec["n_records"], rec["n_tris"], g, need))
    return g, need, boxes_of(rec["nodes4"], order)


def tlas_regime(rec, what, counts=None):
    child, root = tlas_children(rec)
    g, order, holds = guaranteed_depth(child, root, counts)
    need = need4(child, 0, root)
    print("%s: %d records of the instance level: at least %d entries at the first %s, at most %d" % (
        what, len(order), g, "instance" if counts is None else "shutter", need))
    return g, need, boxes_of(rec["nodes4"], order, holds)


# ---- the yardstick: Moller-Trumbore over rays x triangles -----------------------------------------------------------------------------

def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def moller_trumbore(lo, ld, v0, v1, v2):
    """np_denoise._tri_tests' body (main.glsl:224-257) on component tuples of float32 arrays that broadcast against each other: the
    same binary32 operations in the same order.  (accepted, t, u, v, front, plane) -- plane: the ray meets the triangle's plane in
    front of its origin, whatever u and v say (the layer is in the ray's way)"""
    e1, e2 = _sub(v1, v0), _sub(v2, v0)
    pvec = _cross(ld, e2)
    det = _dot(e1, pvec)
    inv_det = F(1.0) / det
    tvec = _sub(lo, v0)
    u = _dot(tvec, pvec) * inv_det
    qvec = _cross(tvec, e1)
    v = _dot(ld, qvec) * inv_det
    t = _dot(e2, qvec) * inv_det
    plane = ~(np.abs(det) < F(1e-5)) & ~((t < 0) | (t > F(1e9)))
    ok = plane & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1))
    front = _dot(_cross(e1, e2), ld) > 0
    return ok, t, u, v, front, plane


def instance_triangles(view):
    """np_denoise._instance_triangles with one walk per BLAS: [the instance's triangle indices, int64]"""
    per_blas = {}
    for inst in view.instances:
        b = int(inst["blas_index"])
        if b not in per_blas:
            per_blas[b] = np.asarray(npp._leaf_triangles(view.bvh_nodes, b), np.int64)
    return [per_blas[int(inst["blas_index"])] for inst in view.instances]


def tri_tests(view, o, d, instances=None, chunk=1024):
    """np_denoise._tri_tests with the triangle loop vectorised over [rays, triangles] blocks of at most `chunk` triangles.  Yields
    (instance, triangle indices [m]) + moller_trumbore's tuple of [n, m] arrays; instances: only those"""
    geom = view.tri_geom["vertices"][..., :3].astype(F)
    o, d = np.asarray(o, F), np.asarray(d, F)
    for i, tris in enumerate(instance_triangles(view)):
        if instances is not None and i not in instances:
            continue
        inv = view.instances[i]["inverse_transform"].astype(F)
        lo, ld = npp._mat_point(inv, o), npp._mat_dir(inv, d)
        lo, ld = tuple(lo[:, k, None] for k in range(3)), tuple(ld[:, k, None] for k in range(3))
        for first in range(0, len(tris), chunk):
            ti = tris[first:first + chunk]
            v0, v1, v2 = (tuple(geom[ti, c, k][None, :] for k in range(3)) for c in range(3))
            yield (i, ti) + moller_trumbore(lo, ld, v0, v1, v2)


def brute_force(view, o, d, instances=None):
    """(the smallest accepted t per ray, 1e9: none; the smallest t at which the ray meets ANY triangle's plane)"""
    best, first = np.full(len(o), nq.MISS_T, F), np.full(len(o), nq.MISS_T, F)
    with np.errstate(all="ignore"):
        for _, _, ok, t, _, _, _, plane in tri_tests(view, o, d, instances):
            assert not (ok & np.isnan(t)).any(), "an accepted test with a NaN t"
            best = np.minimum(best, np.where(ok, t, nq.MISS_T).min(axis=1))
            first = np.minimum(first, np.where(plane, t, nq.MISS_T).min(axis=1))
    return best, first


def closest_mismatches(view, o, d, tmax, hits, best):
    """per ray: is the jpt_ray_hit NOT what the pin asks for?  A ray whose brute-force minimum is not under its tmax: the miss
    encoding, every byte.  Otherwise t is the minimum bit for bit, the (instance, triangle) named is a triangle of that instance
    whose own test is accepted with that t, u and v are that test's, and the flags say valid and which side."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    n = len(o)
    hits = np.ascontiguousarray(hits)
    want_hit = best < nq.effective_tmax(tmax, n)
    got = hits.view(np.uint8).reshape(n, 64)
    is_miss = (got == nq.miss_record(1).view(np.uint8)).all(axis=1)
    tris = instance_triangles(view)
    inst = hits["instance"].astype(np.int64)
    tri = hits["triangle"].astype(np.int64)
    named = (inst >= 0) & (inst < len(tris)) & (tri < len(view.tri_geom))
    named &= np.array([named[k] and bool((tris[inst[k]] == tri[k]).any()) for k in range(n)])
    i, ti = np.where(named, inst, 0), np.where(named, tri, 0)
    geom = view.tri_geom["vertices"][..., :3].astype(F)
    inv = view.instances["inverse_transform"].astype(F).reshape(len(view.instances), 16)[i].T      # [16, n]: np_path's m[k]
    with np.errstate(all="ignore"):
        lo, ld = npp._mat_point(inv, o), npp._mat_dir(inv, d)
        v0, v1, v2 = (tuple(geom[ti, c, k] for k in range(3)) for c in range(3))
        ok, t, u, v, front, _ = moller_trumbore(tuple(lo[:, k] for k in range(3)), tuple(ld[:, k] for k in range(3)), v0, v1, v2)
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    same = named & ok & (bits(t) == bits(best)) & (bits(hits["t"]) == bits(best)) & (bits(hits["u"]) == bits(u)) & (bits(hits["v"]) == bits(v))
    same &= hits["flags"] == nq.VALID + np.where(front, nq.FRONT, 0)
    return ~np.where(want_hit, same, is_miss)


def test_the_vectorised_yardstick_equals_np_querys_on_cornell(oracle):
    ref = oracle.build_scene(scenes.cornell_scene())
    o, d = nq.random_rays(500, seed=31)
    best, first = brute_force(ref, o, d)
    assert np.array_equal(best.view(np.uint32), nq.brute_force_t(ref, o, d).view(np.uint32))
    assert 100 < int((best < nq.MISS_T).sum()) < 500 and (first <= best).all()


# ---- 1. queries, both modes, against brute force ----------------------------------------------------------------------------------------

N_RAYS = 256   # four waves


def stack_rays(seed=77):
    """256 rays through the stack, all crossing every layer's box: half along +z or -z through the rectangle, half up to 30 degrees
    oblique (directions of lengths 0.5 .. 2: t counts in units of them).  (origins, dirs, carries a tmax)"""
    rng = np.random.default_rng(seed)
    z_mid = 0.5 * STACK_STEP * (N_STACK - 1)
    mid = np.stack([rng.uniform(-3.0, 3.0, N_RAYS), rng.uniform(-2.0, 4.0, N_RAYS), np.full(N_RAYS, z_mid)], axis=1)
    axial = np.arange(N_RAYS) % 2 == 0
    mid[axial, 0], mid[axial, 1] = rng.uniform(-5.8, 5.8, int(axial.sum())), rng.uniform(-4.8, 6.8, int(axial.sum()))
    tilt = np.where(axial, 0.0, np.tan(np.deg2rad(rng.uniform(0.0, 30.0, N_RAYS))))
    phi = rng.uniform(0.0, 2.0 * np.pi, N_RAYS)
    sign = np.where(rng.random(N_RAYS) < 0.5, -1.0, 1.0)
    d = np.stack([tilt * np.cos(phi), tilt * np.sin(phi), sign], axis=1)
    o = mid - d * (z_mid + 1.0)               # one unit of z in front of the stack's first layer in ray order
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (N_RAYS, 1))
    return o.astype(F), d.astype(F), np.arange(N_RAYS) % 4 == 1


_stack_case = {}


def stack_case(view):
    """(origins, dirs, tmax, bounded, best, first) for the stack, made once from the first view handed in (every tree holds the same
    triangles and transforms: the caller asserts it) and left unchanged.  A ray with a tmax alternately gets its own brute-force
    minimum (exclusive: a miss, though its line crosses every box) and the minimum plus the depth of a few layers (a hit)."""
    if not _stack_case:
        o, d, bounded = stack_rays()
        best, first = brute_force(view, o, d)
        assert (best < nq.MISS_T).all()
        few_layers = F(4 * 0.2 / N_LAYERS) / np.abs(d[:, 2])
        k = np.cumsum(bounded)
        tmax = np.where(bounded, np.where(k % 2 == 0, best, best + few_layers), F(0.0)).astype(F)
        for a in (o, d, tmax, bounded, best, first):
            a.setflags(write=False)
        _stack_case.update(o=o, d=d, tmax=tmax, bounded=bounded, best=best, first=first)
    c = _stack_case
    return c["o"], c["d"], c["tmax"], c["bounded"], c["best"], c["first"]


def stack_ctx(oracle, tree):
    """(context, the scene as it hands it out) -- read before a rebuild: the host's copy counts as stale after it"""
    sc = scene_of("shutter_stack")
    ctx = host.Context(0)
    try:
        if tree == "native_upload":
            ref = oracle.build_scene(sc)
            ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures)
        else:
            ctx.build_scene(sc, SAH if tree == "sah" else WATERTIGHT)
        view = nq.scene_view(ctx)
        if tree == "rebuilt":
            ctx.rebuild_mesh(0, sc.meshes[0])
            ctx.rebuild_tlas(all_transforms(sc))
    except Exception:
        ctx.close()
        raise
    return ctx, view


_watertight_records = {}


def watertight_mesh_records(name, mesh, **kw):
    """the mesh records of the JPT_BUILD_SAH_WATERTIGHT commit of a scene: the native tree a JPT_BUILD_SAH commit walks too"""
    key = (name, mesh) + tuple(sorted(kw.items()))
    if key not in _watertight_records:
        ctx = host.Context(0)
        try:
            ctx.build_scene(scene_of(name, **kw), WATERTIGHT)
            _watertight_records[key] = ctx.debug_mesh_records(mesh)
        finally:
            ctx.close()
    return _watertight_records[key]


def stack_regime(ctx, tree, view, o, d):
    """(guaranteed, need, which of the rays o, d are shown to enter every box) of the tree `ctx` walks; None for a native upload"""
    if tree == "native_upload":
        return None
    sc = scene_of("shutter_stack")
    tg, tneed, tboxes = tlas_regime(ctx.debug_tlas_records(len(sc.instances)), "the stack, %s" % tree)
    entered, _ = rays_enter_every_box(*tboxes, o, d)
    rec = watertight_mesh_records("shutter_stack", 0) if tree == "sah" else ctx.debug_mesh_records(0)
    mg, mneed, mboxes = mesh_regime(rec, "the stack, %s, the shutter of %d layers" % (tree, N_LAYERS))
    for i in range(len(sc.instances)):
        entered &= rays_cross_every_layer_box(*mboxes, *local_rays(view.instances[i]["inverse_transform"], o, d))
    print("the stack of %d, %s: guaranteed %d + 1 + %d = %d, need %d + 1 + %d = %d; %d of %d unbounded rays enter every box of every record" % (
        N_STACK, tree, tg, mg, tg + 1 + mg, tneed, mneed, tneed + 1 + mneed, int(entered.sum()), len(o)))
    return tg + 1 + mg, tneed + 1 + mneed, entered


@pytest.mark.parametrize("tree", ["sah", "watertight", "rebuilt", "native_upload"])
def test_queries_on_stacked_shutters_equal_brute_force_for_every_ray(oracle, hiplib, tree):
    """jpt_query_rays, closest and any-hit (query_kernel: all 96 rows in LDS, no spill pointer), 256 rays.  Zero mismatches."""
    ctx, view = stack_ctx(oracle, tree)
    try:
        o, d, tmax, bounded, best, first = stack_case(view)
        mine, _ = brute_force(view, o[:8], d[:8])     # this tree holds the triangles and transforms the case was made from
        assert np.array_equal(mine.view(np.uint32), best[:8].view(np.uint32))
        regime = stack_regime(ctx, tree, view, o[~bounded], d[~bounded])
        hits, occ = ctx.query_rays(o, d, tmax)
        any_occ = ctx.query_rays(o, d, tmax, mode=capi.QUERY_ANY)
        free, _ = ctx.query_rays(o, d)
    finally:
        ctx.close()
    if regime is not None:
        guaranteed, need, entered = regime
        assert guaranteed >= GUARANTEED and need <= CAPACITY and entered.all()
    want_hit = best < nq.effective_tmax(tmax, N_RAYS)
    later = best > first                      # the closest hit is not the first layer in the ray's way
    bad = closest_mismatches(view, o, d, tmax, hits, best)
    bad_free = closest_mismatches(view, o, d, None, free, best)
    print("the stack, %s: %d rays, %d with a tmax, %d misses, %d closest hits behind the first layer; mismatches: %d closest, %d unbounded, %d any-hit" % (
        tree, N_RAYS, int(bounded.sum()), int((~want_hit).sum()), int((later & want_hit).sum()), int(bad.sum()), int(bad_free.sum()),
        int((any_occ != want_hit).sum())))
    assert int((later & want_hit).sum()) >= 32 and int((~want_hit).sum()) >= 32 and int(bounded.sum()) == N_RAYS // 4
    assert not bad.any(), "rays whose hit is not the pin's: %s" % np.nonzero(bad)[0][:8].tolist()
    assert not bad_free.any(), "unbounded rays whose hit is not the pin's: %s" % np.nonzero(bad_free)[0][:8].tolist()
    assert np.array_equal(occ, want_hit.astype(np.uint8))
    assert any_occ.dtype == np.uint8 and np.array_equal(any_occ, want_hit.astype(np.uint8))


# ---- deep_cornell's regime ---------------------------------------------------------------------------------------------------------------

def cornell_bound_rays(n=96, seed=9):
    """rays of the two kinds the renders trace through the stack: from the camera to points of the shutter's middle, and from the
    strip of floor in front of the stack to points of the light"""
    rng = np.random.default_rng(seed)
    cam = np.asarray(scenes.cornell_scene().camera.transform, np.float64)[9:12]
    to = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-2.2, -0.3, n), np.full(n, SHUTTER_AT[2])], axis=1)
    floor = np.stack([rng.uniform(-1.0, 1.0, n), np.full(n, -2.999), rng.uniform(2.92, 2.98, n)], axis=1)
    light = np.stack([rng.uniform(-0.9, 0.9, n), np.full(n, 2.9), rng.uniform(-0.9, 0.9, n)], axis=1)
    o = np.concatenate([np.broadcast_to(cam, (n, 3)), floor])
    return o.astype(F), (np.concatenate([to, light]) - o).astype(F)


def deep_cornell_regime(ctx, view, rec, what, **kw):
    """(guaranteed, need) of deep_cornell as `ctx` walks it, rec: the shutter's mesh records.  Asserts for cornell_bound_rays, in
    float64, that they enter every box of the instance level that holds a shutter and every box of every shutter's tree, and (the
    yardstick's float32 test over Cornell's own triangles) that they hit nothing before they have left the last of those boxes."""
    sc = scene_of("deep_cornell", **kw)
    o, d = cornell_bound_rays()
    tl = ctx.debug_tlas_records(len(sc.instances))
    tg, tneed, tboxes = tlas_regime(tl, what, counts=lambda leaf: ~leaf >= FIRST_SHUTTER)
    entered, _ = rays_enter_every_box(*tboxes, o, d)
    in_stack, leaves_at = rays_enter_every_box(tl["lo"][FIRST_SHUTTER:].astype(np.float64), tl["hi"][FIRST_SHUTTER:].astype(np.float64), o, d)
    entered &= in_stack
    mg, mneed, mboxes = mesh_regime(rec, "%s, the shutter of %d layers" % (what, rec["n_tris"]))
    for i in range(FIRST_SHUTTER, len(sc.instances)):
        entered &= rays_cross_every_layer_box(*mboxes, *local_rays(view.instances[i]["inverse_transform"], o, d))
    others, _ = brute_force(view, o, d, instances=range(FIRST_SHUTTER))
    print("%s: guaranteed %d + 1 + %d = %d, need %d + 1 + %d = %d; %d of %d rays enter every box that holds a shutter, %d hit Cornell in front of one" % (
        what, tg, mg, tg + 1 + mg, tneed, mneed, tneed + 1 + mneed, int(entered.sum()), len(o), int((others <= leaves_at).sum())))
    assert entered.all() and (others > leaves_at).all()
    return tg + 1 + mg, tneed + 1 + mneed


@pytest.mark.parametrize("duplicated", [0, 64])
def test_deep_cornell_holds_more_entries_than_either_lds_part(hiplib, duplicated):
    """the trees of tests 2 .. 6: the commit's (JPT_BUILD_SAH and JPT_BUILD_SAH_WATERTIGHT walk the same native tree) and the one
    after jpt_scene_rebuild_mesh of the shutter"""
    kw = dict(duplicated=duplicated) if duplicated else {}
    sc = scene_of("deep_cornell", **kw)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, WATERTIGHT)
        view = nq.scene_view(ctx)
        g, need = deep_cornell_regime(ctx, view, ctx.debug_mesh_records(SHUTTER_MESH), "deep_cornell, %d duplicated, the commit" % duplicated, **kw)
        assert g >= GUARANTEED and need <= CAPACITY
        ctx.rebuild_mesh(SHUTTER_MESH, sc.meshes[SHUTTER_MESH])
        g, need = deep_cornell_regime(ctx, view, ctx.debug_mesh_records(SHUTTER_MESH), "deep_cornell, %d duplicated, the shutter rebuilt" % duplicated, **kw)
        assert g >= GUARANTEED and need <= CAPACITY
    finally:
        ctx.close()


# ---- 2. the guide pass against the pixel queries ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [SAH, WATERTIGHT])
def test_guides_of_deep_cornell_equal_the_pixel_queries(hiplib, builder):
    """the guide kernel and query_kernel, each with its own 96-row stack array in LDS, against each other (test 1 pins the queries):
    record for record as in test_gpu_query.py"""
    w, h = 48, 32
    sc = scene_of("deep_cornell")
    ys, xs = np.mgrid[0:h, 0:w]
    centres = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=1).astype(F)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, builder)
        ctx.set_params(w, h, 3, capi.ACCUM_HDR_F32)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.render(1, 1)
        ctx.denoise()
        position_t, normal, _ = ctx.read_guides()
        hits = ctx.query_pixels(centres)
    finally:
        ctx.close()
    pt, nr = position_t.reshape(-1, 4), normal.reshape(-1, 4)
    valid = (hits["flags"] & capi.HIT_VALID) != 0
    on_shutter = valid & (hits["instance"] >= FIRST_SHUTTER)
    print("deep_cornell, builder %d: %d of %d pixels hit, %d of them a shutter" % (builder, int(valid.sum()), len(valid), int(on_shutter.sum())))
    assert np.array_equal(valid, pt[:, 3] >= 0)
    assert np.array_equal(hits["position"][valid].view(np.uint32), pt[valid, :3].view(np.uint32))
    assert np.array_equal(hits["normal"][valid].view(np.uint32), nr[valid, :3].view(np.uint32))
    assert nq.miss_record(1).tobytes() * int((~valid).sum()) == hits[~valid].tobytes()
    assert int(on_shutter.sum()) >= 32 and int((valid & ~on_shutter).sum()) >= 32


# ---- 3. shadow rays -----------------------------------------------------------------------------------------------------------------------

LIGHTINGS = {"emitters": (True, False), "map": (False, True), "both": (True, True)}


def cornell_ctx(sc, builder, w, h, accum, lighting=None, kernel=WF, bounces=3, extensions=0):
    """lighting: a key of LIGHTINGS (None: BRDF sampling under the gradient sky)"""
    emitters, env = LIGHTINGS[lighting] if lighting else (False, False)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, builder)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_kernel(kernel)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        if extensions:
            ctx.set_material_extensions(extensions)
        if env:
            ctx.set_environment(sun_map())
            ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        if emitters:
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
    except Exception:
        ctx.close()
        raise
    return ctx


def rendered(ctx, frames, kernel=None):
    if kernel is not None:
        ctx.set_kernel(kernel)
    ctx.accum_reset()
    ctx.render(frames, 1)
    return images(ctx)


def differ(a, b):
    return not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("lighting", sorted(LIGHTINGS))
def test_shadow_rays_through_deep_cornell(hiplib, lighting):
    """wf2_occlude / wf2_occlude_lt (all 96 rows in LDS): 24 x 24, 2 frames, 3 bounces, HDR.  The wavefront kernel against the audit
    kernel's own walk over the two-child tree on JPT_BUILD_SAH; the watertight commit against the same context after
    jpt_scene_rebuild_mesh of the shutter, another deep topology over the same triangles.  Live: the image differs from the one
    without the shutters and from the BRDF-sampling one."""
    w = h = 24
    frames = 2
    sc = scene_of("deep_cornell")
    ctx = cornell_ctx(sc, SAH, w, h, capi.ACCUM_HDR_F32, lighting)
    try:
        wavefront = rendered(ctx, frames)
        audit = rendered(ctx, frames, AUDIT)
    finally:
        ctx.close()
    assert_same(wavefront, audit, "%s, JPT_BUILD_SAH: the wavefront kernel against the audit kernel" % lighting)
    ctx = cornell_ctx(sc, WATERTIGHT, w, h, capi.ACCUM_HDR_F32, lighting)
    try:
        commit = rendered(ctx, frames)
        ctx.rebuild_mesh(SHUTTER_MESH, sc.meshes[SHUTTER_MESH])
        rebuilt = rendered(ctx, frames)
    finally:
        ctx.close()
    assert_same(rebuilt, commit, "%s, JPT_BUILD_SAH_WATERTIGHT: after jpt_scene_rebuild_mesh against the commit" % lighting)
    for what, other_scene, other_lighting in (("without the shutters", scene_of("deep_cornell", shutter=False), lighting), ("BRDF sampling", sc, None)):
        ctx = cornell_ctx(other_scene, SAH, w, h, capi.ACCUM_HDR_F32, other_lighting)
        try:
            other = rendered(ctx, frames)
        finally:
            ctx.close()
        n = int((other[0] != wavefront[0]).any(axis=-1).sum())
        print("%s: %d of %d pixels differ from the render %s" % (lighting, n, w * h, what))
        assert differ(other, wavefront), "%s: the render %s is the same image" % (lighting, what)


# ---- 4. the primary-ray families ----------------------------------------------------------------------------------------------------------

ATLAS_SCALE, ATLAS_AT, ATLAS_STEP = 0.5, (0.0, -2.0, 0.0), 0.0005
LYING = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])    # a quarter turn about x: the layers lie flat


def family_stage(family, shutter=True):
    """test_gpu_family_scene_changes.stage without its tube, with a stack of shutters: (scene, the shutter's mesh, its first instance).
    Cornell's box (lens, ortho, equirect, cube): deep_cornell's stack; the panorama is taken from just in front of it, the first
    cube stands just behind it.  The bakes' atlas scene (bake, probe): the stack lies flat, 6 x 6, from 0.2 to 0.38 above the baked
    floor and under the hanging box, so the floor texels' rays cross it upwards and the upper probe's downwards."""
    sc = fam.stage(family, tube=False).scene
    sc.meshes.append(shutter_mesh(N_LAYERS))
    mesh, first = len(sc.meshes) - 1, len(sc.instances)
    if family in fam.ON_THE_ATLAS:
        basis, (x, y, z), step = LYING * ATLAS_SCALE, ATLAS_AT, (0.0, ATLAS_STEP, 0.0)
    else:
        basis, (x, y, z), step = np.eye(3) * SHUTTER_SCALE, SHUTTER_AT, (0.0, 0.0, SHUTTER_STEP)
        if family == "equirect":
            sc.camera = scenes.CameraDesc(scenes.transform12(scenes.rot_y(25.0), (0.2, -0.3, 2.95)))
    if shutter:
        sc.instances += [scenes.Instance(mesh, scenes.transform12(basis, (x + step[0] * k, y + step[1] * k, z + step[2] * k)), [3]) for k in range(N_STACK)]
    return sc, mesh, first


def family_bound_rays(family, sc, n=96, seed=4):
    """candidate rays of the kind the family's primaries are, through the stack: from where they start to points of the stack's middle"""
    rng = np.random.default_rng(seed)
    if family in fam.ON_THE_ATLAS:
        to = np.stack([rng.uniform(-1.5, 1.5, n), np.full(n, ATLAS_AT[1]), rng.uniform(-1.5, 1.5, n)], axis=1)
        if family == "bake":      # from the floor's texels upwards, up to some 25 degrees off the normal
            o = to + np.stack([rng.uniform(-0.08, 0.08, n), np.full(n, -0.199), rng.uniform(-0.08, 0.08, n)], axis=1)
        else:
            o = np.broadcast_to(fam.PROBES[0].astype(np.float64), (n, 3))
        return o.astype(F), (to - o).astype(F)
    to = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-2.2, -0.5, n), np.full(n, SHUTTER_AT[2])], axis=1)
    if family == "ortho":         # parallel rays down -z
        o = to + np.array([0.0, 0.0, 7.0])
    elif family == "cube":
        o = np.broadcast_to(fam.CUBES[0].astype(np.float64), (n, 3))
        to[:, 2] = SHUTTER_AT[2] + SHUTTER_STEP * N_STACK
    else:
        o = np.broadcast_to(np.asarray(sc.camera.transform, np.float64)[9:12], (n, 3))
    return o.astype(F), (to - o).astype(F)


def stack_in_a_scene_regime(ctx, view, sc, mesh, first, o, d, what):
    """(guaranteed, need, how many of the rays o, d it is shown for) of a scene whose instances from `first` on are one stack of
    shutters, as `ctx` walks it: deep_cornell_regime's reasoning, the rays that do not pass its checks left out"""
    tl = ctx.debug_tlas_records(len(sc.instances))
    tg, tneed, tboxes = tlas_regime(tl, what, counts=lambda leaf: ~leaf >= first)
    entered, _ = rays_enter_every_box(*tboxes, o, d)
    in_stack, leaves_at = rays_enter_every_box(tl["lo"][first:].astype(np.float64), tl["hi"][first:].astype(np.float64), o, d)
    rec = ctx.debug_mesh_records(mesh)
    mg, mneed, mboxes = mesh_regime(rec, "%s, the shutter of %d layers" % (what, rec["n_tris"]))
    entered &= in_stack
    for i in range(first, len(sc.instances)):
        entered &= rays_cross_every_layer_box(*mboxes, *local_rays(view.instances[i]["inverse_transform"], o, d))
    others, _ = brute_force(view, o, d, instances=range(first))
    shown = entered & (others > leaves_at)
    print("%s: guaranteed %d + 1 + %d = %d, need %d + 1 + %d = %d, shown for %d of %d rays" % (
        what, tg, mg, tg + 1 + mg, tneed, mneed, tneed + 1 + mneed, int(shown.sum()), len(o)))
    return tg + 1 + mg, tneed + 1 + mneed, int(shown.sum())


@pytest.mark.parametrize("family", fam.FAMILIES)
def test_primary_families_through_a_stack_of_shutters(hiplib, family):
    """every wf2_primary* variant is a kernel of its own with its own scratch layout: each walks the stack, at the sizes of
    test_gpu_family_scene_changes.py, under the gradient sky.  The two yardsticks of test 3; the accumulation differs from the one
    without the stack."""
    sc, mesh, first = family_stage(family)
    ctx = fam.ctx_for(sc, family, "sky", SAH)
    try:
        wavefront = fam.state(ctx, family)
        audit = fam.state(ctx, family, AUDIT)
    finally:
        ctx.close()
    fam.assert_state({name: wavefront[name] for name in audit}, audit, "%s, JPT_BUILD_SAH: the wavefront kernel against the audit kernel" % family)
    o, d = family_bound_rays(family, sc)
    ctx = fam.ctx_for(sc, family, "sky", WATERTIGHT)
    try:
        view = nq.scene_view(ctx)
        regimes = [stack_in_a_scene_regime(ctx, view, sc, mesh, first, o, d, "%s, the commit" % family)]
        commit = fam.state(ctx, family)
        ctx.rebuild_mesh(mesh, sc.meshes[mesh])
        regimes.append(stack_in_a_scene_regime(ctx, view, sc, mesh, first, o, d, "%s, the shutter rebuilt" % family))
        rebuilt = fam.state(ctx, family)
    finally:
        ctx.close()
    fam.assert_state(rebuilt, commit, "%s, JPT_BUILD_SAH_WATERTIGHT: after jpt_scene_rebuild_mesh against the commit" % family)
    for guaranteed, need, shown in regimes:
        assert guaranteed >= GUARANTEED and need <= CAPACITY and shown >= 32
    bare, _, _ = family_stage(family, shutter=False)
    ctx = fam.ctx_for(bare, family, "sky", SAH)
    try:
        without = fam.state(ctx, family)
    finally:
        ctx.close()
    n = fam.differing(without["accumulation"], wavefront["accumulation"])
    print("%s: %d values of the accumulation differ from the render without the stack" % (family, n))
    assert n > 0


def test_primary_families_pinhole_with_glass_shutters(hiplib):
    """the *_tx kernels: deep_cornell with its shutters of glass under JPT_MATERIAL_EXT_TRANSMISSION, the pinhole camera, 48 x 32; the
    two yardsticks of test 3, and the image differs from the one with the extension off"""
    w, h, frames = 48, 32, 2
    base = scene_of("deep_cornell")
    sc = scenes.with_transmissive_materials(base, [len(base.materials) - 1], transmission=0.8, ior=1.5)
    glass = len(sc.materials) - 1
    assert not any(glass in i.material_ids for i in sc.instances)
    for i in sc.instances[FIRST_SHUTTER:]:
        i.material_ids = [glass]
    tx = capi.MATERIAL_EXT_TRANSMISSION
    ctx = cornell_ctx(sc, SAH, w, h, capi.ACCUM_HDR_F32, extensions=tx)
    try:
        wavefront = rendered(ctx, frames)
        audit = rendered(ctx, frames, AUDIT)
    finally:
        ctx.close()
    assert_same(wavefront, audit, "glass shutters, JPT_BUILD_SAH: the wavefront kernel against the audit kernel")
    ctx = cornell_ctx(sc, WATERTIGHT, w, h, capi.ACCUM_HDR_F32, extensions=tx)
    try:
        commit = rendered(ctx, frames)
        ctx.rebuild_mesh(SHUTTER_MESH, sc.meshes[SHUTTER_MESH])
        rebuilt = rendered(ctx, frames)
    finally:
        ctx.close()
    assert_same(rebuilt, commit, "glass shutters, JPT_BUILD_SAH_WATERTIGHT: after jpt_scene_rebuild_mesh against the commit")
    ctx = cornell_ctx(sc, SAH, w, h, capi.ACCUM_HDR_F32)
    try:
        opaque = rendered(ctx, frames)
    finally:
        ctx.close()
    assert differ(opaque, wavefront), "the extension changed nothing"


# ---- 5. the set-aside / tie route ---------------------------------------------------------------------------------------------------------

_wanted = {}


def tie_case(oracle, mode, w=32, h=24, frames=2, bounces=3):
    """deep_cornell with 64 layers of the shutter duplicated exactly, and the oracle's render of it, made once per mode"""
    sc = scene_of("deep_cornell", duplicated=64)
    if mode not in _wanted:
        cam = scenes.camera_block(sc.camera, w, h)
        want, want_ldr, _, _, _ = oracle.render(oracle.build_scene(sc), cam, w, h, bounces, frames, 1, mode)
        _wanted[mode] = (want, want_ldr)
    return (sc, w, h, frames, bounces) + _wanted[mode]


@pytest.mark.parametrize("mode", MODES)
def test_set_aside_route_through_deep_cornell_equals_the_oracle(oracle, hiplib, mode):
    """wf2_finish walks the deep tree from its all-scratch stack: exact ties (duplicated layers) are set aside and re-decided on the
    reference's own trees.  JPT_BUILD_SAH; one blocking render and three queued ones, each against the oracle pixel for pixel, as
    test_gpu_round_masks.check does."""
    sc, w, h, frames, bounces, want, want_ldr = tie_case(oracle, mode)
    ctx = cornell_ctx(sc, SAH, w, h, mode, bounces=bounces)
    try:
        ctx.render(frames, 1, counted=True)
        got, got_ldr, st = ctx.read_accum(), ctx.read_ldr(), ctx.stats()
        for _ in range(3):
            ctx.accum_reset()
            ctx.render(frames, 1, asynchronous=True)
        ctx.sync()
        queued, queued_ldr = ctx.read_accum(), ctx.read_ldr()
    finally:
        ctx.close()
    for how, a, l in (("blocking", got, got_ldr), ("queued", queued, queued_ldr)):
        print("deep_cornell with ties", (w, h, frames, bounces), mode, how, "differing pixels: accumulation", int((a != want).any(axis=-1).sum()),
              "rgba8", int((l != want_ldr).any(axis=-1).sum()), "set aside", st["set_aside"], "dropped", st["set_aside_dropped"])
    assert st["set_aside"] >= 1 and st["set_aside_dropped"] == 0
    assert np.array_equal(got, want) and np.array_equal(got_ldr, want_ldr)
    assert np.array_equal(queued, want) and np.array_equal(queued_ldr, want_ldr)


# ---- 6. the cooperative tail --------------------------------------------------------------------------------------------------------------

def test_the_cooperative_tail_walks_as_deep(hiplib):
    """JPT_TAIL=1 with eager thresholds (coop_walk: 18 rows in LDS, two lent to the pool, and its peek): the switches are read once
    per process, so ONE child process runs this file's render tests (3 to 5) under them, as test_gpu_full.py does for the parity
    suite.  Same assertions, bit for bit."""
    env = dict(os.environ, JPT_TAIL="1", JPT_TAIL_ROUNDS="2", JPT_TAIL_LANES="8")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                        "shadow_rays_through or primary_families or set_aside_route"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout
