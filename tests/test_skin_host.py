"""jpt_scene_set_mesh_rig / jpt_scene_pose_mesh / jpt_scene_clear_mesh_rig and jpt_debug_skin (posing a committed mesh on the device from a
bone palette and blend-shape weights): the arithmetic's host form against the numpy restatement (tests/np_skin.py), bit for bit; every
argument and state check, which run on the host before any device work, on host-only contexts; the header, the binding and the
wrappers."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import np_skin
from gdpathtracing_amd import capi, host, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_INVALID, E_DEVICE, E_LIMIT, E_STATE = 0, -1, -2, -3, -4   # JPT_E_* (include/jpt.h)
BLOB, CUBE = 2, 1   # the demo scene's one-surface character mesh and its three-surface cube


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_debug_skin(device, c):
    r = c["rig"]
    return host.debug_skin(device, c["pos"], c["nrm"], host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas), c["K"], c["S"],
                           c["palette"], c["blend"])


def want_of(c):
    r = c["rig"]
    return np_skin.np_skin(c["pos"], c["nrm"], r.bones, r.weights, c["K"], r.position_deltas, r.normal_deltas, c["palette"], c["blend"])


def test_constants_match_the_header(hiplib):
    pub = open(os.path.join(ROOT, "include", "jpt.h")).read()
    codes = {n: int(v) for n, v in re.findall(r"(JPT_E_\w+)\s*=\s*(-?\d+)", pub)}
    assert (codes["JPT_E_INVALID"], codes["JPT_E_DEVICE"], codes["JPT_E_LIMIT"], codes["JPT_E_STATE"]) == (E_INVALID, E_DEVICE, E_LIMIT, E_STATE)


def test_host_form_equals_numpy_bit_for_bit(hiplib):
    cases = np_skin.debug_cases()
    assert len(cases) > 100
    for label, c in cases:
        want_p, want_n = want_of(c)
        assert np.isfinite(want_p).all() and (want_n is None or np.isfinite(want_n).all()), label
        got_p, got_n = run_debug_skin(-1, c)
        assert np.array_equal(bits(got_p), bits(want_p)), label
        assert (got_n is None) == (want_n is None), label
        if want_n is not None:
            assert np.array_equal(bits(got_n), bits(want_n)), label


def test_all_zero_blend_weights_read_no_delta(hiplib):
    """the deltas may then hold anything a float can (here: huge values a multiply by zero would still keep finite, so the proof is the
    equality with the rig that has no shapes; the C side also never forms an address into them: the active list is empty)"""
    rng = np.random.RandomState(5)
    nv = 65
    pos, nrm = rng.uniform(-1, 1, (nv, 3)).astype(np.float32), np.tile(np.float32([0, 1, 0]), (nv, 1))
    rig = np_skin.random_rig(rng, nv, 4, 2, 7)
    rig.position_deltas[:] = 3e38
    pal = np_skin.random_palette(rng, 7)
    got = host.debug_skin(-1, pos, nrm, host.SurfaceRig(rig.bones, rig.weights, rig.position_deltas, rig.normal_deltas), 4, 2, pal, [0.0, -0.0])
    want = np_skin.np_skin(pos, nrm, rig.bones, rig.weights, 4, None, None, pal, None)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _committed(builder):
    ctx = host.Context(-1)
    sc = scenes.demo_scene(n_tris=512)
    ctx.build_scene(sc, builder)
    return ctx, sc


def _rigs_for(mesh, K=4, S=2, n_bones=6, normal_deltas=True, seed=3):
    rng = np.random.RandomState(seed)
    return [np_skin.random_rig(rng, len(s.vertices), K, S, n_bones, normal_deltas=normal_deltas) for s in mesh.surfaces]


def _set_rc(ctx, mesh_id, mesh, rigs, K, S, with_normals=True, n_surfaces=None, edit=None):
    arr = host._update_surfaces(mesh, with_normals)
    keep = [host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas) for r in rigs]
    rarr = host._rig_surfaces(keep)
    if edit:
        edit(arr, rarr)
    rc = ctx._lib.jpt_scene_set_mesh_rig(ctx.h, mesh_id, arr, rarr, len(mesh.surfaces) if n_surfaces is None else n_surfaces, K, S)
    msg = ctx._lib.jpt_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


@pytest.mark.parametrize("builder,why", [(capi.BUILD_REFERENCE_EXACT, "JPT_BUILD_REFERENCE_EXACT"), (capi.BUILD_SAH, "reach records")])
def test_other_builders_are_refused_with_update_meshs_reasons(hiplib, builder, why):
    ctx, sc = _committed(builder)
    rc, msg = _set_rc(ctx, BLOB, sc.meshes[BLOB], _rigs_for(sc.meshes[BLOB]), 4, 2)
    assert rc == E_STATE and why in msg and "JPT_BUILD_SAH_WATERTIGHT" in msg
    arr = host._update_surfaces(sc.meshes[BLOB])
    assert ctx._lib.jpt_scene_update_mesh(ctx.h, BLOB, arr, 1) == E_STATE
    assert ctx._lib.jpt_last_error(ctx.h).decode() == msg   # the same message
    # no rig can exist here: a pose is a state error too
    assert ctx._lib.jpt_scene_pose_mesh(ctx.h, BLOB, None, 0, None, 0) == E_STATE
    ctx.close()


def test_uncommitted_contexts_are_refused(hiplib):
    ctx = host.Context(-1)
    sc = scenes.demo_scene(n_tris=512)
    rc, msg = _set_rc(ctx, 0, sc.meshes[0], _rigs_for(sc.meshes[0]), 4, 2)
    assert rc == E_STATE and "jpt_scene_set_mesh_rig needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT" in msg
    assert ctx._lib.jpt_scene_pose_mesh(ctx.h, 0, None, 0, None, 0) == E_STATE
    assert ctx._lib.jpt_last_error(ctx.h) == b"jpt_scene_pose_mesh needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT"
    assert ctx._lib.jpt_scene_clear_mesh_rig(ctx.h, 0) == OK
    # while a scene is being described
    ctx2, sc2 = _committed(capi.BUILD_SAH_WATERTIGHT)
    assert ctx2._lib.jpt_scene_begin(ctx2.h) == OK
    rc, msg = _set_rc(ctx2, BLOB, sc2.meshes[BLOB], _rigs_for(sc2.meshes[BLOB]), 4, 2)
    assert rc == E_STATE
    assert ctx2._lib.jpt_scene_pose_mesh(ctx2.h, BLOB, None, 0, None, 0) == E_STATE
    assert b"needs a scene made by jpt_scene_commit" in ctx2._lib.jpt_last_error(ctx2.h)
    ctx.close()
    ctx2.close()


def test_pose_has_update_meshs_state_gate_of_its_own(hiplib):
    """a pose refuses on the scene's state before it looks for a rig: with a watertight commit the answer is 'no rig', after an upload that
    was refused (the scene is gone) or on another builder's scene it is the state rule's, whatever happened to the rigs"""
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    L = ctx._lib
    assert L.jpt_scene_pose_mesh(ctx.h, BLOB, None, 0, None, 0) == E_STATE and b"no rig" in L.jpt_last_error(ctx.h)
    assert L.jpt_scene_upload_reference_layout(ctx.h, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0) == E_INVALID
    assert L.jpt_scene_pose_mesh(ctx.h, BLOB, None, 0, None, 0) == E_STATE
    assert b"jpt_scene_pose_mesh needs a scene made by jpt_scene_commit" in L.jpt_last_error(ctx.h)
    arr = host._update_surfaces(sc.meshes[BLOB])
    assert L.jpt_scene_update_mesh(ctx.h, BLOB, arr, 1) == E_STATE
    ctx.close()
    for builder in (capi.BUILD_SAH, capi.BUILD_REFERENCE_EXACT):
        ctx, sc = _committed(builder)
        assert ctx._lib.jpt_scene_pose_mesh(ctx.h, BLOB, None, 0, None, 0) == E_STATE
        assert b"needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT" in ctx._lib.jpt_last_error(ctx.h)
        ctx.close()


def test_mesh_and_topology_refusals_are_update_meshs(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    blob, cube = sc.meshes[BLOB], sc.meshes[CUBE]
    rc, msg = _set_rc(ctx, len(sc.meshes), blob, _rigs_for(blob), 4, 2)
    assert rc == E_INVALID and "no such mesh" in msg
    m = copy.deepcopy(blob)
    m.surfaces[0].indices = m.surfaces[0].indices.copy()
    m.surfaces[0].indices[[0, 1]] = m.surfaces[0].indices[[1, 0]]
    rc, msg = _set_rc(ctx, BLOB, m, _rigs_for(m), 4, 2)
    assert rc == E_INVALID and "topology changed: commit the scene again" in msg
    rc, msg = _set_rc(ctx, CUBE, cube, _rigs_for(cube), 4, 2, n_surfaces=len(cube.surfaces) - 1)
    assert rc == E_INVALID and "topology changed" in msg
    rc, msg = _set_rc(ctx, 0, blob, _rigs_for(blob), 4, 2)
    assert rc == E_INVALID and "topology changed" in msg
    assert ctx._lib.jpt_scene_set_mesh_rig(ctx.h, BLOB, None, None, 1, 4, 2) == E_INVALID

    def some_normals(arr, rarr):
        arr[0].normals = None
    rc, msg = _set_rc(ctx, CUBE, cube, _rigs_for(cube), 4, 2, edit=some_normals)
    assert rc == E_INVALID and "normals" in msg
    ctx.close()


def test_rig_argument_refusals(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    blob, cube = sc.meshes[BLOB], sc.meshes[CUBE]
    good = _rigs_for(blob)

    def rc_of(K=4, S=2, mesh=blob, mesh_id=BLOB, rigs=None, with_normals=True, edit=None, change=None):
        rigs = copy.deepcopy(good if rigs is None else rigs)
        if change:
            change(rigs)
        return _set_rc(ctx, mesh_id, mesh, rigs, K, S, with_normals=with_normals, edit=edit)

    for K in (-4, 1, 3, 5, 12, 16):
        rc, msg = rc_of(K=K)
        assert rc == E_INVALID and "influences" in msg, K
    assert rc_of(S=-1)[0] == E_INVALID
    rc, msg = rc_of(S=257)
    assert rc == E_LIMIT and "256" in msg
    rc, msg = rc_of(K=0, S=0)
    assert rc == E_INVALID and "bones or blend shapes" in msg
    arr = host._update_surfaces(blob)
    assert ctx._lib.jpt_scene_set_mesh_rig(ctx.h, BLOB, arr, None, 1, 4, 2) == E_INVALID

    def null(field):
        def edit(arr, rarr):
            setattr(rarr[0], field, None)
        return edit
    assert rc_of(edit=null("bones"))[0] == E_INVALID
    assert rc_of(edit=null("weights"))[0] == E_INVALID
    assert rc_of(edit=null("position_deltas"))[0] == E_INVALID
    # bones are not read without influences, deltas not without shapes
    assert rc_of(K=0, edit=null("bones"))[0] == E_DEVICE
    assert rc_of(S=0, edit=null("position_deltas"))[0] == E_DEVICE

    def put(field, value, at=(-1,)):
        def change(rigs):
            getattr(rigs[0], field).reshape(-1)[at[0]] = value
        return change
    for bad in (4096, 70000, -1):
        rc, msg = rc_of(change=put("bones", bad))
        assert rc == E_LIMIT and "4095" in msg, bad
    assert rc_of(change=put("bones", 4095))[0] == E_DEVICE
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = rc_of(change=put("weights", bad))
        assert rc == E_INVALID and "weight" in msg
        rc, msg = rc_of(change=put("position_deltas", bad, (0,)))
        assert rc == E_INVALID and "delta" in msg
        rc, msg = rc_of(change=put("normal_deltas", bad))
        assert rc == E_INVALID and "delta" in msg
    # normal deltas: for every surface or for none, and only beside bind normals
    crigs = _rigs_for(cube)
    rc, msg = _set_rc(ctx, CUBE, cube, crigs, 4, 2, edit=lambda arr, rarr: setattr(rarr[1], "normal_deltas", None))
    assert rc == E_INVALID and "normal deltas" in msg
    rc, msg = rc_of(with_normals=False)
    assert rc == E_INVALID and "normal deltas need bind normals" in msg
    assert rc_of(with_normals=False, edit=null("normal_deltas"))[0] == E_DEVICE
    ctx.close()


def test_a_valid_rig_needs_the_device_and_leaves_the_context_as_it_was(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    for mesh_id, K, S in ((BLOB, 4, 2), (BLOB, 8, 0), (BLOB, 0, 3), (CUBE, 4, 1)):
        mesh = sc.meshes[mesh_id]
        rc, msg = _set_rc(ctx, mesh_id, mesh, _rigs_for(mesh, K, S), K, S)
        assert rc == E_DEVICE and "host-only" in msg, (mesh_id, K, S)
        # nothing was stored: a pose finds no rig
        pal = np_skin.random_palette(np.random.RandomState(1), 6)
        assert ctx._lib.jpt_scene_pose_mesh(ctx.h, mesh_id, host._ptr(pal), 6, None, 0) == E_STATE
    assert len(ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, np.dtype((np.uint8, 48)))) > 0
    ctx.update_tlas()
    ctx.close()


def test_update_meshs_refusals_are_unchanged(hiplib):
    ctx = host.Context(-1)
    sc = scenes.demo_scene(n_tris=512)
    arr = host._update_surfaces(sc.meshes[BLOB])
    assert ctx._lib.jpt_scene_update_mesh(ctx.h, BLOB, arr, 1) == E_STATE
    assert ctx._lib.jpt_last_error(ctx.h).decode() == "jpt_scene_update_mesh needs a scene made by jpt_scene_commit with JPT_BUILD_SAH_WATERTIGHT"
    ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
    L = ctx._lib
    assert L.jpt_scene_update_mesh(ctx.h, 3, arr, 1) == E_INVALID and L.jpt_last_error(ctx.h) == b"no such mesh"
    assert L.jpt_scene_update_mesh(ctx.h, BLOB, None, 1) == E_INVALID and L.jpt_last_error(ctx.h) == b"bad surface array"
    assert L.jpt_scene_update_mesh(ctx.h, BLOB, arr, -1) == E_INVALID and L.jpt_last_error(ctx.h) == b"bad surface array"
    assert L.jpt_scene_update_mesh(ctx.h, 0, arr, 1) == E_INVALID and L.jpt_last_error(ctx.h) == b"topology changed: commit the scene again"
    carr = host._update_surfaces(sc.meshes[CUBE])
    carr[2].normals = None
    assert L.jpt_scene_update_mesh(ctx.h, CUBE, carr, 3) == E_INVALID
    assert L.jpt_last_error(ctx.h) == b"give normals for every surface of the mesh or for none"
    carr[2].vertices = None
    assert L.jpt_scene_update_mesh(ctx.h, CUBE, carr, 3) == E_INVALID and L.jpt_last_error(ctx.h) == b"surface needs a vertex array"
    assert L.jpt_scene_update_mesh(ctx.h, BLOB, arr, 1) == E_DEVICE
    assert L.jpt_last_error(ctx.h) == b"host-only context: the update runs on the device"
    assert L.jpt_scene_update_mesh(None, BLOB, arr, 1) == E_INVALID
    ctx.close()


def test_debug_skin_checks_its_arguments_as_the_context_calls_do(hiplib):
    rng = np.random.RandomState(9)
    nv = 20
    pos, nrm = rng.uniform(-1, 1, (nv, 3)).astype(np.float32), np.tile(np.float32([0, 0, 1]), (nv, 1))
    rig = np_skin.random_rig(rng, nv, 4, 2, 6)
    pal = np_skin.random_palette(rng, 8)

    def code(pos=pos, nrm=nrm, K=4, S=2, palette=pal, blend=(0.5, 0.25), change=None, **over):
        r = copy.deepcopy(rig)
        if change:
            change(r)
        fields = dict(bones=r.bones, weights=r.weights, position_deltas=r.position_deltas, normal_deltas=r.normal_deltas)
        fields.update(over)
        try:
            host.debug_skin(-1, pos, nrm, host.SurfaceRig(**fields), K, S, palette, blend)
        except capi.JptError as e:
            return e.args[1], e.args[0]
        return OK, ""

    assert code()[0] == OK
    # the pose: a palette that reaches the rig's largest bone index (5), one finite weight per shape
    assert code(palette=pal[:6])[0] == OK
    rc, msg = code(palette=pal[:5])
    assert rc == E_INVALID and "bone 5" in msg
    assert code(palette=None)[0] == E_INVALID
    assert code(K=0, palette=None)[0] == OK
    for bad in (np.nan, np.inf):
        rc, msg = code(blend=(0.5, bad))
        assert rc == E_INVALID and "blend weight" in msg
    assert code(blend=None)[0] == E_INVALID   # (the binding passes NULL)
    # the rig: jpt_scene_set_mesh_rig's checks
    assert code(K=3)[0] == E_INVALID
    assert code(S=257)[0] == E_LIMIT
    assert code(K=0, S=0, blend=None)[0] == E_INVALID
    assert code(bones=None)[0] == E_INVALID and code(weights=None)[0] == E_INVALID and code(position_deltas=None)[0] == E_INVALID
    assert code(change=lambda r: r.bones.__setitem__((3, 1), 4096))[0] == E_LIMIT
    assert code(change=lambda r: r.bones.__setitem__((3, 1), -2))[0] == E_LIMIT
    assert code(change=lambda r: r.weights.__setitem__((0, 0), np.nan))[0] == E_INVALID
    assert code(change=lambda r: r.position_deltas.__setitem__((1, 2, 0), np.inf))[0] == E_INVALID
    assert code(change=lambda r: r.normal_deltas.__setitem__((1, 2, 0), np.nan))[0] == E_INVALID
    rc, msg = code(nrm=None)
    assert rc == E_INVALID and "normal deltas need bind normals" in msg
    assert code(nrm=None, normal_deltas=None)[0] == OK
    L = capi.lib()
    assert L.jpt_debug_skin(-1, None, None, 4, None, None, 0, None, None, 0, None, 0, None, None, None) == E_INVALID
    out = np.zeros((nv, 3), np.float32)
    assert L.jpt_debug_skin(-1, host._ptr(pos), None, 0, None, None, 0, host._ptr(rig.position_deltas), None, 2, None, 0, host._ptr(np.float32([1, 1])),
                            host._ptr(out), None) == E_INVALID


# ---- the header, the binding, the wrappers ----------------------------------------------------------------------------------

NEW = ("jpt_scene_set_mesh_rig", "jpt_scene_pose_mesh", "jpt_scene_clear_mesh_rig", "jpt_multi_set_mesh_rig", "jpt_multi_pose_mesh",
       "jpt_multi_clear_mesh_rig", "jpt_debug_skin")

_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "jpt.h"
int main(void)
{
    printf("%d %d\n", JPT_ABI_VERSION, jpt_abi_version());
    printf("%zu %zu %zu %zu %zu\n", sizeof(jpt_surface_rig), offsetof(jpt_surface_rig, bones), offsetof(jpt_surface_rig, weights),
           offsetof(jpt_surface_rig, position_deltas), offsetof(jpt_surface_rig, normal_deltas));
    /* the declared types: a mismatch with these pointers is a compile error */
    int (*a)(jpt_ctx *, uint32_t, const jpt_surface *, const jpt_surface_rig *, int32_t, int32_t, int32_t) = jpt_scene_set_mesh_rig;
    int (*b)(jpt_ctx *, uint32_t, const float *, uint32_t, const float *, uint32_t) = jpt_scene_pose_mesh;
    int (*c)(jpt_ctx *, uint32_t) = jpt_scene_clear_mesh_rig;
    int (*d)(jpt_multi *, uint32_t, const jpt_surface *, const jpt_surface_rig *, int32_t, int32_t, int32_t) = jpt_multi_set_mesh_rig;
    int (*e)(jpt_multi *, uint32_t, const float *, uint32_t, const float *, uint32_t) = jpt_multi_pose_mesh;
    int (*f)(jpt_multi *, uint32_t) = jpt_multi_clear_mesh_rig;
    int (*g)(int, const float *, const float *, uint32_t, const int32_t *, const float *, int32_t, const float *, const float *, int32_t,
             const float *, uint32_t, const float *, float *, float *) = jpt_debug_skin;
    printf("%d\n", a && b && c && d && e && f && g);
    return 0;
}
"""


def test_header_and_binding_agree(hiplib, tmp_path):
    L = capi.lib()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    pub = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, pub), name
    assert re.search(r"#define\s+JPT_ABI_VERSION\s+6\b", pub) and L.jpt_abi_version() == 6
    src, exe = tmp_path / "abi.c", str(tmp_path / "abi")
    src.write_text(_C)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-ljpt_hip",
                           "-Wl,-rpath," + libdir])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert lines[0] == "6 6" and lines[2] == "1"
    R = capi.SurfaceRig
    assert [int(x) for x in lines[1].split()] == [C.sizeof(R), R.bones.offset, R.weights.offset, R.position_deltas.offset, R.normal_deltas.offset]
    assert [n for n, _ in R._fields_] == ["bones", "weights", "position_deltas", "normal_deltas"]
    assert C.sizeof(R) == 4 * C.sizeof(C.c_void_p)
    assert L.jpt_multi_set_mesh_rig(None, 0, None, None, 0, 4, 0) == E_INVALID
    assert L.jpt_multi_pose_mesh(None, 0, None, 0, None, 0) == E_INVALID
    assert L.jpt_multi_clear_mesh_rig(None, 0) == E_INVALID
    assert L.jpt_scene_set_mesh_rig(None, 0, None, None, 0, 4, 0) == E_INVALID
    assert L.jpt_scene_pose_mesh(None, 0, None, 0, None, 0) == E_INVALID
    assert L.jpt_scene_clear_mesh_rig(None, 0) == E_INVALID


def test_python_wrappers_reach_the_calls(hiplib):
    ctx, sc = _committed(capi.BUILD_SAH_WATERTIGHT)
    rigs = [host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas) for r in _rigs_for(sc.meshes[BLOB])]
    pal = np_skin.random_palette(np.random.RandomState(2), 6)
    with pytest.raises(capi.JptError, match="jpt_scene_set_mesh_rig failed .*host-only"):
        ctx.set_mesh_rig(BLOB, sc.meshes[BLOB], rigs, 4, 2)
    with pytest.raises(capi.JptError, match=r"jpt_scene_pose_mesh failed \(-4\).*no rig"):
        ctx.pose_mesh(BLOB, pal, [0.5, 0.0])
    ctx.clear_mesh_rig(BLOB)
    assert host.Context.debug_skin is host.debug_skin
    g = host.GeometryGroup3D(scenes.demo_scene(n_tris=512), capi.BUILD_SAH_WATERTIGHT)
    g.build(host.Context(-1))
    with pytest.raises(capi.JptError, match="jpt_scene_set_mesh_rig failed .*host-only"):
        g.set_mesh_rig(BLOB, rigs, 4, 2)
    with pytest.raises(capi.JptError, match=r"jpt_scene_pose_mesh failed \(-4\)"):
        g.pose_mesh(BLOB, pal, [0.5, 0.0])
    g.clear_mesh_rig(BLOB)
    for name in ("set_mesh_rig", "pose_mesh", "clear_mesh_rig", "debug_skin"):
        assert hasattr(host.MultiContext, name) and hasattr(host.GeometryGroup3D, name), name
    ctx.close()


_CPP = r"""
#include <cstdio>
#include <stdexcept>
#include "jpt_host.hpp"
using namespace jpt_host;

int main()
{
    jpt_ctx* ctx = nullptr;
    if (jpt_create(JPT_DEVICE_HOST_ONLY, &ctx) != JPT_OK) return 2;
    ArrayMesh mesh, other;
    Surface x;
    x.vertices = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    x.normals = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    x.uvs = {0, 0, 1, 0, 0, 1, 1, 1};
    x.indices = {0, 1, 2, 0, 1, 3, 0, 2, 3, 1, 2, 3};
    mesh.surfaces.push_back(x);
    other = mesh;
    MeshInstance3D node;
    node.mesh = &mesh;
    GeometryGroup3D g;
    g.builder = JPT_BUILD_SAH_WATERTIGHT;
    g.add_child(node);
    g.build(ctx);
    SurfaceRig r;
    r.bones = {0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0};
    r.weights = {1, 0, 0, 0, 0.5f, 0.5f, 0, 0, 1, 0, 0, 0, 0.25f, 0.75f, 0, 0};
    const std::vector<float> palette = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0.5f, 0};
    auto attempt = [](const char* what, auto&& f) {
        try {
            f();
            std::printf("%s: done\n", what);
        } catch (const std::exception& e) {
            std::printf("%s: %s\n", what, e.what());
        }
    };
    attempt("set", [&] { g.set_mesh_rig(&mesh, {r}, 4, 0); });
    attempt("pose", [&] { g.pose_mesh(&mesh, palette, {}); });
    attempt("clear", [&] { g.clear_mesh_rig(&mesh); });
    attempt("other", [&] { g.set_mesh_rig(&other, {r}, 4, 0); });
    jpt_destroy(ctx);
    return 0;
}
"""


def test_cpp_geometry_group_wrappers_reach_the_calls(hiplib, tmp_path):
    src, exe = tmp_path / "rig.cpp", str(tmp_path / "rig")
    src.write_text(_CPP)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-ljpt_hip",
                           "-Wl,-rpath," + libdir])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[0].startswith("set: ") and "jpt_scene_set_mesh_rig" in lines[0] and "host-only" in lines[0], lines
    assert lines[1].startswith("pose: ") and "jpt_scene_pose_mesh" in lines[1] and "no rig" in lines[1], lines
    assert lines[2] == "clear: done", lines
    assert "not part of the last build()" in lines[3], lines
