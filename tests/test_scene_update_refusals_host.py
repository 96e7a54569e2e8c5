"""The refusals of the calls that change a committed scene without a new commit -- jpt_scene_set_instance_transform, jpt_scene_update_tlas,
jpt_scene_refit_tlas, jpt_scene_rebuild_tlas, jpt_scene_update_mesh, jpt_scene_set_mesh_rig, jpt_scene_pose_mesh -- and of the two calls that
read their results, jpt_debug_mesh_records and jpt_debug_tlas_records, on host-only contexts: every state and argument check runs before the
device is asked for, so each is reached without one.  Return code and the whole jpt_last_error text against a literal table, written down from
the library as it was before the device updates were gathered into one file (csrc/jpt_scene_update.cpp)."""
import copy
import ctypes as C

import numpy as np
import pytest

import np_skin
from gdpathtracing_amd import capi, host, scenes, wire

OK, E_INVALID, E_DEVICE, E_STATE = 0, -1, -2, -4   # JPT_OK, JPT_E_INVALID, JPT_E_DEVICE, JPT_E_STATE of include/jpt.h
BOX, CUBE = 0, 1   # the scene's one-surface box and its three-surface open cube
K, S, N_BONES = 4, 2, 6


def make_scene():
    """two small meshes, three instances"""
    base = scenes.cornell_scene()
    inst = [scenes.Instance(BOX, scenes.transform12(scenes.rot_y(-17.0), (1.0, -2.15, 0.9)), [2]),
            scenes.Instance(CUBE, base.instances[1].transform, [2, 3, 4]),
            scenes.Instance(BOX, scenes.transform12(scenes.rot_y(20.0), (-1.0, -1.3, -0.9)), [6])]
    return scenes.Scene("two_meshes", [scenes.box_mesh(1.7, 1.7, 1.7), scenes.cornell_cube_mesh()], inst, base.materials, base.camera)


SCENE = make_scene()
T3 = np.ascontiguousarray(np.stack([i.transform for i in SCENE.instances]), dtype=np.float32)
PALETTE = np_skin.random_palette(np.random.RandomState(2), N_BONES)


def rigs_of(mesh):
    rng = np.random.RandomState(3)
    return [np_skin.random_rig(rng, len(s.vertices), K, S, N_BONES) for s in mesh.surfaces]


def swapped(mesh):
    """the mesh with two indices of its first triangle exchanged: another topology"""
    m = copy.deepcopy(mesh)
    m.surfaces[0].indices[[0, 1]] = m.surfaces[0].indices[[1, 0]]
    return m


# ---- the calls, each with arguments that are in order unless the row says otherwise -------------------------------------------------

def set_transform(L, h, instance=0, t=T3[0]):
    return L.jpt_scene_set_instance_transform(h, instance, host._ptr(t))


def update_tlas(L, h):
    return L.jpt_scene_update_tlas(h)


def refit(L, h, t=T3, n=3):
    return L.jpt_scene_refit_tlas(h, host._ptr(t), n)


def rebuild(L, h, t=T3, n=3):
    return L.jpt_scene_rebuild_tlas(h, host._ptr(t), n)


def update_mesh(L, h, mesh_id=BOX, mesh=None, edit=None):
    mesh = SCENE.meshes[mesh_id if mesh_id < len(SCENE.meshes) else BOX] if mesh is None else mesh
    arr = host._update_surfaces(mesh)
    if edit:
        edit(arr)
    return L.jpt_scene_update_mesh(h, mesh_id, arr, len(mesh.surfaces))


def set_rig(L, h, mesh_id=BOX, mesh=None, edit=None, null_rigs=False):
    mesh = SCENE.meshes[mesh_id if mesh_id < len(SCENE.meshes) else BOX] if mesh is None else mesh
    arr = host._update_surfaces(mesh)
    keep = [host.SurfaceRig(r.bones, r.weights, r.position_deltas, r.normal_deltas) for r in rigs_of(mesh)]
    rarr = host._rig_surfaces(keep)
    if edit:
        edit(arr)
    return L.jpt_scene_set_mesh_rig(h, mesh_id, arr, None if null_rigs else rarr, len(mesh.surfaces), K, S)


def pose(L, h, mesh_id=BOX):
    return L.jpt_scene_pose_mesh(h, mesh_id, host._ptr(PALETTE), N_BONES, host._ptr(np.float32([0.5, 0.25])), S)


def mesh_records(L, h, mesh_id=BOX):
    info = (C.c_int32 * 6)()
    return L.jpt_debug_mesh_records(h, mesh_id, None, None, 0, None, None, 0, info)


def tlas_records(L, h):
    n, root = C.c_uint32(), C.c_int32()
    return L.jpt_debug_tlas_records(h, None, None, 0, C.byref(n), C.byref(root), None, None)


CALLS = dict(jpt_scene_set_instance_transform=set_transform, jpt_scene_update_tlas=update_tlas, jpt_scene_refit_tlas=refit,
             jpt_scene_rebuild_tlas=rebuild, jpt_scene_update_mesh=update_mesh, jpt_scene_set_mesh_rig=set_rig, jpt_scene_pose_mesh=pose,
             jpt_debug_mesh_records=mesh_records, jpt_debug_tlas_records=tlas_records)


# ---- the states ------------------------------------------------------------------------------------------------------------------------

def _upload(ctx, as_given):
    src = host.Context(-1)
    src.build_scene(SCENE, capi.BUILD_REFERENCE_EXACT)
    bufs = [src.reference_buffer(which, dtype) for which, dtype in
            ((capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY), (capi.BUF_TRI_DATA, wire.TRI_DATA), (capi.BUF_MATERIALS, wire.MATERIAL),
             (capi.BUF_BVH_NODES, wire.BVH_NODE), (capi.BUF_INSTANCES, wire.BLAS_INSTANCE), (capi.BUF_TLAS_NODES, wire.TLAS_NODE))]
    src.close()
    ctx.upload_reference_layout(*bufs, as_given=as_given)


def _begun(ctx):
    ctx.build_scene(SCENE, capi.BUILD_SAH_WATERTIGHT)
    assert ctx._lib.jpt_scene_begin(ctx.h) == OK


STATES = {
    "no scene": lambda ctx: None,
    "begun": _begun,                                               # between jpt_scene_begin and the commit
    "upload": lambda ctx: _upload(ctx, False),                     # a reference-layout upload (the native tree over it): not from a commit
    "upload as given": lambda ctx: _upload(ctx, True),
    "reference exact": lambda ctx: ctx.build_scene(SCENE, capi.BUILD_REFERENCE_EXACT),
    "sah": lambda ctx: ctx.build_scene(SCENE, capi.BUILD_SAH),
    "watertight": lambda ctx: ctx.build_scene(SCENE, capi.BUILD_SAH_WATERTIGHT),
}
NOT_COMMITTED = ("no scene", "begun", "upload", "upload as given")

COMMIT = " needs a scene made by jpt_scene_commit"
NATIVE = COMMIT + " with the native builder"
WATERTIGHT = COMMIT + " with JPT_BUILD_SAH_WATERTIGHT"
REFERENCE_TREES = ("the scene was committed with JPT_BUILD_REFERENCE_EXACT: its trees are the reference's own, which a refit would not keep "
                   "(commit with JPT_BUILD_SAH_WATERTIGHT to deform meshes on the device)")
SAH_TREES = ("the scene was committed with JPT_BUILD_SAH: its reach records and tie shadow are the reference builder's tree of the committed "
             "vertices (commit with JPT_BUILD_SAH_WATERTIGHT to deform meshes on the device)")
REFIT_HOST_ONLY = "host-only context: the refit runs on the device (jpt_scene_update_tlas is the host route)"
RECORDS_HOST_ONLY = "host-only context: the records are on the device"
NO_RIG = "jpt_scene_pose_mesh: the mesh has no rig (jpt_scene_set_mesh_rig; a commit or an upload drops it)"
DONE = (OK, None)   # the call succeeds: there is no text of its own to compare


def _row(not_committed, reference_exact, sah, watertight):
    row = {s: not_committed for s in NOT_COMMITTED}
    row.update({"reference exact": reference_exact, "sah": sah, "watertight": watertight})
    return row


# call -> state -> (return code, the whole text)
TABLE = {
    "jpt_scene_set_instance_transform": _row((E_STATE, "jpt_scene_set_instance_transform" + COMMIT), DONE, DONE, DONE),
    "jpt_scene_update_tlas": _row((E_STATE, "jpt_scene_update_tlas" + COMMIT), DONE, DONE, DONE),
    "jpt_scene_refit_tlas": _row((E_STATE, "jpt_scene_refit_tlas" + NATIVE), (E_STATE, "jpt_scene_refit_tlas" + NATIVE),
                                 (E_DEVICE, REFIT_HOST_ONLY), (E_DEVICE, REFIT_HOST_ONLY)),
    "jpt_scene_rebuild_tlas": _row((E_STATE, "jpt_scene_rebuild_tlas" + NATIVE), (E_STATE, "jpt_scene_rebuild_tlas" + NATIVE),
                                   (E_DEVICE, REFIT_HOST_ONLY), (E_DEVICE, REFIT_HOST_ONLY)),
    "jpt_scene_update_mesh": _row((E_STATE, "jpt_scene_update_mesh" + WATERTIGHT), (E_STATE, REFERENCE_TREES), (E_STATE, SAH_TREES),
                                  (E_DEVICE, "host-only context: the update runs on the device")),
    "jpt_scene_set_mesh_rig": _row((E_STATE, "jpt_scene_set_mesh_rig" + WATERTIGHT), (E_STATE, REFERENCE_TREES), (E_STATE, SAH_TREES),
                                   (E_DEVICE, "host-only context: the rig is kept on the device")),
    "jpt_scene_pose_mesh": _row((E_STATE, "jpt_scene_pose_mesh" + WATERTIGHT), (E_STATE, "jpt_scene_pose_mesh" + WATERTIGHT),
                                (E_STATE, "jpt_scene_pose_mesh" + WATERTIGHT), (E_STATE, NO_RIG)),
    "jpt_debug_mesh_records": _row((E_STATE, "jpt_debug_mesh_records needs a scene committed with JPT_BUILD_SAH_WATERTIGHT"),
                                   (E_STATE, "jpt_debug_mesh_records needs a scene committed with JPT_BUILD_SAH_WATERTIGHT"),
                                   (E_STATE, "jpt_debug_mesh_records needs a scene committed with JPT_BUILD_SAH_WATERTIGHT"),
                                   (E_DEVICE, RECORDS_HOST_ONLY)),
    "jpt_debug_tlas_records": _row((E_STATE, "jpt_debug_tlas_records" + NATIVE), (E_STATE, "jpt_debug_tlas_records" + NATIVE),
                                   (E_DEVICE, RECORDS_HOST_ONLY), (E_DEVICE, RECORDS_HOST_ONLY)),
}


def some_normals(arr):
    arr[2].normals = None


# the argument refusals, on the watertight commit: label -> (the call, return code, the whole text)
ARGUMENTS = {
    "a null transform: set_instance_transform": (lambda L, h: set_transform(L, h, t=None), E_INVALID, "null transform"),
    "a null transform: refit": (lambda L, h: refit(L, h, t=None), E_INVALID, "null transforms"),
    "a null transform: rebuild": (lambda L, h: rebuild(L, h, t=None), E_INVALID, "null transforms"),
    "an instance past the end": (lambda L, h: set_transform(L, h, instance=3), E_INVALID, "no such instance"),
    "a wrong instance count: refit": (lambda L, h: refit(L, h, n=2), E_INVALID, "one transform per instance of the committed scene"),
    "a wrong instance count: rebuild": (lambda L, h: rebuild(L, h, n=2), E_INVALID, "one transform per instance of the committed scene"),
    "a mesh id past the end: update_mesh": (lambda L, h: update_mesh(L, h, mesh_id=2), E_INVALID, "no such mesh"),
    "a mesh id past the end: set_mesh_rig": (lambda L, h: set_rig(L, h, mesh_id=2), E_INVALID, "no such mesh"),
    "a mesh id past the end: pose_mesh": (lambda L, h: pose(L, h, mesh_id=2), E_STATE, NO_RIG),
    "a mesh id past the end: mesh_records": (lambda L, h: mesh_records(L, h, mesh_id=2), E_INVALID, "no such mesh"),
    "a changed topology: update_mesh": (lambda L, h: update_mesh(L, h, mesh=swapped(SCENE.meshes[BOX])), E_INVALID,
                                        "topology changed: commit the scene again"),
    "a changed topology: set_mesh_rig": (lambda L, h: set_rig(L, h, mesh=swapped(SCENE.meshes[BOX])), E_INVALID,
                                         "topology changed: commit the scene again"),
    "another mesh's arrays: update_mesh": (lambda L, h: update_mesh(L, h, mesh_id=BOX, mesh=SCENE.meshes[CUBE]), E_INVALID,
                                           "topology changed: commit the scene again"),
    "normals for some surfaces only: update_mesh": (lambda L, h: update_mesh(L, h, mesh_id=CUBE, edit=some_normals), E_INVALID,
                                                    "give normals for every surface of the mesh or for none"),
    "normals for some surfaces only: set_mesh_rig": (lambda L, h: set_rig(L, h, mesh_id=CUBE, edit=some_normals), E_INVALID,
                                                     "give normals for every surface of the mesh or for none"),
    "a null surface array: update_mesh": (lambda L, h: L.jpt_scene_update_mesh(h, BOX, None, 1), E_INVALID, "bad surface array"),
    "a null rig array": (lambda L, h: set_rig(L, h, null_rigs=True), E_INVALID, "jpt_scene_set_mesh_rig: bad rig array"),
    "a pose of a mesh without a rig": (lambda L, h: pose(L, h, mesh_id=CUBE), E_STATE, NO_RIG),
}

# the order: the scene's state is asked before the arguments -- the same bad arguments where no scene was committed
STATE_FIRST = {
    "jpt_scene_set_instance_transform": lambda L, h: set_transform(L, h, t=None),
    "jpt_scene_refit_tlas": lambda L, h: refit(L, h, t=None, n=2),
    "jpt_scene_rebuild_tlas": lambda L, h: rebuild(L, h, t=None, n=2),
    "jpt_scene_update_mesh": lambda L, h: update_mesh(L, h, mesh_id=2),
    "jpt_scene_set_mesh_rig": lambda L, h: set_rig(L, h, mesh_id=2, null_rigs=True),
    "jpt_scene_pose_mesh": lambda L, h: pose(L, h, mesh_id=2),
    "jpt_debug_mesh_records": lambda L, h: mesh_records(L, h, mesh_id=2),
}


def context_in(state):
    ctx = host.Context(-1)
    STATES[state](ctx)
    return ctx


def refusal(L, h, call):
    L.jpt_set_kernel_timing(h, 0)   # (a call that succeeds and leaves the error text alone: the text below is this call's)
    rc = call(L, h)
    return rc, L.jpt_last_error(h).decode()


def check(L, h, call, want):
    rc, text = refusal(L, h, call)
    assert (rc, text if want[1] is not None else None) == want


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_refusal_of_each_call_in_each_state(hiplib, name, state):
    ctx = context_in(state)
    try:
        check(capi.lib(), ctx.h, CALLS[name], TABLE[name][state])
    finally:
        ctx.close()


@pytest.mark.parametrize("label", sorted(ARGUMENTS))
def test_the_argument_refusals(hiplib, label):
    call, rc, text = ARGUMENTS[label]
    ctx = context_in("watertight")
    try:
        check(capi.lib(), ctx.h, call, (rc, text))
    finally:
        ctx.close()


@pytest.mark.parametrize("state", NOT_COMMITTED)
@pytest.mark.parametrize("name", sorted(STATE_FIRST))
def test_the_state_is_asked_before_the_arguments(hiplib, name, state):
    ctx = context_in(state)
    try:
        check(capi.lib(), ctx.h, STATE_FIRST[name], TABLE[name][state])
    finally:
        ctx.close()


def test_the_builder_is_asked_before_the_arguments_and_the_arguments_before_the_device(hiplib):
    L = capi.lib()
    for state, trees in (("reference exact", REFERENCE_TREES), ("sah", SAH_TREES)):
        ctx = context_in(state)
        check(L, ctx.h, STATE_FIRST["jpt_scene_update_mesh"], (E_STATE, trees))
        check(L, ctx.h, STATE_FIRST["jpt_scene_set_mesh_rig"], (E_STATE, trees))
        ctx.close()
    ctx = context_in("sah")
    check(L, ctx.h, STATE_FIRST["jpt_scene_refit_tlas"], (E_INVALID, "null transforms"))
    check(L, ctx.h, lambda L, h: refit(L, h, n=2), (E_INVALID, "one transform per instance of the committed scene"))
    check(L, ctx.h, refit, (E_DEVICE, REFIT_HOST_ONLY))
    ctx.close()


def test_calls_without_a_context_or_a_result_array(hiplib):
    L = capi.lib()
    for call in CALLS.values():
        assert call(L, None) == E_INVALID
    ctx = context_in("watertight")
    assert L.jpt_debug_mesh_records(ctx.h, BOX, None, None, 0, None, None, 0, None) == E_INVALID
    ctx.close()
