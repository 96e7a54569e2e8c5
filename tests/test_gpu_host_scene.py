"""The host scene's transitions (csrc/jpt_scene.cpp) as the device sees them: what a rejected update, a refused upload and jpt_scene_share
leave for the next render and the next ray query (csrc/jpt_query.cpp).  Every case is a refusal the library returns or a render of a
scene it accepted; cornell_scene() at 32 x 32, 2 frames, 2 bounces; every comparison is bitwise.  The two word-for-word "a mesh was
deformed on the device" refusals and jpt_scene_share's own are here too: only a device deforms a mesh."""
import ctypes as C

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

pytestmark = pytest.mark.gpu

OK, E_INVALID, E_LIMIT, E_STATE = 0, -1, -3, -4   # include/jpt.h
W = H = 32
SCENE = scenes.cornell_scene()
CAMERA = scenes.camera_block(SCENE.camera, W, H)
T12 = np.ascontiguousarray(np.stack([i.transform for i in SCENE.instances]), dtype=np.float32)
NO_SCENE = "no scene: call jpt_scene_upload_reference_layout or jpt_scene_commit first"
DEFORMED = "a mesh was deformed on the device (jpt_scene_update_mesh): the host's copy of the scene is stale until the next jpt_scene_commit"
DEFORMED_SOURCE = ("the source context's meshes were deformed on the device (jpt_scene_update_mesh): its host copy of the scene is stale until "
                   "the next jpt_scene_commit")
NOT_NATIVE_FIT = ("the new instance level does not fit the native tree of the last upload (TLAS child index out of range): upload the whole "
                  "scene again, or with JPT_UPLOAD_WALK_AS_GIVEN")


@pytest.fixture(scope="module")
def arrays(hiplib):
    """the scene as a host would upload it: the arrays of a reference-exact commit"""
    src = host.Context(-1)
    src.build_scene(SCENE, capi.BUILD_REFERENCE_EXACT)
    out = [src.reference_buffer(which, dtype) for which, dtype in
           ((capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY), (capi.BUF_TRI_DATA, wire.TRI_DATA), (capi.BUF_MATERIALS, wire.MATERIAL),
            (capi.BUF_BVH_NODES, wire.BVH_NODE), (capi.BUF_INSTANCES, wire.BLAS_INSTANCE), (capi.BUF_TLAS_NODES, wire.TLAS_NODE))]
    src.close()
    return out


def deep(arrays, depth=200):
    """tests/test_capi_host.py's chain of `depth` internal nodes under one instance: refused as too deep when walked as given"""
    tri, dat = np.repeat(arrays[0][:1], depth + 1), np.repeat(arrays[1][:1], depth + 1)
    nodes = np.zeros(2 * depth + 1, dtype=wire.BVH_NODE)
    nodes["aabbMin"][:, :3] = -1
    nodes["aabbMax"][:, :3] = 1
    for i in range(depth):
        nodes[2 * i]["left_child"], nodes[2 * i]["right_child"] = 2 * i + 1, 2 * i + 2
        nodes[2 * i + 1]["first_tri_index"], nodes[2 * i + 1]["tri_count"] = i, 1
    nodes[2 * depth]["first_tri_index"], nodes[2 * depth]["tri_count"] = depth, 1
    inst = arrays[4][:1].copy()
    inst["blas_index"] = 0
    tlas = np.zeros(2, dtype=wire.TLAS_NODE)
    tlas["aabbMin"], tlas["aabbMax"] = -1, 1
    return [tri, dat, arrays[2], nodes, inst, tlas]


def context():
    ctx = host.Context(0)
    ctx.set_params(W, H, 2, capi.ACCUM_REF_LDR8)
    ctx.set_camera(CAMERA)
    return ctx


def rendered(ctx):
    """the sum and the display image of frames 1 and 2, from a sum that starts over"""
    ctx.accum_reset()
    ctx.render(2, 1)
    return ctx.read_accum().tobytes(), ctx.read_ldr().tobytes()


def rays16():
    rng = np.random.RandomState(16)
    origins = np.tile(np.float32(SCENE.camera.transform[9:12]), (16, 1))
    dirs = rng.normal(size=(16, 3)).astype(np.float32) * np.float32([0.4, 0.4, 0.1]) + np.float32([0, 0, -1])
    return origins, dirs


def queried(ctx):
    hits, occ = ctx.query_rays(*rays16())
    return hits.tobytes(), occ.tobytes()


@pytest.mark.parametrize("as_given", [True, False])
def test_a_rejected_reference_tlas_update_leaves_the_render(hiplib, arrays, as_given):
    ctx = context()
    try:
        ctx.upload_reference_layout(*arrays, as_given=as_given)
        before, hits = rendered(ctx), queried(ctx)
        bad = arrays[5].copy()
        bad["leftRight"][0] = 0xFFFF_FFFF   # slot 0 is the root: both children out of range
        rc = hiplib.jpt_scene_update_reference_tlas(ctx.h, host._ptr(arrays[4]), len(arrays[4]), host._ptr(bad), len(bad))
        assert (rc, ctx.last_error()) == (E_INVALID, "tlas update: TLAS child index out of range" if as_given else NOT_NATIVE_FIT)
        assert ctx.tree_kind() == (capi.TREE_AS_GIVEN if as_given else capi.TREE_NATIVE_REACH)
        assert rendered(ctx) == before and queried(ctx) == hits
    finally:
        ctx.close()


def test_a_refused_upload_leaves_no_scene_and_a_good_one_renders_like_a_fresh_context(hiplib, arrays):
    ctx, fresh = context(), context()
    try:
        ctx.upload_reference_layout(*arrays)
        first, hits = rendered(ctx), queried(ctx)
        assert any(hits[1])   # some of the 16 rays hit the box
        with pytest.raises(capi.JptError, match="acceleration structure too deep: a traversal could need 201 stack entries, the kernels hold 96"):
            ctx.upload_reference_layout(*deep(arrays), as_given=True)
        assert ctx.tree_kind() == capi.TREE_NONE
        for entry in ("jpt_render", "jpt_render_counted", "jpt_render_async"):
            assert (getattr(hiplib, entry)(ctx.h, 1, 1), ctx.last_error()) == (E_STATE, NO_SCENE)
        rays = host.make_rays(*rays16())
        out, occ = np.zeros(16, wire.RAY_HIT), np.zeros(16, np.uint8)
        rc = hiplib.jpt_query_rays(ctx.h, capi.QUERY_CLOSEST, host._ptr(rays), 16, host._ptr(out), host._ptr(occ))
        assert (rc, ctx.last_error()) == (E_STATE, "jpt_query_rays: no scene")
        rc = hiplib.jpt_query_rays(ctx.h, capi.QUERY_ANY, host._ptr(rays), 16, None, host._ptr(occ))
        assert (rc, ctx.last_error()) == (E_STATE, "jpt_query_rays: no scene")
        xy = np.float32([[16.5, 16.5]])
        assert (hiplib.jpt_query_pixels(ctx.h, host._ptr(xy), 1, host._ptr(out)), ctx.last_error()) == (E_STATE, "jpt_query_pixels: no scene")
        ctx.upload_reference_layout(*arrays)
        fresh.upload_reference_layout(*arrays)
        again = rendered(ctx)
        assert again == rendered(fresh) == first
        assert queried(ctx) == queried(fresh) == hits
    finally:
        ctx.close()
        fresh.close()


def test_a_share_from_a_context_refitted_on_the_device(hiplib):
    src, dst = context(), context()
    try:
        src.build_scene(SCENE, capi.BUILD_SAH)
        moved = T12.copy()
        moved[1, 9:12] += np.float32([0.4, 0.0, -0.3])
        src.refit_tlas(moved)
        rendered(src)
        dst.share_scene_from(src)   # (brings the source's host arrays up to date first: jpt_scene_update_tlas)
        assert dst.tree_kind() == src.tree_kind() == capi.TREE_NATIVE_REACH
        for which in (capi.BUF_INSTANCES, capi.BUF_TLAS_NODES, capi.BUF_REACH_INSTANCES):
            assert dst.reference_buffer(which, np.uint8).tobytes() == src.reference_buffer(which, np.uint8).tobytes()
        assert rendered(dst) == rendered(src)
        assert queried(dst) == queried(src)
    finally:
        dst.close()
        src.close()


def test_the_refusals_of_a_scene_whose_mesh_was_deformed_on_the_device(hiplib):
    ctx, dst = context(), host.Context(-1)
    try:
        ctx.build_scene(SCENE, capi.BUILD_SAH_WATERTIGHT)
        ctx.update_mesh(1, SCENE.meshes[1])   # (the committed vertices again: deformed all the same)
        ctx.sync()
        assert (hiplib.jpt_scene_update_tlas(ctx.h), ctx.last_error()) == (E_STATE, DEFORMED)
        n = C.c_size_t()
        for which in (capi.BUF_TRI_GEOMETRY, capi.BUF_INSTANCES):
            hiplib.jpt_set_kernel_timing(ctx.h, 0)
            assert (hiplib.jpt_scene_get_reference_buffer(ctx.h, which, None, 0, C.byref(n)), ctx.last_error()) == (E_STATE, DEFORMED)
        assert (hiplib.jpt_scene_share(dst.h, ctx.h), dst.last_error()) == (E_STATE, DEFORMED_SOURCE)
        assert dst.tree_kind() == capi.TREE_NONE and ctx.tree_kind() == capi.TREE_NATIVE_WATERTIGHT
        ctx.build_scene(SCENE, capi.BUILD_SAH_WATERTIGHT)   # the next commit: the host's copy is the scene again
        ctx.update_tlas()
        assert len(ctx.reference_buffer(capi.BUF_INSTANCES, wire.BLAS_INSTANCE)) == len(SCENE.instances)
        rendered(ctx)
    finally:
        dst.close()
        ctx.close()
