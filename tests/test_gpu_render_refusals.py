"""The refusals of the three render entry points -- jpt_render, jpt_render_counted, jpt_render_async -- on the device: return code and the
whole jpt_last_error text against a literal table, written down from the library as it was before the render pipeline was gathered into one
file (csrc/jpt_render.cpp).  On the device, because a host-only context refuses every render with its own sentence first (that row:
test_the_host_only_refusal_comes_first, which needs no GPU).  Cornell at 16 x 16 with one bounce: no row renders more than two frames."""
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

OK, E_INVALID, E_DEVICE, E_LIMIT, E_STATE = 0, -1, -2, -3, -4   # JPT_OK and the JPT_E_* codes of include/jpt.h
W = H = 16
SCENE = scenes.cornell_scene()
CAMERA = scenes.camera_block(SCENE.camera, W, H)
T12 = np.ascontiguousarray(np.stack([i.transform for i in SCENE.instances]), dtype=np.float32)
ENTRIES = ("jpt_render", "jpt_render_counted", "jpt_render_async")

HOST_ONLY = "host-only context (JPT_DEVICE_HOST_ONLY) cannot render: there is no CPU fallback"
NO_SCENE = "no scene: call jpt_scene_upload_reference_layout or jpt_scene_commit first"
NO_PARAMS = "jpt_set_params not called"
NO_CAMERA = "jpt_set_camera not called"
NEGATIVE = "n_frames < 0"
BUDGET = r"jpt_set_memory_policy: one frame of this resolution needs a workspace of \d+ bytes, the budget is 1 \(raise it, or render with JPT_KERNEL_REFERENCE_LAYOUT, which needs none\)"
ONE_FRAME = "temporal reprojection renders one frame per call"
NO_TEMPORAL = "jpt_set_temporal_params not called"
OTHER_SIZE = "temporal RenderParameters width/height differ from jpt_set_params"
WHOLE_IMAGE = "temporal reprojection needs the whole image in one context (world == 1)"
REFITTED = "jpt_scene_refit_tlas refits the default kernel's records only: call jpt_scene_update_tlas before rendering with another kernel"
DEFORMED = "jpt_scene_update_mesh refits the default kernel's records only: call jpt_scene_commit before rendering with another kernel"


def temporal_params(w=W, h=H):
    p = np.zeros((), dtype=wire.TEMPORAL_PARAMS)
    p["deltaMatrix"] = np.eye(4, dtype=np.float32).reshape(-1)
    p["width"], p["height"], p["frame_count"] = w, h, 1
    p["blendFactor"], p["nearPlane"], p["farPlane"] = 0.75, 0.01, 1000.0
    return p


def context(device=0, scene=True, params=True, camera=True, builder=capi.BUILD_SAH):
    ctx = host.Context(device)
    try:
        if scene:
            ctx.build_scene(SCENE, builder)
        if params:
            ctx.set_params(W, H, 1, capi.ACCUM_REF_LDR8)
        if camera:
            ctx.set_camera(CAMERA)
    except Exception:
        ctx.close()
        raise
    return ctx


def render(ctx, entry, n_frames=1, first=1):
    """-> (return code, the whole text the context holds) after one call of the entry point"""
    rc = getattr(ctx._lib, entry)(ctx.h, n_frames, first)
    return rc, ctx.last_error()


def refused(ctx, want, n_frames=1, entries=ENTRIES):
    for entry in entries:
        assert render(ctx, entry, n_frames) == want, entry


def renders(ctx, n_frames=1, entries=ENTRIES):
    for entry in entries:
        assert render(ctx, entry, n_frames)[0] == OK, (entry, ctx.last_error())
    ctx.sync()


@pytest.fixture
def ctx_of():
    made = []

    def make(**kw):
        made.append(context(**kw))
        return made[-1]
    yield make
    for ctx in made:
        ctx.close()


def test_the_host_only_refusal_comes_first(hiplib):
    """a host-only context holds a scene and nothing else: its own sentence, before the missing params, camera and the frame count"""
    ctx = context(device=-1, params=False, camera=False)
    try:
        refused(ctx, (E_DEVICE, HOST_ONLY), n_frames=-1)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_what_is_missing_is_named_in_order(hiplib, ctx_of):
    """rows 1 to 4: each context lacks everything after the named step as well, and the frame count is bad throughout"""
    refused(ctx_of(scene=False, params=False, camera=False), (E_STATE, NO_SCENE), n_frames=-1)
    refused(ctx_of(params=False, camera=False), (E_STATE, NO_PARAMS), n_frames=-1)
    refused(ctx_of(camera=False), (E_STATE, NO_CAMERA), n_frames=-1)
    refused(ctx_of(), (E_INVALID, NEGATIVE), n_frames=-1)


@pytest.mark.gpu
def test_no_frames_is_no_render(hiplib, ctx_of):
    """row 5: n_frames = 0 succeeds and leaves the frame count and the sum bit for bit what they were"""
    ctx = ctx_of()
    ctx.render(2, 1)
    frames, accum = ctx.stats()["frames"], ctx.read_accum()
    assert frames == 2 and accum[..., :3].max() > 0
    for entry in ENTRIES:
        assert render(ctx, entry, 0, 3)[0] == OK, entry
        ctx.sync()
        assert ctx.stats()["frames"] == frames and ctx.read_accum().tobytes() == accum.tobytes(), entry


@pytest.mark.gpu
def test_a_workspace_budget_is_a_cap(hiplib, ctx_of):
    """rows 6 and 7: a budget of one byte refuses every entry point of the default kernel; the reference-layout kernel needs no workspace"""
    ctx = ctx_of()
    ctx.set_memory_policy(0, 1)
    for entry in ENTRIES:
        rc, text = render(ctx, entry)
        assert rc == E_LIMIT and re.fullmatch(BUDGET, text), (entry, rc, text)
    assert ctx.workspace_bytes() == 0 and ctx.stats()["frames"] == 0
    ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
    renders(ctx)
    assert ctx.stats()["frames"] == len(ENTRIES) and ctx.workspace_bytes() == 0


@pytest.mark.gpu
def test_the_temporal_pass_refuses_in_its_order(hiplib, ctx_of):
    """rows 8 to 11: two frames; a partition; no RenderParameters; RenderParameters of another width -- each context lacks what the
    later checks ask for as well, until the last"""
    ctx = ctx_of()
    ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
    ctx.set_partition(0, 2)
    refused(ctx, (E_INVALID, ONE_FRAME), n_frames=2)
    refused(ctx, (E_STATE, WHOLE_IMAGE))
    ctx.set_partition(0, 1)
    refused(ctx, (E_STATE, NO_TEMPORAL))
    ctx.set_temporal_params(temporal_params(w=W + 1))
    refused(ctx, (E_INVALID, OTHER_SIZE))
    ctx.set_temporal_params(temporal_params())
    ctx.set_partition(0, 2)
    refused(ctx, (E_STATE, WHOLE_IMAGE))
    ctx.set_partition(0, 1)
    renders(ctx, entries=("jpt_render",))
    assert ctx.stats()["frames"] == 1


@pytest.mark.gpu
def test_a_refitted_instance_level_is_the_default_kernels(hiplib, ctx_of):
    """rows 12, 13 and 15: after jpt_scene_refit_tlas the reference-layout kernel and DEBUG_STEPS are refused in the same words, until
    jpt_scene_update_tlas"""
    ctx = ctx_of()
    ctx.refit_tlas(T12)
    renders(ctx, entries=("jpt_render",))
    ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
    refused(ctx, (E_STATE, REFITTED))
    ctx.set_kernel(capi.KERNEL_WAVEFRONT)
    ctx.set_debug_steps(True)
    refused(ctx, (E_STATE, REFITTED))
    ctx.update_tlas()
    renders(ctx, entries=("jpt_render",))
    ctx.set_debug_steps(False)
    ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
    renders(ctx, entries=("jpt_render",))


@pytest.mark.gpu
def test_a_deformed_mesh_is_the_default_kernels(hiplib, ctx_of):
    """rows 14 and 15: after jpt_scene_update_mesh the reference-layout kernel and DEBUG_STEPS are refused, until a fresh commit"""
    ctx = ctx_of(builder=capi.BUILD_SAH_WATERTIGHT)
    ctx.update_mesh(0, SCENE.meshes[0])
    renders(ctx, entries=("jpt_render",))
    ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
    refused(ctx, (E_STATE, DEFORMED))
    ctx.set_kernel(capi.KERNEL_WAVEFRONT)
    ctx.set_debug_steps(True)
    refused(ctx, (E_STATE, DEFORMED))
    ctx.set_debug_steps(False)
    ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
    ctx.build_scene(SCENE, capi.BUILD_SAH_WATERTIGHT)
    renders(ctx, entries=("jpt_render",))
