"""The tracing launches keep a wave's bookkeeping in scalar lane masks (walk_round_masked, trace_queue: jpt_kernels_wf2.hip) and
restore the world ray's slab constants only where a lane leaves an instance into a TLAS record (pop_next<true>, jpt_trace_core.h).
Neither changes a ray's steps, so every render here equals the CPU oracle's pixel for pixel, in the accumulation and in rgba8, on
the native tree (four-child records: the form those kernels run in)."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

pytestmark = pytest.mark.gpu

MODES = [wire.ACCUM_REF_LDR8, wire.ACCUM_HDR_F32]


def _context(sc, cam, w, h, bounces, mode):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, bounces, mode)
    ctx.set_camera(cam)
    return ctx


def _check(sc, w, h, frames, bounces, mode, oracle):
    cam = scenes.camera_block(sc.camera, w, h)
    want, want_ldr, _, _, _ = oracle.render(oracle.build_scene(sc), cam, w, h, bounces, frames, 1, mode)
    ctx = _context(sc, cam, w, h, bounces, mode)
    try:
        ctx.render(frames, 1)
        got, got_ldr = ctx.read_accum(), ctx.read_ldr()
    finally:
        ctx.close()
    print(sc.name, (w, h, frames, bounces, mode), "differing pixels: accumulation", int((got != want).any(axis=-1).sum()),
          "rgba8", int((got_ldr != want_ldr).any(axis=-1).sum()))
    assert np.array_equal(got, want)
    assert np.array_equal(got_ldr, want_ldr)


@pytest.fixture(scope="module")
def many_instances():
    """18 instances: the instance level has several records, so a lane leaves an instance into a TLAS record"""
    return scenes.instanced_scene(n_side=4, n_unique=2, tris_per_mesh=96)


@pytest.mark.parametrize("mode", MODES)
def test_leaving_an_instance_into_a_tlas_record(oracle, hiplib, many_instances, mode):
    assert len(many_instances.instances) >= 5
    _check(many_instances, 64, 64, 2, 3, mode, oracle)


@pytest.mark.parametrize("mode", MODES)
def test_one_partly_filled_draining_wave(oracle, hiplib, mode):
    """64 paths: one wave, whose rays thin out bounce by bounce -- the caps of the phase thresholds, a lane mask with few bits"""
    _check(scenes.cornell_scene(), 8, 8, 1, 4, mode, oracle)


@pytest.mark.parametrize("mode", MODES)
def test_a_frame_count_that_divides_nothing(oracle, hiplib, mode):
    """3 frames: 64 / n_frames is not whole, and the last chunk of path ids is short"""
    _check(scenes.cornell_scene(), 40, 24, 3, 3, mode, oracle)


@pytest.mark.parametrize("mode", MODES)
def test_queued_renders_equal_a_blocking_one(oracle, hiplib, many_instances, mode):
    sc, w, h, frames, bounces = many_instances, 64, 64, 2, 3
    cam = scenes.camera_block(sc.camera, w, h)
    want, want_ldr, _, _, _ = oracle.render(oracle.build_scene(sc), cam, w, h, bounces, frames, 1, mode)
    images = []
    for queued in (True, False):
        ctx = _context(sc, cam, w, h, bounces, mode)
        try:
            for _ in range(3 if queued else 1):
                ctx.accum_reset()
                ctx.render(frames, 1, asynchronous=queued)
            ctx.sync()
            images.append((ctx.read_accum(), ctx.read_ldr()))
        finally:
            ctx.close()
    assert np.array_equal(images[0][0], images[1][0]) and np.array_equal(images[0][1], images[1][1])
    assert np.array_equal(images[1][0], want) and np.array_equal(images[1][1], want_ldr)
