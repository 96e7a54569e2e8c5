"""Directional lightmaps on the device (jpt_set_bake_directional): the moment planes of bake renders against the numpy restatement
(tests/np_bake_dir.py) bit for bit -- whole paths from numpy, longer and continued renders, queued renders and frame groups from the
frames the device's own one-frame renders give --, what the switch leaves untouched, ranks, the finished planes against
tests/np_lightmap.py, and the refusals.  32 x 32 or 33 x 17 texels, 4 bounces."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, partition

import np_bake as nb
import np_bake_dir as nbd
import np_lightmap as nl
from test_bake_host import SIZES, atlas, same_bits
from test_gpu_bake import atlas_want, bake_ctx   # noqa: F401  (atlas_want: the module's fixture of numpy frames, shared)
from test_gpu_transmission import np_sum

pytestmark = pytest.mark.gpu

F = np.float32
E_STATE = -4   # JPT_E_STATE
ACCUMS = (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def differing(got, want):
    """a message naming the first texels whose bits differ, or None"""
    bad = np.argwhere(~((_bits(np.ascontiguousarray(got, F)) == _bits(np.ascontiguousarray(want, F))) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    k = tuple(bad[0])
    return "%d values differ, first %s: %r vs %r" % (len(bad), bad[:3].tolist(), got[k], want[k])


def dir_ctx(scene, p4, n4, **kw):
    """test_gpu_bake.bake_ctx with the switch on"""
    ctx = bake_ctx(scene, p4, n4, **kw)
    try:
        ctx.set_bake_directional(True)
    except Exception:
        ctx.close()
        raise
    return ctx


def device_frames(scene, p4, n4, accum, lighting, n, first=1):
    """the values of frames first .. first + n - 1 as the accumulation adds them, read from one-frame renders after a reset with the
    switch off: the render path that exists without this feature.  [n, H, W, 3]"""
    ctx = bake_ctx(scene, p4, n4, accum=accum, lighting=lighting)
    try:
        out = []
        for f in range(n):
            ctx.accum_reset()
            ctx.render(1, first + f)
            out.append(ctx.read_accum()[..., :3].copy())
        return np.stack(out)
    finally:
        ctx.close()


# ---- 1. whole paths from numpy: no device value in the expectation ----------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT])
@pytest.mark.parametrize("size", SIZES)
def test_the_planes_equal_numpy(hiplib, atlas_want, size, builder):
    """two frames through np_bake.trace_frame under the sky and under sun_map() (np_bake restates the map's BRDF mode; the MIS mode's
    frames come from the device in the tests below)"""
    sc, p4, n4, sky, _, env = atlas_want[size]
    valid = nb.texel_valid(n4)
    for accum in ACCUMS:
        ldr8 = accum == capi.ACCUM_REF_LDR8
        for lighting, frames in (("sky", sky), ("map", env)):
            want = nbd.moments(p4, n4, frames, 1, ldr8)
            ctx = dir_ctx(sc, p4, n4, builder=builder, accum=accum, lighting=lighting)
            try:
                ctx.render(2, 1)
                got, acc = ctx.read_bake_directional(), ctx.read_accum()[..., :3]
                ptr, nbytes = ctx.device_bake_directional()
            finally:
                ctx.close()
            assert got.shape == (3,) + n4.shape and ptr and nbytes == got.nbytes
            why = differing(got, want)
            assert why is None, "accum %d %s builder %d: %s" % (accum, lighting, builder, why)
            assert differing(acc, np_sum(frames, ldr8)) is None
            assert (_bits(got[:, ~valid]) == 0).all() and (_bits(got[..., 3]) == 0).all()
            assert (got[:, valid][..., :3] > 0).any() and (got[:, valid][..., :3] < 0).any()


# ---- 2. longer and continued renders, blocking and queued ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames16(hiplib):
    """(accum, lighting) -> (scene, p4, n4, the values of frames 1 .. 16 at 33 x 17 from the device's one-frame renders)"""
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)
    return {(accum, lighting): (sc, p4, n4, device_frames(sc, p4, n4, accum, lighting, 16)) for accum in ACCUMS for lighting in ("sky", "map_mis")}


@pytest.mark.parametrize("lighting", ["sky", "map_mis"])
@pytest.mark.parametrize("accum", ACCUMS)
def test_longer_and_continued_renders(hiplib, frames16, accum, lighting):
    """3 frames (the per-frame loop), 4 and 8 (the 16-byte loads), each continued by a second render; then the same frames as queued
    renders in a row (the slots' route)"""
    sc, p4, n4, fr = frames16[accum, lighting]
    ldr8 = accum == capi.ACCUM_REF_LDR8
    ctx = dir_ctx(sc, p4, n4, accum=accum, lighting=lighting)
    try:
        for n, more in ((3, 3), (4, 4), (8, 3)):
            ctx.accum_reset()
            ctx.render(n, 1)
            first = nbd.moments(p4, n4, fr[:n], 1, ldr8)
            why = differing(ctx.read_bake_directional(), first)
            assert why is None, "%d frames: %s" % (n, why)
            ctx.render(more, 1 + n)
            both = nbd.moments(p4, n4, fr[n:n + more], 1 + n, ldr8, frame_count=n + 1, prev=first)
            why = differing(ctx.read_bake_directional(), both)
            assert why is None, "%d + %d frames: %s" % (n, more, why)
            assert differing(ctx.read_accum()[..., :3], np_sum(list(fr[:n + more]), ldr8)) is None
        # queued: four renders in a row without a sync between them
        ctx.accum_reset()
        want, at = None, 0
        for n in (4, 3, 8, 1):
            ctx.render(n, 1 + at, asynchronous=True)
            want = nbd.moments(p4, n4, fr[at:at + n], 1 + at, ldr8, frame_count=at + 1, prev=want)
            at += n
        why = differing(ctx.read_bake_directional(), want)
        assert why is None, "queued: %s" % why
        assert differing(ctx.read_accum()[..., :3], np_sum(list(fr[:16]), ldr8)) is None
    finally:
        ctx.close()


# ---- 3. frame groups ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accum", ACCUMS)
def test_five_frames_in_one_render(hiplib, accum):
    """5 frames in one blocking render, continued by 5 more: under JPT_GROUPS=3 / 2 (the parent test below) the groups are of unequal
    size and every group's values live in a block of their own, which the kernel must find as wf2_accumulate does"""
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)
    ldr8 = accum == capi.ACCUM_REF_LDR8
    fr = device_frames(sc, p4, n4, accum, "sky", 10)
    ctx = dir_ctx(sc, p4, n4, accum=accum)
    try:
        ctx.render(5, 1)
        first = nbd.moments(p4, n4, fr[:5], 1, ldr8)
        why = differing(ctx.read_bake_directional(), first)
        assert why is None, why
        ctx.render(5, 6)
        why = differing(ctx.read_bake_directional(), nbd.moments(p4, n4, fr[5:], 6, ldr8, frame_count=6, prev=first))
        assert why is None, why
        ctx.accum_reset()
        ctx.render(5, 1, asynchronous=True)
        ctx.render(5, 6, asynchronous=True)
        assert differing(ctx.read_bake_directional(), nbd.moments(p4, n4, fr[5:], 6, ldr8, frame_count=6, prev=first)) is None
    finally:
        ctx.close()


@pytest.mark.parametrize("switch", ["JPT_GROUPS=3", "JPT_GROUPS=2 JPT_PIPE_SLOTS=2"])
def test_frame_groups_give_the_same_planes(hiplib, switch):
    """the switches are read once per process (test_gpu_full.test_alternative_tracing_launches_are_bit_identical): a child process"""
    env = dict(os.environ)
    for kv in switch.split():
        k, v = kv.split("=")
        env[k] = v
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_five_frames_in_one_render"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accum", ACCUMS)
def test_the_switch_leaves_every_other_image_alone(hiplib, accum):
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)

    def run(on):
        ctx = bake_ctx(sc, p4, n4, accum=accum)
        try:
            if on:
                ctx.set_bake_directional(True)
            ctx.render(2, 1)
            ctx.render(3, 3, asynchronous=True)
            ctx.render(4, 6, asynchronous=True)
            out = ctx.read_accum(), ctx.read_ldr(), ctx.read_depth(), ctx.workspace_bytes()
            if not on:
                planes = np.zeros((3, h, w, 4), F)
                assert ctx._lib.jpt_read_bake_directional_f32(ctx.h, host._ptr(planes)) == E_STATE
                msg = ctx._lib.jpt_last_error(ctx.h)
                assert b"jpt_read_bake_directional_f32" in msg and b"switched off" in msg, msg
                assert ctx.device_bake_directional() == (None, 0)
            else:
                assert (ctx.read_bake_directional()[..., :3] != 0).any()
            return out
        finally:
            ctx.close()
    off, on = run(False), run(True)
    for a, b in zip(off[:3], on[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert off[3] == on[3]


def test_the_switch_resets_the_accumulation_and_ignores_camera_renders(hiplib):
    w, h = 32, 32
    sc, p4, n4 = atlas(w, h)
    ctx = bake_ctx(sc, p4, n4)
    try:
        ctx.render(2, 1)
        assert ctx.stats()["frames"] == 2
        ctx.set_bake_directional(False)          # no change of the value: nothing happens
        assert ctx.stats()["frames"] == 2
        ctx.set_bake_directional(True)
        assert ctx.stats()["frames"] == 0
        ctx.render(1, 1)
        one = ctx.read_bake_directional()
        ctx.set_bake_directional(True)           # again no change
        assert ctx.stats()["frames"] == 1 and same_bits(ctx.read_bake_directional(), one)
        # without bake images the switch has no effect: a camera render, on either kernel, as with the switch off
        ctx.set_bake_texels(None, None)
        ctx.accum_reset()
        ctx.render(2, 1)
        with_switch = ctx.read_accum()
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        ctx.accum_reset()
        ctx.render(2, 1)
        ctx.set_kernel(capi.KERNEL_WAVEFRONT)
        ctx.set_bake_directional(False)
        ctx.render(2, 1)
        assert np.array_equal(_bits(ctx.read_accum()), _bits(with_switch))
    finally:
        ctx.close()


# ---- 5. ranks ---------------------------------------------------------------------------------------------------------------------------------------

def test_two_partitions_equal_one_context(hiplib):
    w, h = 33, 17    # (three 8-row strips, the last one short)
    sc, p4, n4 = atlas(w, h)
    one = dir_ctx(sc, p4, n4, accum=capi.ACCUM_REF_LDR8)
    try:
        one.render(4, 1)
        one.render(3, 5)
        want = one.read_bake_directional()
    finally:
        one.close()
    got = np.zeros_like(want)
    seen = np.zeros(h, bool)
    for r in range(2):
        part = dir_ctx(sc, p4, n4, accum=capi.ACCUM_REF_LDR8, rank=r, world=2)
        try:
            part.render(4, 1)
            part.render(3, 5)
            rows = partition.rows_of_rank(h, r, 2)
            planes = part.read_bake_directional()
            assert planes.shape == (3, len(rows), w, 4)
            got[:, rows] = planes
            seen[rows] = True
        finally:
            part.close()
    assert seen.all() and np.array_equal(_bits(got), _bits(want))


# ---- 6. the finished planes -----------------------------------------------------------------------------------------------------------------------

def test_the_finished_planes_equal_the_lightmap_filter_of_each_plane(hiplib):
    w, h = 33, 17
    sc, p4, n4 = atlas(w, h)
    ctx = dir_ctx(sc, p4, n4)
    other = dict(passes=2, normal_power_log2=1, dilate=3, sigma_distance=2.0, sigma_plane=0.5, sigma_color=0.75)
    try:
        ctx.render(3, 1)
        planes, accum = ctx.read_bake_directional(), ctx.read_accum()
        ctx.bake_finish()
        ctx.bake_finish_directional()
        l0, got = ctx.read_lightmap(), ctx.read_lightmap_directional()
        ptr, nbytes = ctx.device_bake_directional(finished=True)
        assert ptr and nbytes == got.nbytes and got.shape == (3, h, w, 4)
        with np.errstate(all="ignore"):
            means = (planes / F(3.0)).astype(F)
            assert nl.same_bits(l0, nl.finish((accum / F(3.0)).astype(F), p4, n4)).all()      # the L0 map is what it was
        for k in range(3):
            bad = ~nl.same_bits(got[k], nl.finish(means[k], p4, n4))
            assert not bad.any(), "plane %d: %d values differ, first %s" % (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            # coverage: the charts 1, the dilated ring 0.5 exactly where jpt_bake_finish puts it, the rest 0 with colour 0
            assert np.array_equal(got[k][..., 3], l0[..., 3])
            assert (got[k][..., 3] == 0.5).any() and (got[k][..., 3] == 0).any()
            assert (got[k][got[k][..., 3] == 0] == 0).all()
        assert (got[..., :3] < 0).any()                                                        # signed colours go through the filter
        valid = nb.texel_valid(n4)
        assert not np.array_equal(got[0][valid][:, :3], means[0][valid][:, :3])              # ... which is not the identity
        ctx.set_bake_finish_params(**other)
        assert nl.same_bits(ctx.read_lightmap_directional()[1], nl.finish(means[1], p4, n4)).all()   # parameters take effect at the next call
        ctx.bake_finish_directional()
        got2 = ctx.read_lightmap_directional()
        for k in range(3):
            assert nl.same_bits(got2[k], nl.finish(means[k], p4, n4, **other)).all(), k
        assert not nl.same_bits(got2, got).all()
        assert same_bits(ctx.read_bake_directional(), planes) and nl.same_bits(ctx.read_lightmap(), l0).all()   # nothing else was written
    finally:
        ctx.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_what_is_refused_and_why(hiplib):
    w, h = 32, 32
    sc, p4, n4 = atlas(w, h)
    ctx = bake_ctx(sc, p4, n4)
    L = ctx._lib
    out = np.zeros((3, h, w, 4), F)

    def refused(rc, *words):
        assert rc == E_STATE, rc
        msg = L.jpt_last_error(ctx.h)
        for word in words:
            assert word in msg, msg

    def render_refused(*words):
        refused(L.jpt_render(ctx.h, 1, 1), b"jpt_set_bake_directional", *words)
        refused(L.jpt_render_async(ctx.h, 1, 1), b"jpt_set_bake_directional", *words)
    try:
        # the switch off: no planes to read or to finish
        ctx.render(1, 1)
        refused(L.jpt_bake_finish_directional(ctx.h), b"jpt_bake_finish_directional", b"switched off")
        refused(L.jpt_read_bake_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_bake_directional_f32", b"switched off")
        refused(L.jpt_read_lightmap_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_directional_f32")
        ctx.set_bake_directional(True)
        # finish and read before a render
        refused(L.jpt_bake_finish_directional(ctx.h), b"jpt_bake_finish_directional", b"no frame")
        refused(L.jpt_read_bake_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_bake_directional_f32", b"no bake render")
        # the renders it refuses
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT)
        render_refused(b"reference-layout")
        ctx.set_kernel(capi.KERNEL_WAVEFRONT)
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        render_refused(b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_NONE)
        render_refused(b"JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        render_refused(b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.render(2, 1)
        ctx.read_bake_directional()
        refused(L.jpt_read_lightmap_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_directional_f32", b"no jpt_bake_finish_directional")
        ctx.bake_finish_directional()
        ctx.read_lightmap_directional()
        # jpt_bake_finish's own refusals
        ctx.set_debug_steps(True)
        refused(L.jpt_bake_finish_directional(ctx.h), b"jpt_bake_finish_directional", b"DEBUG_STEPS")
        ctx.set_debug_steps(False)
        # new images: what was finished from the old ones is gone, the raw planes follow the images
        ctx.set_bake_texels(p4[::-1].copy(), n4[::-1].copy())
        refused(L.jpt_read_lightmap_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_lightmap_directional_f32")
        # the images dropped: the planes go with them
        ctx.set_bake_texels(None, None)
        refused(L.jpt_read_bake_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_bake_directional_f32", b"no bake images")
        refused(L.jpt_bake_finish_directional(ctx.h), b"jpt_bake_finish_directional", b"no bake images")
        assert ctx.device_bake_directional() == (None, 0)
        ctx.set_bake_texels(p4, n4)
        refused(L.jpt_read_bake_directional_f32(ctx.h, host._ptr(out)), b"jpt_read_bake_directional_f32", b"no bake render")
        ctx.accum_reset()
        ctx.render(1, 1)
        assert (ctx.read_bake_directional()[..., :3] != 0).any()
    finally:
        ctx.close()
