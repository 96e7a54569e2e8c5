"""Reflection probes on the host (jpt_set_reflection_probes, jpt_reflection_prefilter; CPU): the host's copy of the cube ray, of the
sample table and of the prefilter's pinned sum against tests/np_reflection.py, what the two maps and the filter must do whatever the
mirror says, and the argument checks that need no device.  Faces of 4, 8 and 16 texels; three probes, two to a row, so the fourth strip
has no probe."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_reflection as nrf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # JPT_E_*
N_PROBES, PER_ROW = 3, 2
POSITIONS = np.array([(0.0, 0.0, 0.0), (1.5, -0.25, 2.0), (-3.0, 0.5, 0.75)], F)
# (face size, levels, samples, probes, probes per row): the smallest chain; one empty strip; a table longer than a wave
PREFILTER_CASES = ((4, 3, 8, 1, 1), (8, 4, 16, 3, 2), (16, 5, 96, 1, 1))


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((_u32(a) == _u32(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def accum_image(s, n, per_row, frames, seed=11, specials=True):
    """a random positive accumulation of `frames` frames for n probes, zeros in the strips without a probe; with `specials` one NaN
    and one inf texel (in two probes when there are two)"""
    rng = np.random.default_rng(seed + s)
    w, h = nrf.image_size(n, s, per_row)
    a = (rng.uniform(0.0, 4.0, (h, w, 4)) * frames).astype(F)
    a[..., 3] = 1.0
    for p in range(n, -(-n // per_row) * per_row):
        a[(p // per_row) * s:(p // per_row + 1) * s, (p % per_row) * 6 * s:(p % per_row + 1) * 6 * s] = 0.0
    if specials:
        a[1, 2, 0] = np.nan
        a[s - 1, 6 * s * min(per_row, n) - 2, 1] = np.inf
    return a


# ---- 1. the cube ray ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", (4, 8))
def test_host_cube_rays_equal_numpy_and_point_out_of_their_faces(s):
    w, h = nrf.image_size(N_PROBES, s, PER_ROW)
    assert (w, h) == host.reflection_image_size(N_PROBES, s, PER_ROW) == (12 * s, 2 * s)
    p, f, ci, cj, ok = nrf.pixel_cells(N_PROBES, s, PER_ROW)
    for frame in (0, 7):
        rays = host.debug_cube_rays(HOST_ONLY, POSITIONS, s, PER_ROW, frame)
        assert rays.shape == (h, w, 6)
        o, d = rays.reshape(-1, 6)[:, :3], rays.reshape(-1, 6)[:, 3:]
        _, wo, wd, wv = nrf.cube_rays(POSITIONS, s, PER_ROW, frame)
        assert np.array_equal(wv, ok) and not wv.all()
        assert same_bits(o, wo) and same_bits(d, wd), frame
        # the strip past the last probe is all zeros, and only it
        assert not rays[s:, 6 * s:].any() and d.reshape(h, w, 3)[:s].any(axis=-1).all() and d.reshape(h, w, 3)[s:, :6 * s].any(axis=-1).all()
        assert same_bits(o[ok], POSITIONS[p[ok]])                                  # the origin is the probe, no offset
        # independent of the mirror: the major axis of a direction of face f is axis f // 2, its sign + for even f, and |d| = 1
        dd = d[ok].astype(np.float64)
        axis = np.argmax(np.abs(dd), axis=1)
        assert np.array_equal(axis, f[ok] // 2), frame
        major = dd[np.arange(len(dd)), axis]
        assert np.array_equal(major > 0, f[ok] % 2 == 0), frame
        assert np.abs(np.sqrt((dd * dd).sum(axis=1)) - 1.0).max() <= 2 * 2.0 ** -23  # 2 ulp at 1
    a = host.debug_cube_rays(HOST_ONLY, POSITIONS, s, PER_ROW, 1)
    b = host.debug_cube_rays(HOST_ONLY, POSITIONS, s, PER_ROW, 2)
    assert not np.array_equal(a, b)
    assert nrf.HASH == (0x1f83d9ab, 0x5be0cd19) and set(nrf.HASH).isdisjoint({0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c})


# ---- 2. the two maps agree ------------------------------------------------------------------------------------------------------------------

def test_looking_up_a_texels_own_direction_returns_the_texel():
    """for every texel of every level of S = 16: the lookup of the texel's centre direction N is that face and that texel -- a face table
    that capture and lookup disagree on fails here; and the library's own capture directions land in their own texels"""
    for level in range(5):
        s = 16 >> level
        f, j, i = np.meshgrid(np.arange(6), np.arange(s), np.arange(s), indexing="ij")
        face, si, ti = nrf.lookup(nrf.texel_normals(s), s)
        assert np.array_equal(face, f) and np.array_equal(si, i) and np.array_equal(ti, j), level
    p, f, ci, cj, ok = nrf.pixel_cells(1, 16, 1)
    for frame in (0, 7):
        d = host.debug_cube_rays(HOST_ONLY, POSITIONS[:1], 16, 1, frame).reshape(-1, 6)[:, 3:]
        face, si, ti = nrf.lookup(d, 16)
        assert np.array_equal(face, f) and np.array_equal(si, ci) and np.array_equal(ti, cj), frame


# ---- 3. the table --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((16, 5, 96), (8, 4, 16), (64, 7, 256), (4, 2, 8)))
def test_the_sample_table_is_the_float64_construction(shape):
    s, n_levels, K = shape
    top = nrf.log2i(s)
    for level in range(1, n_levels):
        got, lvl = host.debug_reflection_samples(s, n_levels, K, level)
        Lw, w, expr, kept = nrf.sample_table64(s, n_levels, K, level)
        # no sample of these shapes stands within 1e-9 of a level boundary: the comparison of the levels below excludes nothing
        assert (np.abs(expr - np.round(expr)) > 1e-9).all(), (shape, level)
        assert len(got) == int(kept.sum()) == len(lvl)
        want = np.concatenate([Lw[kept], w[kept, None]], axis=1)
        ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        print("table S %d levels %d K %d level %d: kept %d, worst error %.3g ulp" % (s, n_levels, K, level, len(got), float((err / ulp).max())))
        assert (err <= ulp).all(), float((err / ulp).max())
        assert np.array_equal(lvl, np.clip(np.floor(expr[kept]) + 1, 0, top).astype(np.uint8))
        assert abs(float(got[:, 3].astype(np.float64).sum()) - 1.0) <= K * 2.0 ** -24
        assert (got[:, 2] > 0).all() and (got[:, 3] > 0).all()
        if level == n_levels - 1:                                              # r = 1: half the lobe points below the horizon
            assert len(got) < K, len(got)
    # the library's default: every level down to 1 x 1
    a = host.debug_reflection_samples(s, 0, K, 1)
    b = host.debug_reflection_samples(s, top + 1, K, 1)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 4. the prefilter, bit for bit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PREFILTER_CASES)
def test_host_prefilter_equals_numpy_bit_for_bit(case):
    s, n_levels, K, n, per_row = case
    for frames in (1, 3):
        a = accum_image(s, n, per_row, frames)
        for level in range(n_levels):
            got = host.debug_reflection_prefilter(HOST_ONLY, a, frames, n, s, per_row, level, n_levels=n_levels, samples=K)
            table, lvl = host.debug_reflection_samples(s, n_levels, K, level) if level else (None, None)
            want = nrf.prefilter(a, frames, n, s, per_row, n_levels, level, table, lvl)
            assert got.shape == (n, 6, s >> level, s >> level, 4) and same_bits(got, want), (frames, level)
            assert (got[..., 3] == 1).all()
        assert np.isnan(got).any() or np.isinf(got).any()                          # the NaN and the inf reach the last level
    # the probes are apart: another probe's strip does not leak in
    if n > 1:
        a2 = accum_image(s, n, per_row, 1, specials=False)
        want = host.debug_reflection_prefilter(HOST_ONLY, a2, 1, n, s, per_row, 2, n_levels=n_levels, samples=K)
        a2[:s, :6 * s] *= F(2.0)
        got = host.debug_reflection_prefilter(HOST_ONLY, a2, 1, n, s, per_row, 2, n_levels=n_levels, samples=K)
        assert not same_bits(got[0], want[0]) and same_bits(got[1:], want[1:])


# ---- 5. a constant cube -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PREFILTER_CASES)
def test_a_constant_cube_stays_constant(case):
    """every texel c per channel: the source levels are exactly c (sums of equal numbers and a power of two), and an output texel is
    sum_k c w_k -- each weight rounded once (2^-24 relative each, K of them), each product once, each of the K adds once: within
    (2 K + 2) 2^-24 relative of c"""
    s, n_levels, K, n, per_row = case
    colour = np.array([0.375, 1.7, 0.013], F)
    w, h = nrf.image_size(n, s, per_row)
    a = np.zeros((h, w, 4), F)
    a[..., :3] = colour * F(2.0)
    for level in nrf.source_chain(a, 2, n, s, per_row):
        assert (level == colour).all()
    bound = (2 * K + 2) * 2.0 ** -24
    for level in range(n_levels):
        got = host.debug_reflection_prefilter(HOST_ONLY, a, 2, n, s, per_row, level, n_levels=n_levels, samples=K)[..., :3].astype(np.float64)
        rel = np.abs(got / colour.astype(np.float64) - 1.0).max()
        print("S %d level %d K %d: off by %.3g relative, bound %.3g" % (s, level, K, rel, bound))
        assert rel <= bound and (level > 0 or rel == 0.0)


# ---- 6. concentration -------------------------------------------------------------------------------------------------------------------------

def test_one_bright_texel_spreads_with_the_level():
    s, n_levels, K = 16, 5, 64
    f, i, j = 4, 5, 9
    a = np.zeros((s, 6 * s, 4), F)
    a[j, f * s + i, :3] = 1000.0
    at, total = [], []
    for level in range(n_levels):
        got = host.debug_reflection_prefilter(HOST_ONLY, a, 1, 1, s, 1, level, n_levels=n_levels, samples=K)[0, ..., 0].astype(np.float64)
        assert (got >= 0).all()
        at.append(got[f, j >> level, i >> level])
        total.append(float((got * nrf.texel_solid_angles(s >> level)[None]).sum()))
    print("the texel at the bright direction, by level:", at, "-- the levels' integrals:", total)
    assert all(at[k + 1] < at[k] for k in range(n_levels - 1)), at
    assert all(t > 0 for t in total), total
    assert abs(nrf.texel_solid_angles(16).sum() * 6 - 4 * np.pi) < 1e-12


# ---- 8. the checks ------------------------------------------------------------------------------------------------------------------------------

def test_the_calls_check_their_arguments_on_a_host_only_context(L):
    for name in ("jpt_set_reflection_probes", "jpt_get_reflection_image_size", "jpt_read_reflection_probes", "jpt_set_reflection_params",
                 "jpt_reflection_prefilter", "jpt_get_reflection_chain_size", "jpt_read_reflection_f32", "jpt_get_reflection_timing",
                 "jpt_debug_cube_rays", "jpt_debug_reflection_samples", "jpt_debug_reflection_prefilter"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.jpt_abi_version() == 6
    pos = np.zeros((8, 3), F)
    ctx = host.Context(HOST_ONLY)
    try:
        def refused(rc, code, call, word=None):
            assert rc == code, (rc, code, call)
            msg = L.jpt_last_error(ctx.h)
            assert call.encode() in msg and (word is None or word.encode() in msg), msg
        S = lambda p, n, s, per: L.jpt_set_reflection_probes(ctx.h, None if p is None else p.ctypes.data, n, s, per)   # noqa: E731
        for s in (2, 3, 12, 48, 512, 0, -4):
            refused(S(pos, 8, s, 4), E_INVALID, "jpt_set_reflection_probes", "face_size")
        refused(S(pos, 0, 16, 4), E_LIMIT, "jpt_set_reflection_probes", "n_probes")
        refused(S(pos, -1, 16, 4), E_LIMIT, "jpt_set_reflection_probes", "n_probes")
        refused(S(pos, (1 << 20) + 1, 16, 4), E_LIMIT, "jpt_set_reflection_probes", "n_probes")
        refused(S(pos, 8, 16, 0), E_INVALID, "jpt_set_reflection_probes", "probes_per_row")
        refused(S(None, 8, 16, 4), E_INVALID, "jpt_set_reflection_probes", "NULL")
        big = np.zeros((1 << 20, 3), F)
        refused(S(big, 1 << 20, 4, 1024), E_LIMIT, "jpt_set_reflection_probes", "2^26")   # 2^20 strips of 96 pixels
        refused(S(big, 1 << 19, 4, 1024), E_DEVICE, "jpt_set_reflection_probes")          # 2^19 * 96 < 2^26: the checks pass
        refused(S(big, 171, 256, 1), E_LIMIT, "jpt_set_reflection_probes", "2^26")        # 171 * 6 * 2^16 > 2^26
        refused(S(big, 170, 256, 1), E_DEVICE, "jpt_set_reflection_probes")
        for bad in (np.nan, np.inf, -np.inf):
            q = pos.copy()
            q[5, 1] = bad
            refused(S(q, 8, 16, 4), E_INVALID, "jpt_set_reflection_probes", "probe 5")
        refused(S(pos, 8, 16, 4), E_DEVICE, "jpt_set_reflection_probes")                   # the checks passed: no device
        refused(S(pos, 8, 4, 3), E_DEVICE, "jpt_set_reflection_probes")
        refused(S(pos, 8, 256, 8), E_DEVICE, "jpt_set_reflection_probes")
        refused(S(None, 0, 0, 0), E_DEVICE, "jpt_set_reflection_probes")                   # (freeing)
        w, h = C.c_int32(0), C.c_int32(0)
        refused(L.jpt_get_reflection_image_size(ctx.h, None, C.byref(h)), E_INVALID, "jpt_get_reflection_image_size")
        refused(L.jpt_get_reflection_image_size(ctx.h, C.byref(w), C.byref(h)), E_DEVICE, "jpt_get_reflection_image_size")
        refused(L.jpt_read_reflection_probes(ctx.h, None), E_INVALID, "jpt_read_reflection_probes")
        refused(L.jpt_read_reflection_probes(ctx.h, pos.ctypes.data), E_DEVICE, "jpt_read_reflection_probes")
        # the parameters: the ranges, then the device
        P = lambda n_levels, samples: L.jpt_set_reflection_params(ctx.h, C.byref(capi.ReflectionParams(n_levels, samples)))   # noqa: E731
        for n_levels in (1, -1, 10):
            refused(P(n_levels, 64), E_INVALID, "jpt_set_reflection_params", "n_levels")
        for samples in (7, 0, 257, -8):
            refused(P(0, samples), E_INVALID, "jpt_set_reflection_params", "samples")
        refused(P(0, 64), E_DEVICE, "jpt_set_reflection_params")
        refused(P(9, 256), E_DEVICE, "jpt_set_reflection_params")
        refused(L.jpt_set_reflection_params(ctx.h, None), E_DEVICE, "jpt_set_reflection_params")
        # jpt_reflection_prefilter: the state errors that need no device, then the device
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        refused(L.jpt_reflection_prefilter(ctx.h), E_STATE, "jpt_reflection_prefilter", "JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_reflection_prefilter(ctx.h), E_STATE, "jpt_reflection_prefilter", "DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.set_partition(1, 2)
        refused(L.jpt_reflection_prefilter(ctx.h), E_STATE, "jpt_reflection_prefilter", "whole image on one context")
        ctx.set_partition(0, 1)
        refused(L.jpt_reflection_prefilter(ctx.h), E_DEVICE, "jpt_reflection_prefilter")
        out = np.zeros(6 * 4, F)
        s, off = C.c_int32(0), C.c_uint64(0)
        refused(L.jpt_get_reflection_chain_size(ctx.h, 0, None, C.byref(off)), E_INVALID, "jpt_get_reflection_chain_size")
        refused(L.jpt_get_reflection_chain_size(ctx.h, 0, C.byref(s), C.byref(off)), E_DEVICE, "jpt_get_reflection_chain_size")
        refused(L.jpt_read_reflection_f32(ctx.h, 0, None), E_INVALID, "jpt_read_reflection_f32")
        refused(L.jpt_read_reflection_f32(ctx.h, 0, out.ctypes.data), E_DEVICE, "jpt_read_reflection_f32")
        ms = C.c_float(0)
        refused(L.jpt_get_reflection_timing(ctx.h, None, C.byref(ms)), E_INVALID, "jpt_get_reflection_timing")
        refused(L.jpt_get_reflection_timing(ctx.h, C.byref(ms), C.byref(ms)), E_DEVICE, "jpt_get_reflection_timing")
        with pytest.raises(capi.JptError, match="face_size"):
            ctx.set_reflection_probes(pos, 6, 4)
        with pytest.raises(capi.JptError, match="jpt_reflection_prefilter"):
            ctx.reflection_prefilter()
        with pytest.raises(capi.JptError, match="samples"):
            ctx.set_reflection_params(samples=4)
    finally:
        ctx.close()
    assert L.jpt_set_reflection_probes(None, pos.ctypes.data, 8, 16, 4) == E_INVALID and L.jpt_reflection_prefilter(None) == E_INVALID
    assert L.jpt_read_reflection_f32(None, 0, pos.ctypes.data) == E_INVALID and L.jpt_read_reflection_probes(None, pos.ctypes.data) == E_INVALID
    assert L.jpt_get_reflection_image_size(None, None, None) == E_INVALID and L.jpt_set_reflection_params(None, None) == E_INVALID
    assert L.jpt_get_reflection_chain_size(None, 0, None, None) == E_INVALID and L.jpt_get_reflection_timing(None, None, None) == E_INVALID


def test_the_debug_calls_check_their_arguments(L):
    pos = np.zeros((2, 3), F)
    rays = np.zeros((4, 48, 6), F)
    R = L.jpt_debug_cube_rays
    assert R(HOST_ONLY, None, 2, 4, 2, 1, rays.ctypes.data) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 4, 2, 1, None) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 6, 2, 1, rays.ctypes.data) == E_INVALID
    assert b"jpt_debug_cube_rays" in L.jpt_debug_last_error() and b"face_size" in L.jpt_debug_last_error()
    assert R(HOST_ONLY, pos.ctypes.data, 0, 4, 2, 1, rays.ctypes.data) == E_LIMIT
    bad = pos.copy()
    bad[1, 2] = np.nan
    assert R(HOST_ONLY, bad.ctypes.data, 2, 4, 2, 1, rays.ctypes.data) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 4, 2, 1, rays.ctypes.data) == capi.OK and rays.any()
    t, lv = np.zeros((8, 4), F), np.zeros(8, np.uint8)
    T = L.jpt_debug_reflection_samples
    assert T(8, 4, 8, 1, None, lv.ctypes.data) == E_INVALID and T(8, 4, 8, 1, t.ctypes.data, None) == E_INVALID
    assert T(6, 3, 8, 1, t.ctypes.data, lv.ctypes.data) == E_INVALID and T(8, 5, 8, 1, t.ctypes.data, lv.ctypes.data) == E_INVALID
    assert b"n_levels" in L.jpt_debug_last_error()
    assert T(8, 1, 8, 1, t.ctypes.data, lv.ctypes.data) == E_INVALID and T(8, 4, 7, 1, t.ctypes.data, lv.ctypes.data) == E_INVALID
    assert T(8, 4, 8, 0, t.ctypes.data, lv.ctypes.data) == E_INVALID and T(8, 4, 8, 4, t.ctypes.data, lv.ctypes.data) == E_INVALID
    assert b"jpt_debug_reflection_samples" in L.jpt_debug_last_error() and b"level" in L.jpt_debug_last_error()
    assert T(8, 4, 8, 3, t.ctypes.data, lv.ctypes.data) == capi.OK and t.any() and (lv == 0xff).any()
    a, out = np.zeros((4, 48, 4), F), np.zeros((2, 6, 4, 4, 4), F)
    prm = capi.ReflectionParams(3, 8)
    J = L.jpt_debug_reflection_prefilter
    assert J(HOST_ONLY, None, 1, 2, 4, 2, C.byref(prm), 0, out.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, C.byref(prm), 0, None) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 0, 2, 4, 2, C.byref(prm), 0, out.ctypes.data) == E_INVALID
    assert b"frame_count" in L.jpt_debug_last_error()
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 5, 2, C.byref(prm), 0, out.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 0, 4, 2, C.byref(prm), 0, out.ctypes.data) == E_LIMIT
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, C.byref(capi.ReflectionParams(4, 8)), 0, out.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, C.byref(capi.ReflectionParams(3, 300)), 0, out.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, C.byref(prm), 3, out.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, C.byref(prm), 0, out.ctypes.data) == capi.OK
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 4, 2, None, 2, out.ctypes.data) == capi.OK       # the defaults: three levels, 64 samples
    with pytest.raises(capi.JptError, match="face_size"):
        host.debug_reflection_samples(12, 3, 8, 1)
    with pytest.raises(ValueError):
        host.debug_reflection_prefilter(HOST_ONLY, a[:2], 1, 2, 4, 2, 0)


def test_the_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for proto in (
            r"int jpt_set_reflection_probes\(jpt_ctx \*ctx, const float \*position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row\);",
            r"int jpt_get_reflection_image_size\(jpt_ctx \*ctx, int32_t \*width, int32_t \*height\);",
            r"int jpt_read_reflection_probes\(jpt_ctx \*ctx, float \*position3\);",
            r"typedef struct \{ int32_t n_levels; int32_t samples; \} jpt_reflection_params;",
            r"int jpt_set_reflection_params\(jpt_ctx \*ctx, const jpt_reflection_params \*params\);",
            r"int jpt_reflection_prefilter\(jpt_ctx \*ctx\);",
            r"int jpt_get_reflection_chain_size\(jpt_ctx \*ctx, int32_t level, int32_t \*face_size, uint64_t \*offset_texels\);",
            r"int jpt_read_reflection_f32\(jpt_ctx \*ctx, int32_t level, float \*out\);",
            r"int jpt_debug_cube_rays\(int device_id, const float \*position3, int32_t n_probes, int32_t face_size, int32_t probes_per_row,\s+uint32_t frame_index, float \*rays_out\);",
            r"int jpt_debug_reflection_samples\(int32_t face_size, int32_t n_levels, int32_t samples, int32_t level, float \*table_out, uint8_t \*src_level_out\);",
            r"int jpt_debug_reflection_prefilter\(int device_id, const float \*accum4, uint32_t frame_count, int32_t n_probes, int32_t face_size,\s+int32_t probes_per_row, const jpt_reflection_params \*params, int32_t level, float \*out\);"):
        assert re.search(proto, text), proto
    assert re.search(r"#define JPT_ABI_VERSION 6\b", text)
    assert "0x1f83d9ab, 0x5be0cd19" in text
    assert not hasattr(capi.lib(), "jpt_multi_reflection_prefilter")
    hpp = open(os.path.join(ROOT, "include", "jpt_host.hpp")).read()
    for name in ("set_reflection_probes", "reflection_image_size", "read_reflection_probes", "set_reflection_params", "reflection_prefilter",
                 "reflection_chain_size", "read_reflection"):
        assert hasattr(host.Context, name), name
        assert re.search(r"void %s\(" % name, hpp), name
    for name in ("debug_cube_rays", "debug_reflection_samples", "debug_reflection_prefilter", "reflection_image_size"):
        assert hasattr(host, name), name
    src = open(os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_cube.h")).read()
    assert "0x1f83d9abu" in src and "0x5be0cd19u" in src
