"""Light probes on the host (jpt_set_probes, jpt_probe_project; CPU): the host's copy of the probe ray, of the quadrature table and of
the projection's pinned sum against tests/np_probe.py, what the table recovers, and the argument checks that need no device.  Tiles
8 x 4 (32 lanes of the projection idle), 12 x 6 (lanes 8.. hold one cell fewer) and 16 x 8; five probes, three to a row, so the sixth
tile has no probe."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_probe as npb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # JPT_E_*
TILES = ((8, 4), (12, 6), (16, 8))
N_PROBES, PER_ROW = 5, 3
POSITIONS = np.array([(0.0, 0.0, 0.0), (1.5, -0.25, 2.0), (-3.0, 0.5, 0.75), (0.125, 4.0, -2.5), (2.0, 1.0, 1.0)], F)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((_u32(a) == _u32(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def L():
    return capi.lib()


# ---- 1. the probe ray --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", TILES)
def test_host_probe_rays_equal_numpy_and_stay_in_their_cells(tile):
    tw, th = tile
    w, h = npb.image_size(N_PROBES, tw, th, PER_ROW)
    assert (w, h) == host.probe_image_size(N_PROBES, tw, th, PER_ROW) == (3 * tw, 2 * th)
    for frame in (1, 78):
        o, d, valid = host.debug_probe_rays(HOST_ONLY, POSITIONS, tw, th, PER_ROW, frame)
        _, wo, wd, wv = npb.probe_rays(POSITIONS, tw, th, PER_ROW, frame)
        assert np.array_equal(valid.reshape(-1) != 0, wv), frame
        assert same_bits(o.reshape(-1, 3), wo) and same_bits(d.reshape(-1, 3), wd), frame
        # the tile past the last probe is invalid, and only it
        v = valid.reshape(h, w) != 0
        assert not v[th:, 2 * tw:].any() and v[:th].all() and v[th:, :2 * tw].all()
        assert not o[th:, 2 * tw:].any() and not d[th:, 2 * tw:].any()
        p, ci, cj, ok = npb.pixel_cells(N_PROBES, tw, th, PER_ROW)
        assert same_bits(o.reshape(-1, 3)[ok], POSITIONS[p[ok]])                 # the origin is the probe, no offset
        # every valid direction lies inside its own cell: undo the map in float64, one float ulp of slack at the borders
        dd = d.reshape(-1, 3).astype(np.float64)[ok]
        assert np.abs(np.sqrt((dd * dd).sum(axis=1)) - 1.0).max() < 1e-6
        u = np.arctan2(dd[:, 0], dd[:, 2]) / (2.0 * np.pi) + 0.5
        vv = (1.0 - dd[:, 1]) / 2.0
        fi, fj = u * tw - ci[ok], vv * th - cj[ok]
        eps_u, eps_v = tw * float(np.finfo(F).eps), th * float(np.finfo(F).eps)   # one ulp of u (v) at 1, in cells
        wrap = (ci[ok] == tw - 1) & (fi < -0.5)                                  # (phi = +pi comes back from atan2 as -pi)
        fi = np.where(wrap, fi + tw, fi)
        assert (fi >= -eps_u).all() and (fi <= 1.0 + eps_u).all(), (fi.min(), fi.max())
        assert (fj >= -eps_v).all() and (fj <= 1.0 + eps_v).all(), (fj.min(), fj.max())
    # other frames draw other directions, and the hash is not the bake's
    a = host.debug_probe_rays(HOST_ONLY, POSITIONS, tw, th, PER_ROW, 1)[1]
    b = host.debug_probe_rays(HOST_ONLY, POSITIONS, tw, th, PER_ROW, 2)[1]
    assert not np.array_equal(a, b)
    assert npb.HASH == (0x510e527f, 0x9b05688c) and set(npb.HASH).isdisjoint({0x3c6ef372, 0xa54ff53a})


# ---- 2. the table ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE))
@pytest.mark.parametrize("tile", TILES)
def test_the_table_is_the_closed_forms_to_one_ulp_and_its_columns_sum_as_they_must(tile, flags):
    tw, th = tile
    cells = tw * th
    got = host.debug_probe_basis(tw, th, flags)
    want = npb.table64(tw, th, flags)
    assert got.shape == (th, tw, 9) and got.dtype == F
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print("table %d x %d flags %d: worst error %.3g ulp" % (tw, th, flags, float((err / ulp).max())))
    assert (err <= ulp).all(), float((err / ulp).max())
    sums = got.astype(np.float64).reshape(cells, 9).sum(axis=0)
    factor = npb.BAND_FACTOR if flags else np.ones(9)
    # each entry is rounded once, by at most half an ulp <= 2^-24 of its magnitude, and no entry exceeds 4 pi / cells * max|Y| / G
    # < 4 pi (in fact ~ 1 / cells): the sum of `cells` entries is within cells * 2^-23 * 4 pi of the exact sum, 2 sqrt(pi) or 0
    bound = cells * 2.0 ** -23 * 4.0 * np.pi
    assert abs(sums[0] - 2.0 * np.sqrt(np.pi) * factor[0]) <= bound, sums[0]
    assert (np.abs(sums[1:]) <= bound).all(), sums


def test_the_basis_is_orthonormal_and_the_table_is_its_dual():
    """the basis of np_probe (and of the header) is orthonormal over the sphere, and the float64 table recovers each function from its
    own cell means: sum over cells of table[k] * mean(Y_l) = delta_kl"""
    tw, th = 16, 8
    d = npb.directions(tw, th, 64)
    y = npb.basis(d)
    gram = np.einsum("ijk,ijl->kl", y, y) * (4.0 * np.pi / (tw * th * 64 * 64))
    assert np.abs(gram - np.eye(9)).max() < 5e-4
    means = y.reshape(th, 64, tw, 64, 9).mean(axis=(1, 3))
    dual = np.einsum("ijk,ijl->kl", npb.table64(tw, th), means)
    assert np.abs(dual - np.eye(9)).max() < 5e-4, np.abs(dual - np.eye(9)).max()


LIMIT_TILES = ((4, 2), (4, 8), (5, 2), (16, 2), (64, 16), (32, 32), (5, 3))


@pytest.mark.parametrize("flags", (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE))
@pytest.mark.parametrize("tile", LIMIT_TILES)
def test_the_table_is_finite_at_the_limit_shapes_and_zero_where_the_grid_is_blind(tile, flags):
    """two rows of cells cannot tell Y6 from a constant (the mean of z^2 over either half is 1/3) and four columns cannot see cos 2 phi
    (Y8): those columns are zero, not 0 / 0; every other column of every accepted tile is the dual of the cell means"""
    tw, th = tile
    got = host.debug_probe_basis(tw, th, flags).astype(np.float64)
    factor = npb.BAND_FACTOR if flags else np.ones(9)
    assert np.isfinite(got).all()
    # |t| = w |mean| / G <= sqrt(w / G) by Cauchy-Schwarz (w mean^2 <= G), G >= 0.2 for a kept column and w <= 4 pi / 8
    assert (np.abs(got) <= np.sqrt(4.0 * np.pi / 8.0 / 0.2) * factor).all(), np.abs(got).max()
    blind = np.zeros(9, bool)
    blind[6], blind[8] = th == 2, tw == 4
    for k in range(9):
        assert (got[..., k] == 0).all() == bool(blind[k]), (k, tile)
    # the Gram diagonals the rule keeps are nowhere near its threshold (1e-9), and those it drops are rounding noise
    means = npb.cell_means(tw, th)
    w = 4.0 * np.pi / (tw * th)
    gram = (w * means * means).reshape(-1, 9).sum(axis=0)
    assert (gram[~blind] > 0.2).all() and (gram[blind] < 1e-30).all(), gram
    want = npb.table64(tw, th, flags)
    assert np.isfinite(want).all() and (np.abs(got - want) <= np.spacing(np.abs(want).astype(F)).astype(np.float64)).all()
    # dual to the cell means: sum over cells of t_k * mean_l = delta_kl for the columns kept, to the rounding of the float entries
    # (each within 2^-24 of its magnitude)
    t = (got / factor).reshape(-1, 9)
    m = means.reshape(-1, 9)
    dual, slack = t.T @ m, 2.0 ** -24 * (np.abs(t).T @ np.abs(m)) + 1e-14
    assert (np.abs(dual - np.diag((~blind).astype(np.float64))) <= slack).all(), np.abs(dual - np.diag((~blind).astype(np.float64))).max()
    # and a projection through it is finite: constant radiance lands in coefficient 0 alone
    a = np.ones((th, tw, 4), F)
    sh = host.debug_probe_project(HOST_ONLY, a, 1, 1, tw, th, 1, got.astype(F))[0, :, 0].astype(np.float64)
    assert np.isfinite(sh).all() and abs(sh[0] - 2.0 * np.sqrt(np.pi) * factor[0]) < 1e-4 and (np.abs(sh[1:]) < 1e-4).all(), sh


# ---- 3. the projection ---------------------------------------------------------------------------------------------------------------------

def accum_image(tw, th, frames, seed=5):
    rng = np.random.default_rng(seed)
    w, h = npb.image_size(N_PROBES, tw, th, PER_ROW)
    a = (rng.uniform(0.0, 4.0, (h, w, 4)) * frames).astype(F)
    a[..., 3] = 1.0
    a[th:, 2 * tw:] = 0.0
    return a


@pytest.mark.parametrize("tile", TILES)
def test_host_projection_equals_numpy_bit_for_bit(tile):
    tw, th = tile
    for frames in (1, 3):
        a = accum_image(tw, th, frames)
        for flags in (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE):
            table = host.debug_probe_basis(tw, th, flags)
            got = host.debug_probe_project(HOST_ONLY, a, frames, N_PROBES, tw, th, PER_ROW, table)
            want = npb.project(a, frames, N_PROBES, tw, th, PER_ROW, table)
            assert got.shape == (N_PROBES, 9, 4) and same_bits(got, want), (frames, flags)
            assert (got[..., 3] == 0).all() and (got[:, 0, :3] > 0).all()
    # the probes are apart: another probe's tile does not leak in
    a2 = a.copy()
    a2[:th, :tw] *= F(2.0)
    got2 = host.debug_probe_project(HOST_ONLY, a2, 3, N_PROBES, tw, th, PER_ROW, table)
    assert not same_bits(got2[0], got[0]) and same_bits(got2[1:], got[1:])


@pytest.mark.parametrize("tile", TILES)
def test_band_limited_radiance_is_recovered(tile):
    """nine coefficients in [-1, 1]; every cell holds the float64 mean of that radiance over 64 x 64 midpoint sub-samples; the
    projection returns the coefficients within 5e-4 (the test's own sub-sampling: 1.1e-4 at worst), and with JPT_PROBE_IRRADIANCE the
    same after dividing by the band factors"""
    tw, th = tile
    rng = np.random.default_rng(1 + tw)
    coeff = rng.uniform(-1.0, 1.0, (3, 9))
    y = npb.basis(npb.directions(tw, th, 64))
    w, h = npb.image_size(1, tw, th, 1)
    a = np.zeros((h, w, 4), F)
    for ch in range(3):
        a[..., ch] = (y @ coeff[ch]).reshape(th, 64, tw, 64).mean(axis=(1, 3))
    for flags in (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE):
        table = host.debug_probe_basis(tw, th, flags)
        got = host.debug_probe_project(HOST_ONLY, a, 1, 1, tw, th, 1, table)[0, :, :3].astype(np.float64).T
        if flags:
            got = got / npb.BAND_FACTOR
        err = np.abs(got - coeff).max()
        print("recovery %d x %d flags %d: worst error %.3g" % (tw, th, flags, err))
        assert err <= 5e-4, err


# ---- 4. the checks ---------------------------------------------------------------------------------------------------------------------------

def test_the_calls_check_their_arguments_on_a_host_only_context(L):
    for name in ("jpt_set_probes", "jpt_get_probe_image_size", "jpt_read_probes", "jpt_probe_project", "jpt_read_probe_sh_f32", "jpt_debug_probe_rays",
                 "jpt_debug_probe_basis", "jpt_debug_probe_project"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.jpt_abi_version() == 6
    pos = np.zeros((8, 3), F)
    ctx = host.Context(HOST_ONLY)
    try:
        def refused(rc, code, call, word=None):
            assert rc == code, (rc, code, call)
            msg = L.jpt_last_error(ctx.h)
            assert call.encode() in msg and (word is None or word.encode() in msg), msg
        S = lambda p, n, tw, th, per: L.jpt_set_probes(ctx.h, None if p is None else p.ctypes.data, n, tw, th, per)   # noqa: E731
        for tw in (3, 65, 0, -1):
            refused(S(pos, 8, tw, 8, 4), E_INVALID, "jpt_set_probes", "tile_w")
        for th in (1, 33, 0):
            refused(S(pos, 8, 16, th, 4), E_INVALID, "jpt_set_probes", "tile_h")
        refused(S(pos, 8, 64, 32, 4), E_INVALID, "jpt_set_probes", "1024")
        refused(S(pos, 8, 64, 17, 4), E_INVALID, "jpt_set_probes", "1024")
        refused(S(pos, 0, 16, 8, 4), E_LIMIT, "jpt_set_probes", "n_probes")
        refused(S(pos, -1, 16, 8, 4), E_LIMIT, "jpt_set_probes", "n_probes")
        refused(S(pos, (1 << 20) + 1, 16, 8, 4), E_LIMIT, "jpt_set_probes", "n_probes")
        refused(S(pos, 8, 16, 8, 0), E_INVALID, "jpt_set_probes", "probes_per_row")
        refused(S(None, 8, 16, 8, 4), E_INVALID, "jpt_set_probes", "NULL")
        big = np.zeros((1 << 20, 3), F)
        refused(S(big, 1 << 20, 64, 16, 1024), E_LIMIT, "jpt_set_probes", "2^26")          # 2^20 tiles of 2^10 pixels
        refused(S(big, 1 << 20, 8, 8, 1024), E_DEVICE, "jpt_set_probes")                   # 2^26 pixels exactly: the checks pass
        for bad in (np.nan, np.inf, -np.inf):
            q = pos.copy()
            q[5, 1] = bad
            refused(S(q, 8, 16, 8, 4), E_INVALID, "jpt_set_probes", "probe 5")
        refused(S(pos, 8, 16, 8, 4), E_DEVICE, "jpt_set_probes")                           # the checks passed: no device
        refused(S(pos, 8, 4, 2, 3), E_DEVICE, "jpt_set_probes")
        refused(S(pos, 8, 64, 16, 8), E_DEVICE, "jpt_set_probes")
        refused(S(None, 0, 0, 0, 0), E_DEVICE, "jpt_set_probes")                           # (freeing)
        w, h = C.c_int32(0), C.c_int32(0)
        refused(L.jpt_get_probe_image_size(ctx.h, None, C.byref(h)), E_INVALID, "jpt_get_probe_image_size")
        refused(L.jpt_get_probe_image_size(ctx.h, C.byref(w), C.byref(h)), E_DEVICE, "jpt_get_probe_image_size")
        refused(L.jpt_read_probes(ctx.h, None), E_INVALID, "jpt_read_probes")
        refused(L.jpt_read_probes(ctx.h, pos.ctypes.data), E_DEVICE, "jpt_read_probes")
        # jpt_probe_project: the flags, then the state errors that need no device, then the device
        for flags in (2, -1, 3):
            refused(L.jpt_probe_project(ctx.h, flags), E_INVALID, "jpt_probe_project", "flags")
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        refused(L.jpt_probe_project(ctx.h, 0), E_STATE, "jpt_probe_project", "JPT_DENOISE_PROGRESSIVE")
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_probe_project(ctx.h, 0), E_STATE, "jpt_probe_project", "DEBUG_STEPS")
        ctx.set_debug_steps(False)
        ctx.set_partition(1, 2)
        refused(L.jpt_probe_project(ctx.h, 1), E_STATE, "jpt_probe_project", "whole image on one context")
        ctx.set_partition(0, 1)
        refused(L.jpt_probe_project(ctx.h, 1), E_DEVICE, "jpt_probe_project")
        out = np.zeros(36, F)
        refused(L.jpt_read_probe_sh_f32(ctx.h, None), E_INVALID, "jpt_read_probe_sh_f32")
        refused(L.jpt_read_probe_sh_f32(ctx.h, out.ctypes.data), E_DEVICE, "jpt_read_probe_sh_f32")
        with pytest.raises(capi.JptError, match="tile_w"):
            ctx.set_probes(pos, 2, 8, 4)
        with pytest.raises(capi.JptError, match="jpt_probe_project"):
            ctx.probe_project()
        with pytest.raises(capi.JptError, match="jpt_read_probe_sh_f32"):
            ctx.read_probe_sh()
    finally:
        ctx.close()
    assert L.jpt_set_probes(None, pos.ctypes.data, 8, 16, 8, 4) == E_INVALID and L.jpt_probe_project(None, 0) == E_INVALID
    assert L.jpt_read_probe_sh_f32(None, pos.ctypes.data) == E_INVALID and L.jpt_read_probes(None, pos.ctypes.data) == E_INVALID
    assert L.jpt_get_probe_image_size(None, None, None) == E_INVALID


def test_the_debug_calls_check_their_arguments(L):
    pos = np.zeros((2, 3), F)
    o, d, v = np.zeros((8, 16, 3), F), np.zeros((8, 16, 3), F), np.zeros((8, 16), np.uint8)
    R = L.jpt_debug_probe_rays
    assert R(HOST_ONLY, None, 2, 8, 4, 2, 1, o.ctypes.data, d.ctypes.data, v.ctypes.data) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 8, 4, 2, 1, None, d.ctypes.data, v.ctypes.data) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 3, 4, 2, 1, o.ctypes.data, d.ctypes.data, v.ctypes.data) == E_INVALID
    assert b"jpt_debug_probe_rays" in L.jpt_debug_last_error() and b"tile_w" in L.jpt_debug_last_error()
    assert R(HOST_ONLY, pos.ctypes.data, 0, 8, 4, 2, 1, o.ctypes.data, d.ctypes.data, v.ctypes.data) == E_LIMIT
    bad = pos.copy()
    bad[1, 2] = np.nan
    assert R(HOST_ONLY, bad.ctypes.data, 2, 8, 4, 2, 1, o.ctypes.data, d.ctypes.data, v.ctypes.data) == E_INVALID
    assert R(HOST_ONLY, pos.ctypes.data, 2, 8, 4, 2, 1, o.ctypes.data, d.ctypes.data, v.ctypes.data) == capi.OK
    t = np.zeros((4, 8, 9), F)
    B = L.jpt_debug_probe_basis
    assert B(8, 4, 0, None) == E_INVALID and B(8, 4, 2, t.ctypes.data) == E_INVALID and B(8, 1, 0, t.ctypes.data) == E_INVALID
    assert B(65, 4, 0, t.ctypes.data) == E_INVALID and B(64, 32, 0, t.ctypes.data) == E_INVALID
    assert b"jpt_debug_probe_basis" in L.jpt_debug_last_error()
    assert B(8, 4, 1, t.ctypes.data) == capi.OK and t.any()
    a, sh = np.zeros((4, 16, 4), F), np.zeros((2, 9, 4), F)
    J = L.jpt_debug_probe_project
    assert J(HOST_ONLY, None, 1, 2, 8, 4, 2, t.ctypes.data, sh.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 8, 4, 2, None, sh.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 0, 2, 8, 4, 2, t.ctypes.data, sh.ctypes.data) == E_INVALID
    assert b"frame_count" in L.jpt_debug_last_error()
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 8, 40, 2, t.ctypes.data, sh.ctypes.data) == E_INVALID
    assert J(HOST_ONLY, a.ctypes.data, 1, 0, 8, 4, 2, t.ctypes.data, sh.ctypes.data) == E_LIMIT
    assert J(HOST_ONLY, a.ctypes.data, 1, 2, 8, 4, 2, t.ctypes.data, sh.ctypes.data) == capi.OK
    with pytest.raises(capi.JptError, match="tile_h"):
        host.debug_probe_basis(8, 40)
    with pytest.raises(ValueError):
        host.debug_probe_project(HOST_ONLY, a[:2], 1, 2, 8, 4, 2, t)


def test_the_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for proto in (
            r"int jpt_set_probes\(jpt_ctx \*ctx, const float \*position3, int32_t n_probes, int32_t tile_w, int32_t tile_h, int32_t probes_per_row\);",
            r"int jpt_get_probe_image_size\(jpt_ctx \*ctx, int32_t \*width, int32_t \*height\);",
            r"int jpt_read_probes\(jpt_ctx \*ctx, float \*position3\);",
            r"enum \{ JPT_PROBE_RADIANCE = 0, JPT_PROBE_IRRADIANCE = 1 \};",
            r"int jpt_probe_project\(jpt_ctx \*ctx, int32_t flags\);",
            r"int jpt_read_probe_sh_f32\(jpt_ctx \*ctx, float \*out\);",
            r"int jpt_debug_probe_rays\(int device_id, const float \*position3, int32_t n_probes, int32_t tile_w, int32_t tile_h,\s+int32_t probes_per_row, uint32_t frame_index, float \*origins3_out, float \*dirs3_out, uint8_t \*valid_out\);",
            r"int jpt_debug_probe_basis\(int32_t tile_w, int32_t tile_h, int32_t flags, float \*table_out\);",
            r"int jpt_debug_probe_project\(int device_id, const float \*accum4, uint32_t frame_count, int32_t n_probes, int32_t tile_w, int32_t tile_h,\s+int32_t probes_per_row, const float \*table, float \*sh_out\);"):
        assert re.search(proto, text), proto
    assert re.search(r"#define JPT_ABI_VERSION 6\b", text)
    assert "144\n * B per probe" in text or "144 B per probe" in text
    assert "0x510e527f, 0x9b05688c" in text
    assert "lightmaps and SH probes" not in text                                  # no longer out of the bake section's scope
    hpp = open(os.path.join(ROOT, "include", "jpt_host.hpp")).read()
    for name in ("set_probes", "probe_image_size", "read_probes", "probe_project", "read_probe_sh"):
        assert hasattr(host.Context, name), name
        assert re.search(r"void %s\(" % name, hpp), name
    for name in ("debug_probe_rays", "debug_probe_basis", "debug_probe_project", "probe_image_size"):
        assert hasattr(host, name), name
    assert (capi.PROBE_RADIANCE, capi.PROBE_IRRADIANCE) == (0, 1)
    src = open(os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_probe.h")).read()
    assert "0x510e527fu" in src and "0x9b05688cu" in src
