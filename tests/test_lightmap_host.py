"""jpt_bake_finish without a GPU (csrc/jpt_lightmap.h): the host form of the whole transform (jpt_debug_bake_finish, device -1) against
the float32 numpy restatement (tests/np_lightmap.py) bit for bit, properties of the restatement itself -- charts that touch in the
atlas do not bleed, the filter filters, the dilation fills exactly the rings it is asked for --, the C ABI's refusals on a host-only
context and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_bake as nb
import np_lightmap as nl

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # JPT_E_* of include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (5, 3), (33, 17), (32, 32), (70, 41))
NOISE_SEED = 5


@pytest.fixture(scope="module")
def L():
    return capi.lib()


# ---- 1. the host form equals the restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_numpy_restatement_bit_for_bit(size):
    """charts that touch in the atlas, an isolated valid texel (fp2 = 0), invalid texels holding NaN and non-finite means in valid
    texels (np_lightmap.synthetic_case); every passes value, with no dilation, one ring, the default and the most"""
    w, h = size
    mean, p4, n4 = nl.synthetic_case(w, h, seed=w)
    xg, _ = nl.guides(p4, n4)
    assert xg[0, w - 1, 3] == 0                                  # the isolated texel: valid, no valid 4-neighbour
    if w * h > 16:
        valid = nb.texel_valid(n4)
        assert 0 < valid.sum() < w * h and np.isnan(p4[~valid]).any() and not np.isfinite(mean[valid][:, :3]).all()
        assert (xg[..., 3] > 0).any()
    for passes in range(0, 7):
        for dilate in (0, 1, 4, 64):
            got = host.debug_bake_finish(HOST_ONLY, mean, p4, n4, passes=passes, dilate=dilate)
            want = nl.finish(mean, p4, n4, passes=passes, dilate=dilate)
            bad = ~nl.same_bits(got, want)
            assert not bad.any(), "%dx%d passes %d dilate %d: %d values differ, first %s" % (w, h, passes, dilate, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_other_parameters_and_the_defaults_equal_numpy_too():
    mean, p4, n4 = nl.synthetic_case(70, 41, seed=9)
    for prm in (dict(passes=4, normal_power_log2=0, sigma_distance=1.5, sigma_plane=0.25, sigma_color=0.5, dilate=2),
                dict(passes=6, normal_power_log2=8, sigma_distance=64.0, sigma_plane=8.0, sigma_color=64.0, dilate=7)):
        assert nl.same_bits(host.debug_bake_finish(HOST_ONLY, mean, p4, n4, **prm), nl.finish(mean, p4, n4, **prm)).all(), prm
    assert nl.same_bits(host.debug_bake_finish(HOST_ONLY, mean, p4, n4), nl.finish(mean, p4, n4, **nl.DEFAULTS)).all()
    assert nl.same_bits(host.debug_bake_finish(HOST_ONLY, mean, p4, n4, params=capi.BakeFinishParams()), nl.finish(mean, p4, n4)).all()


# ---- 2. charts that touch in the atlas do not bleed ------------------------------------------------------------------------------------------

def test_charts_that_touch_in_the_atlas_do_not_bleed():
    """np_lightmap.three_charts(): after 5 passes with the defaults every texel of A is exactly 1 and every texel of C exactly 2 -- A
    and B are 50 units apart (the distance test), B and C have perpendicular normals (the normal weight), and a weighted mean of equal
    values is exact.  B, a ramp of slope 0.01 per texel over 30 texels, keeps the edge bias of a ramp: every output is a weighted
    mean of B's own values, so it stays inside their range, and the worst case is an edge texel drawn to the chart's mean, half the
    range = 0.145 (the float64 prototype of the design measured at most 0.15; this restatement 0.088)."""
    truth, p4, n4, (a, b, c) = nl.three_charts()
    for out in (nl.finish(truth, p4, n4, passes=5, dilate=0), host.debug_bake_finish(HOST_ONLY, truth, p4, n4, passes=5, dilate=0)):
        assert (out[a][:, :3] == 1).all() and (out[c][:, :3] == 2).all()
        assert (out[a | b | c][:, 3] == 1).all() and (out[~(a | b | c)] == 0).all()
        err = np.abs(out[b][:, :3].astype(np.float64) - truth[b][:, :3])
        print("chart B: max |out - truth| = %.4f" % err.max())
        assert err.max() <= 0.15
        assert out[b][:, :3].min() >= truth[b][:, :3].min() - 1e-6 and out[b][:, :3].max() <= truth[b][:, :3].max() + 1e-6
    # the filter did something to B: it is not the identity
    assert not np.array_equal(out[b], truth[b])
    # without the distance test A and B would mix: the same images with B moved onto A's plane
    flat = p4.copy()
    flat[b, 2] = 0.0
    flat[b, 0] += F(2.8)
    mixed = nl.finish(truth, flat, n4, passes=5, dilate=0)
    assert (mixed[a][:, :3] != 1).any()


# ---- 3. the filter filters -------------------------------------------------------------------------------------------------------------------

def test_noise_on_the_three_charts_is_halved_at_least():
    """truth + N(0, 0.3) on the valid texels, seed 5, 3 passes, on the restatement: RMSE(out - truth) < 0.5 RMSE(mean - truth) over the
    valid texels.  Measured here: 0.0269 against 0.3020, a ratio of 0.089 (1, 2, 4, 5 passes: 0.30, 0.15, 0.091, 0.14); the float64
    prototype of the design gave 0.10.  The cap is loose: it only has to show that the filter filters."""
    truth, p4, n4, (a, b, c) = nl.three_charts()
    valid = a | b | c
    rng = np.random.default_rng(NOISE_SEED)
    noisy = truth.copy()
    noisy[valid, :3] += (rng.standard_normal((int(valid.sum()), 3)) * 0.3).astype(F)

    def rmse(img):
        return float(np.sqrt(np.mean((img[valid][:, :3].astype(np.float64) - truth[valid][:, :3]) ** 2)))

    out = nl.finish(noisy, p4, n4, passes=3, dilate=0)
    print("RMSE mean %.4f, 3 passes %.4f, ratio %.3f" % (rmse(noisy), rmse(out), rmse(out) / rmse(noisy)))
    assert rmse(out) < 0.5 * rmse(noisy)


# ---- 4. dilation -----------------------------------------------------------------------------------------------------------------------------

def _chebyshev(valid):
    """per texel, the Chebyshev distance to the nearest True texel (a large number where there is none), by growing rings"""
    h, w = valid.shape
    dist = np.where(valid, 0, 10 ** 6)
    reach = valid.copy()
    for d in range(1, max(h, w) + 1):
        grown = reach.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                grown |= nl._shift(reach, dx, dy)[0]
        dist = np.where(grown & ~reach, d, dist)
        reach = grown
    return dist


@pytest.mark.parametrize("passes", (0, 2))
def test_dilation_fills_exactly_the_rings_it_is_asked_for(passes):
    truth, p4, n4, (a, b, c) = nl.three_charts()
    p4[20, 69], n4[20, 69] = (9.0, 9.0, 9.0, 0.0), (0.0, 1.0, 0.0, 1.0)          # a lone valid texel at the image's edge
    truth[20, 69, :3] = 3.0
    valid = nb.texel_valid(n4)
    dist = _chebyshev(valid)
    assert dist.max() >= 2 and valid[20, 69]
    base = nl.finish(truth, p4, n4, passes=passes, dilate=0)
    assert (base[..., 3] == np.where(valid, 1, 0)).all() and (base[~valid] == 0).all()
    if passes == 0:
        assert np.array_equal(base[..., :3], np.where(valid[..., None], truth[..., :3], 0))   # the mean itself, with coverage
    for d in (1, 2, 4, 64):
        out = nl.finish(truth, p4, n4, passes=passes, dilate=d)
        assert nl.same_bits(out, host.debug_bake_finish(HOST_ONLY, truth, p4, n4, passes=passes, dilate=d)).all()
        filled = ~valid & (dist <= d)
        assert (out[..., 3] == np.where(valid, 1.0, np.where(filled, 0.5, 0.0))).all(), d
        assert (out[~valid & ~filled] == 0).all()
        assert np.array_equal(out[valid], base[valid])                           # a valid texel's colour is unchanged by dilation
        assert np.isfinite(out).all()
        # a filled texel is a mean of what its ring saw: inside the range of the map
        assert out[filled][:, :3].min() >= base[valid][:, :3].min() - 1e-6 and out[filled][:, :3].max() <= base[valid][:, :3].max() + 1e-6
    assert (nl.finish(truth, p4, n4, passes=passes, dilate=64)[..., 3] > 0).all()   # 64 rings cover the whole 70 x 41 atlas
    # the first ring, by hand: the texel left of chart A's edge sees three texels of A, weights 1 2 1, all exactly 1
    one = nl.finish(truth, p4, n4, passes=0, dilate=1)
    assert (one[10, 1] == (1, 1, 1, 0.5)).all() and (one[1, 1] == (1, 1, 1, 0.5)).all() and (one[10, 0] == 0).all()
    # ... and the one between A's last column and B's first does not exist (they touch); C's right neighbour sees C alone
    assert (one[10, 68] == (2, 2, 2, 0.5)).all()


def test_a_non_finite_texel_is_neither_a_tap_nor_a_source_of_dilation():
    truth, p4, n4, (a, b, c) = nl.three_charts()
    mean = truth.copy()
    mean[10, 2, 0] = np.inf                                                      # chart A's edge texel
    out = nl.finish(mean, p4, n4, passes=3, dilate=2)
    assert out[10, 2, 0] == np.inf and out[10, 2, 3] == 1                        # passes through
    rest = a.copy()
    rest[10, 2] = False
    assert (out[rest][:, :3] == 1).all()                                         # nobody took it as a tap
    assert np.isfinite(out[:, :2]).all() and (out[9:12, 1, :3] == 1).all()       # the ring beside it is filled from its neighbours


# ---- 5. the C ABI ----------------------------------------------------------------------------------------------------------------------------

BAD_PARAMS = [dict(passes=-1), dict(passes=7), dict(normal_power_log2=-1), dict(normal_power_log2=9), dict(dilate=-1), dict(dilate=65)] + [
    {field: value} for field in ("sigma_distance", "sigma_plane", "sigma_color") for value in (0.0, -1.0, float("nan"), float("inf"))]


def test_refusals_on_a_host_only_context(L):
    for name in ("jpt_set_bake_finish_params", "jpt_bake_finish", "jpt_read_lightmap_f32", "jpt_debug_bake_finish"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.jpt_abi_version() == 6
    ctx = host.Context(HOST_ONLY)
    try:
        def refused(rc, code, call):
            assert rc == code, (rc, code, call)
            assert call.encode() in L.jpt_last_error(ctx.h), L.jpt_last_error(ctx.h)
        S = L.jpt_set_bake_finish_params
        for fields in BAD_PARAMS:
            refused(S(ctx.h, C.byref(capi.BakeFinishParams(**fields))), E_INVALID, "jpt_set_bake_finish_params")
        for fields in (dict(passes=0, dilate=0), dict(passes=6, dilate=64, normal_power_log2=8), dict(normal_power_log2=0)):
            refused(S(ctx.h, C.byref(capi.BakeFinishParams(**fields))), E_DEVICE, "jpt_set_bake_finish_params")   # checks passed: no device
        refused(S(ctx.h, None), E_DEVICE, "jpt_set_bake_finish_params")
        # the state errors that need no device come before the device is asked for
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        refused(L.jpt_bake_finish(ctx.h), E_STATE, "jpt_bake_finish")
        assert b"JPT_DENOISE_PROGRESSIVE" in L.jpt_last_error(ctx.h)
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        refused(L.jpt_bake_finish(ctx.h), E_STATE, "jpt_bake_finish")
        assert b"DEBUG_STEPS" in L.jpt_last_error(ctx.h)
        ctx.set_debug_steps(False)
        ctx.set_partition(1, 2)
        refused(L.jpt_bake_finish(ctx.h), E_STATE, "jpt_bake_finish")
        assert b"whole image on one context" in L.jpt_last_error(ctx.h)
        ctx.set_partition(0, 1)
        # (no bake images, another size, no frame: a host-only context cannot hold images -- tests/test_gpu_lightmap.py)
        refused(L.jpt_bake_finish(ctx.h), E_DEVICE, "jpt_bake_finish")
        out = np.zeros(4, F)
        refused(L.jpt_read_lightmap_f32(ctx.h, None), E_INVALID, "jpt_read_lightmap_f32")
        refused(L.jpt_read_lightmap_f32(ctx.h, out.ctypes.data), E_DEVICE, "jpt_read_lightmap_f32")
        with pytest.raises(capi.JptError, match="jpt_bake_finish"):
            ctx.bake_finish()
        with pytest.raises(capi.JptError, match="jpt_read_lightmap_f32"):
            ctx.read_lightmap()
        with pytest.raises(capi.JptError, match="passes"):
            ctx.set_bake_finish_params(passes=9)
    finally:
        ctx.close()
    assert L.jpt_set_bake_finish_params(None, None) == E_INVALID and L.jpt_bake_finish(None) == E_INVALID
    assert L.jpt_read_lightmap_f32(None, np.zeros(4, F).ctypes.data) == E_INVALID


def test_the_debug_call_checks_its_arguments(L):
    mean, p4, n4 = nl.synthetic_case(8, 8, seed=1)
    out = np.zeros((8, 8, 4), F)
    D = L.jpt_debug_bake_finish
    pm, pp, pn, po = (x.ctypes.data for x in (mean, p4, n4, out))

    def refused(rc, code, *words):
        assert rc == code, (rc, code)
        for word in ("jpt_debug_bake_finish",) + words:
            assert word.encode() in L.jpt_debug_last_error(), L.jpt_debug_last_error()
    for k in range(4):
        ptrs = [pm, pp, pn, po]
        ptrs[k] = None
        refused(D(HOST_ONLY, 8, 8, None, *ptrs), E_INVALID, "null")
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        refused(D(HOST_ONLY, w, h, None, pm, pp, pn, po), E_INVALID, "width and height")
    refused(D(HOST_ONLY, 1 << 13, (1 << 13) + 1, None, pm, pp, pn, po), E_LIMIT, "2^26")       # refused before a read
    refused(D(HOST_ONLY, 1 << 30, 1 << 30, None, pm, pp, pn, po), E_LIMIT, "2^26")
    for fields in BAD_PARAMS:
        refused(D(HOST_ONLY, 8, 8, C.byref(capi.BakeFinishParams(**fields)), pm, pp, pn, po), E_INVALID, list(fields)[0])
    # a valid texel with a non-finite position or normal component, as jpt_set_bake_texels refuses it
    valid = np.argwhere(nb.texel_valid(n4))[0]
    for img, bad in ((p4, np.nan), (p4, np.inf), (n4, np.inf)):
        b_p, b_n = p4.copy(), n4.copy()
        (b_p if img is p4 else b_n)[valid[0], valid[1], 1] = bad
        refused(D(HOST_ONLY, 8, 8, None, pm, b_p.ctypes.data, b_n.ctypes.data, po), E_INVALID, "non-finite")
    assert D(HOST_ONLY, 8, 8, None, pm, pp, pn, po) == 0
    assert nl.same_bits(out, nl.finish(mean, p4, n4)).all()
    with pytest.raises(capi.JptError, match="jpt_debug_bake_finish: dilate"):
        host.debug_bake_finish(HOST_ONLY, mean, p4, n4, dilate=65)


# ---- 6. declarations -------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for proto in (
            r"int jpt_set_bake_finish_params\(jpt_ctx \*ctx, const jpt_bake_finish_params \*params\);",
            r"int jpt_bake_finish\(jpt_ctx \*ctx\);",
            r"int jpt_read_lightmap_f32\(jpt_ctx \*ctx, float \*out\);",
            r"int jpt_debug_bake_finish\(int device_id, int32_t width, int32_t height, const jpt_bake_finish_params \*params,\s+const float \*mean4, const float \*position4, const float \*normal4, float \*out\);",
            r"typedef struct jpt_bake_finish_params \{\s+int32_t passes;[^}]*int32_t normal_power_log2;[^}]*int32_t dilate;[^}]*float\s+sigma_distance;[^}]*float\s+sigma_plane;[^}]*float\s+sigma_color;[^}]*\} jpt_bake_finish_params;"):
        assert re.search(proto, text), proto
    assert re.search(r"#define JPT_ABI_VERSION 6\b", text)
    assert "64 B per" in text and "dilation of the finished map (do it" not in text
    hpp = open(os.path.join(ROOT, "include", "jpt_host.hpp")).read()
    for name in ("set_bake_finish_params", "bake_finish", "read_lightmap"):
        assert hasattr(host.Context, name), name
        assert re.search(r"void %s\(" % name, hpp), name
    assert hasattr(host, "debug_bake_finish")
    assert C.sizeof(capi.BakeFinishParams) == 24
    d = capi.BakeFinishParams()
    assert (d.passes, d.normal_power_log2, d.dilate, d.sigma_distance, d.sigma_plane, d.sigma_color) == (3, 4, 4, 4.0, 1.0, 4.0)
