"""jpt_query_rays / jpt_query_rays_device / jpt_query_pixels without a GPU: the wire sizes in the header, in ctypes and in numpy, the
C ABI's refusals on a host-only context in the order the header gives (arguments, then the device), n = 0, and the numpy
restatement (np_query) against itself: the records it makes from its own brute force are the ones it accepts, on the triangle
order each kind of scene hands out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_denoise as nd
import np_query as nq

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def test_the_header_declares_the_records_at_32_and_64_bytes_and_the_abi_is_still_6(L, tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "jpt.h"\n#include "jpt_host.hpp"\n#include <cstddef>\n'
                   'static_assert(sizeof(jpt_ray) == 32 && sizeof(jpt_ray_hit) == 64, "sizes");\n'
                   'static_assert(offsetof(jpt_ray, tmax) == 12 && offsetof(jpt_ray, dir) == 16, "jpt_ray");\n'
                   'static_assert(offsetof(jpt_ray_hit, instance) == 12 && offsetof(jpt_ray_hit, triangle) == 16 && offsetof(jpt_ray_hit, flags) == 24 && '
                   'offsetof(jpt_ray_hit, position) == 28 && offsetof(jpt_ray_hit, normal) == 40 && offsetof(jpt_ray_hit, uv) == 52, "jpt_ray_hit");\n'
                   'static_assert(JPT_ABI_VERSION == 6, "abi");\n'
                   'static_assert(JPT_HIT_VALID == 1 && JPT_HIT_FRONT == 2 && JPT_HIT_BAD_RAY == 4 && JPT_QUERY_CLOSEST == 0 && JPT_QUERY_ANY == 1, "enums");\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
    assert L.jpt_abi_version() == 6


def test_ctypes_sizes_equal_the_wire_dtypes():
    assert C.sizeof(capi.Ray) == wire.RAY.itemsize == 32 and C.sizeof(capi.RayHit) == wire.RAY_HIT.itemsize == 64
    for struct, dt in ((capi.Ray, wire.RAY), (capi.RayHit, wire.RAY_HIT)):
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dt.fields[name][1], name
            assert getattr(struct, name).size == dt.fields[name][0].itemsize, name
    assert (capi.QUERY_CLOSEST, capi.QUERY_ANY) == (0, 1) and (capi.HIT_VALID, capi.HIT_FRONT, capi.HIT_BAD_RAY) == (1, 2, 4)
    assert all(s in capi.SYMBOLS for s in ("jpt_query_rays", "jpt_query_rays_device", "jpt_query_pixels"))


def test_argument_checks_come_first_then_the_device_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        rays, hits, occ, xy = np.zeros(4, wire.RAY), np.zeros(4, wire.RAY_HIT), np.zeros(4, np.uint8), np.zeros((4, 2), F)
        r, h, o, p = rays.ctypes.data, hits.ctypes.data, occ.ctypes.data, xy.ctypes.data
        for Q in (L.jpt_query_rays, L.jpt_query_rays_device):
            assert Q(None, capi.QUERY_CLOSEST, r, 4, h, o) == E_INVALID
            for mode in (-1, 2):
                assert Q(ctx.h, mode, r, 4, h, o) == E_INVALID and b"mode" in L.jpt_last_error(ctx.h)
            assert Q(ctx.h, capi.QUERY_CLOSEST, None, 4, h, o) == E_INVALID and b"null rays" in L.jpt_last_error(ctx.h)
            assert Q(ctx.h, capi.QUERY_CLOSEST, r, 4, None, o) == E_INVALID and b"hits_out" in L.jpt_last_error(ctx.h)
            assert Q(ctx.h, capi.QUERY_ANY, r, 4, h, o) == E_INVALID and b"must be NULL" in L.jpt_last_error(ctx.h)
            assert Q(ctx.h, capi.QUERY_ANY, r, 4, None, None) == E_INVALID and b"occluded_out" in L.jpt_last_error(ctx.h)
            # the arguments pass: no device
            assert Q(ctx.h, capi.QUERY_CLOSEST, r, 4, h, o) == E_DEVICE and b"host-only" in L.jpt_last_error(ctx.h)
            assert Q(ctx.h, capi.QUERY_CLOSEST, r, 4, h, None) == E_DEVICE
            assert Q(ctx.h, capi.QUERY_ANY, r, 4, None, o) == E_DEVICE
        assert r % 16 == 0 and h % 16 == 0
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, r + 4, 3, h, None) == E_INVALID and b"aligned" in L.jpt_last_error(ctx.h)
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, r, 3, h + 8, None) == E_INVALID
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, r, 3, h, o + 1) == E_INVALID
        assert L.jpt_query_pixels(None, p, 4, h) == E_INVALID
        assert L.jpt_query_pixels(ctx.h, None, 4, h) == E_INVALID and L.jpt_query_pixels(ctx.h, p, 4, None) == E_INVALID
        assert L.jpt_query_pixels(ctx.h, p, 4, h) == E_DEVICE
        with pytest.raises(capi.JptError, match=r"\(-2\).*host-only"):
            ctx.query_rays(np.zeros((2, 3), F), np.ones((2, 3), F))
        with pytest.raises(capi.JptError, match=r"\(-2\).*host-only"):
            ctx.query_pixels([[0.5, 0.5]])
    finally:
        ctx.close()


def test_no_rays_succeed_and_touch_nothing(L):
    ctx = host.Context(HOST_ONLY)
    try:
        hits, occ = nq.miss_record(2, 7), np.full(2, 9, np.uint8)
        before = hits.copy()
        assert L.jpt_query_rays(ctx.h, capi.QUERY_CLOSEST, None, 0, None, None) == 0
        assert L.jpt_query_rays(ctx.h, capi.QUERY_CLOSEST, None, 0, hits.ctypes.data, occ.ctypes.data) == 0
        assert L.jpt_query_rays(ctx.h, capi.QUERY_ANY, None, 0, None, occ.ctypes.data) == 0
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, None, 0, None, None) == 0
        assert L.jpt_query_pixels(ctx.h, None, 0, hits.ctypes.data) == 0
        assert np.array_equal(hits, before) and (occ == 9).all()
        assert L.jpt_query_rays(ctx.h, 5, None, 0, None, None) == E_INVALID     # (a bad mode is a bad mode at any n)
        h, o = ctx.query_rays(np.zeros((0, 3), F), np.zeros((0, 3), F))
        assert h.dtype == wire.RAY_HIT and len(h) == 0 and len(o) == 0 and len(ctx.query_pixels(np.zeros((0, 2), F))) == 0
    finally:
        ctx.close()


def test_make_rays_lays_out_the_wire_record():
    rays = host.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, -1], [0, 2, 0]], [0.5, np.inf])
    raw = rays.view(F).reshape(2, 8)
    assert raw[0].tolist() == [1, 2, 3, 0.5, 0, 0, -1, 0] and raw[1, 3] == np.inf and raw[1, 4:7].tolist() == [0, 2, 0]
    assert (host.make_rays(np.zeros((3, 3)), np.ones((3, 3)))["tmax"] == 0).all()


# ---- the restatement against itself, on the host's copy of each kind of scene --------------------------------------------------------

def _self_made_hits(ref, o, d):
    """the record of the FIRST triangle at each ray's brute-force minimum"""
    with np.errstate(all="ignore"):
        best = nq.brute_force_t(ref, o, d)
        hits, done = nq.miss_record(len(o)), best >= nq.MISS_T
        for i, ti, ok, t, lpos, lout, u, v, front in nd._tri_tests(ref, o, d):
            sel = np.nonzero(ok & (t == best) & ~done)[0]
            if len(sel):
                hits[sel] = nq._records_of(ref, len(sel), ti, i, t[sel], lpos[sel], lout[sel], u[sel], v[sel], front[sel])
                done[sel] = True
    return hits, best


@pytest.mark.parametrize("route", ["sah", "watertight", "reference_exact", "native_upload"])
def test_the_restatement_accepts_its_own_records_on_the_order_each_scene_hands_out(oracle, L, route):
    """the buffers a context hands out (jpt_scene_get_reference_buffer: the triangle order jpt_ray_hit.triangle indexes) describe
    the scene the oracle builds -- the same brute-force minimum for every ray, whatever the order --, and the checker takes a
    record made from them, refuses one with another t, another triangle or a miss, and knows the bad rays and tmax"""
    sc = scenes.cornell_scene()
    ref = oracle.build_scene(sc)
    ctx = host.Context(HOST_ONLY)
    try:
        if route == "native_upload":
            ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures)
        else:
            ctx.build_scene(sc, dict(sah=capi.BUILD_SAH, watertight=capi.BUILD_SAH_WATERTIGHT, reference_exact=capi.BUILD_REFERENCE_EXACT)[route])
        view = nq.scene_view(ctx)
    finally:
        ctx.close()
    o, d = nq.random_rays(300, 11)
    hits, best = _self_made_hits(view, o, d)
    assert np.array_equal(best.view(np.uint32), nq.brute_force_t(ref, o, d).view(np.uint32))
    hit = best < nq.MISS_T
    assert hit.sum() > 100 and (~hit).sum() > 10
    assert not nq.closest_mismatches(view, o, d, None, hits)[0].any()
    assert not nq.closest_mismatches(ref, o, d, None, hits, indexed=False)[0].any()
    k = int(np.nonzero(hit)[0][0])
    for field, value in (("t", np.nextafter(hits["t"][k], F(np.inf))), ("triangle", hits["triangle"][k] ^ 1), ("flags", hits["flags"][k] ^ 2), ("reserved", 1)):
        wrong = hits.copy()
        wrong[field][k] = value
        assert nq.closest_mismatches(view, o, d, None, wrong)[0].nonzero()[0].tolist() == [k], field
    wrong = hits.copy()
    wrong[k] = nq.miss_record(1)[0]
    assert nq.closest_mismatches(view, o, d, None, wrong)[0].nonzero()[0].tolist() == [k]
    # tmax = t is a miss, the next float above it a hit; a bad ray is a bad ray
    at_t = np.where(hit, best, F(0.0))
    assert nq.closest_mismatches(view, o, d, at_t, hits)[0].nonzero()[0].tolist() == np.nonzero(hit)[0].tolist()
    assert not nq.closest_mismatches(view, o, d, np.nextafter(at_t, F(np.inf)), hits)[0].any()
    o2 = o.copy()
    o2[k, 1] = np.nan
    assert nq.closest_mismatches(view, o2, d, None, hits)[0].nonzero()[0].tolist() == [k]
    hits[k] = nq.miss_record(1, nq.BAD_RAY)[0]
    assert not nq.closest_mismatches(view, o2, d, None, hits)[0].any()
