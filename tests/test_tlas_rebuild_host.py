"""jpt_scene_rebuild_tlas on the host: the template and the host form of the sort against their numpy restatement
(tests/np_tlas_rebuild.py), the declarations, and the state and argument checks, which run before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_tlas_rebuild as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4
TEMPLATE_COUNTS = list(range(2, 301)) + [1024, 1025, 4096, 4097, 32767]


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for name, value in (("INVALID", E_INVALID), ("DEVICE", E_DEVICE), ("STATE", E_STATE), ("LIMIT", E_LIMIT)):
        assert re.search(r"JPT_E_%s\s*=\s*%d\b" % (name, value), text), name


def test_template_is_numpys_and_well_formed(hiplib):
    for n in TEMPLATE_COUNTS:
        t = host.debug_tlas_template(n)
        child, levels = ref.template(n)
        assert np.array_equal(t["child"], child), n
        R = len(child)
        assert R <= n - 1, n
        assert t["n_levels"] == levels == ref.ceil_log4(n), n
        assert t["stack_need"] == ref.stack_need(child) <= 3 * levels, n
        # every position in exactly one leaf slot
        leaves = child[(child < 0) & (child != ref.EMPTY)]
        assert np.array_equal(np.sort(~leaves), np.arange(n)), n
        # breadth first: the internal references, read record by record and slot by slot, count 1, 2, 3, ...; every record but
        # the root has one parent; every record two children or more, empty slots last
        internal = child[child >= 0]
        assert np.array_equal(internal, np.arange(1, R)), n
        used = child != ref.EMPTY
        assert (used.sum(axis=1) >= 2).all(), n
        assert (used[:, :-1] >= used[:, 1:]).all(), n


def test_template_refuses_counts_it_does_not_cover(hiplib):
    L = capi.lib()
    for n in (0, 1, 32768):
        assert L.jpt_debug_tlas_template(n, None, 0, None, None, None) == E_INVALID
    nr = C.c_uint32()
    child = np.zeros((1, 4), np.int32)
    assert L.jpt_debug_tlas_template(9, child.ctypes.data_as(C.c_void_p), 1, C.byref(nr), None, None) == E_INVALID
    assert nr.value == 5   # 9 = 3 + 2 + 2 + 2: the root and four records below it


def order_cases():
    rng = np.random.RandomState(11)
    cases = {}
    for n in (2, 3, 17, 300, 5000):
        lo = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
        cases["seeded%d" % n] = (lo, lo + rng.uniform(0, 3, (n, 3)).astype(np.float32))
    one = np.tile(np.float32([1, 2, 3]), (40, 1))
    cases["all_equal"] = (one, one + np.float32(1))
    for flat in ((0,), (0, 2), (0, 1, 2)):
        lo = rng.uniform(-5, 5, (70, 3)).astype(np.float32)
        hi = lo + rng.uniform(0, 1, (70, 3)).astype(np.float32)
        for k in flat:
            lo[:, k], hi[:, k] = np.float32(0.25), np.float32(0.75)
        cases["flat" + "".join("xyz"[k] for k in flat)] = (lo, hi)
    lo = rng.uniform(-5, 5, (33, 3)).astype(np.float32)
    hi = lo + np.float32(1)
    lo[3], hi[3] = np.float32(3e38), np.float32(3e38)        # the centre overflows to +inf
    lo[4], hi[4] = np.float32(-3e38), np.float32(-3e38)
    lo[5, 1], hi[5, 1] = np.float32(np.nan), np.float32(np.nan)
    lo[6], hi[6] = np.float32(np.nan), np.float32(1)
    lo[7], hi[7] = np.float32(-np.inf), np.float32(np.inf)   # inf - inf
    cases["non_finite"] = (lo, hi)
    cases["all_nan"] = (np.full((9, 3), np.nan, np.float32), np.full((9, 3), np.nan, np.float32))
    # finite centres whose extent overflows: (c - bmin) * 0 is NaN for the far one, cell 0
    lo = np.float32([[-3e38] * 3, [3e38] * 3, [0, 0, 0]])
    cases["extent_overflow"] = (lo, lo.copy())
    cases["two"] = (np.float32([[1, 0, 0], [0, 0, 0]]), np.float32([[2, 1, 1], [1, 1, 1]]))
    return cases


ORDER_CASES = order_cases()


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_host_order_is_numpys(hiplib, name):
    lo, hi = ORDER_CASES[name]
    keys, order = host.debug_tlas_order(-1, lo, hi)
    want_keys, want_order = ref.order(lo, hi)
    assert np.array_equal(keys, want_keys)
    assert np.array_equal(order, want_order)
    assert (keys >> np.uint64(45) == 0).all() and len(np.unique(keys)) == len(keys)
    _, order_only = host.debug_tlas_order(-1, lo, hi, with_keys=False)
    assert np.array_equal(order_only, want_order)


def test_non_finite_boxes_fall_into_cell_zero(hiplib):
    lo, hi = ORDER_CASES["non_finite"]
    keys, _ = host.debug_tlas_order(-1, lo, hi)
    assert (keys[[3, 4, 6, 7]] >> np.uint64(15) == 0).all()
    lo, hi = ORDER_CASES["all_equal"]
    keys, order = host.debug_tlas_order(-1, lo, hi)
    assert (keys >> np.uint64(15) == 0).all() and np.array_equal(order, np.arange(len(lo)))   # the index breaks the tie


def test_order_argument_checks(hiplib):
    L = capi.lib()
    out = np.zeros(4, np.uint32)
    box = np.zeros((4, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.jpt_debug_tlas_order(-1, None, p(box), 4, None, p(out)) == E_INVALID
    assert L.jpt_debug_tlas_order(-1, p(box), p(box), 4, None, None) == E_INVALID
    assert L.jpt_debug_tlas_order(-1, p(box), p(box), 32768, None, p(out)) == E_LIMIT
    assert L.jpt_debug_tlas_order(-1, None, None, 0, None, None) == 0


def test_header_declares_the_calls_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for decl in (r"int jpt_scene_rebuild_tlas\(jpt_ctx \*ctx, const float \*transforms12, uint32_t n_instances\);",
                 r"int jpt_multi_rebuild_tlas\(jpt_multi \*m, const float \*transforms12, uint32_t n_instances\);",
                 r"int jpt_debug_tlas_order\(int device_id, const float \*lo3, const float \*hi3, uint32_t n, uint64_t \*keys_out, uint32_t \*sorted_instances_out\);",
                 r"int jpt_debug_tlas_template\(uint32_t n, int32_t \*child_out, uint32_t capacity, uint32_t \*n_records, uint32_t \*n_levels, uint32_t \*stack_need\);",
                 r"int jpt_debug_tlas_records\(jpt_ctx \*ctx, void \*nodes4_out, void \*nodesq_out, uint32_t capacity, uint32_t \*n_records, int32_t \*root_out,\s+float \*inst_lo3, float \*inst_hi3\);"):
        assert re.search(decl, text), decl
    assert "#define JPT_ABI_VERSION 6" in text


def test_abi_version_is_six(hiplib):
    assert capi.lib().jpt_abi_version() == 6


def _both(ctx, t12, n):
    """(code, message) of the refit and of the rebuild for the same arguments"""
    out = []
    for name in ("jpt_scene_refit_tlas", "jpt_scene_rebuild_tlas"):
        rc = getattr(ctx._lib, name)(ctx.h, None if t12 is None else t12.ctypes.data_as(C.c_void_p), n)
        msg = ctx._lib.jpt_last_error(ctx.h)
        out.append((rc, (msg.decode() if msg else "").replace(name, "CALL")))
    return out


def test_state_errors_match_the_refits_on_a_host_only_context(hiplib):
    sc = scenes.demo_scene(n_tris=256)
    t12 = np.stack([np.asarray(i.transform, np.float32).reshape(12) for i in sc.instances])
    n = len(sc.instances)
    # nothing committed
    ctx = host.Context(-1)
    a, b = _both(ctx, t12, n)
    assert a == b and a[0] == E_STATE and "needs a scene made by jpt_scene_commit" in a[1]
    ctx.close()
    # a reference-exact commit: not the native records
    ctx = host.Context(-1)
    ctx.build_scene(sc, capi.BUILD_REFERENCE_EXACT)
    a, b = _both(ctx, t12, n)
    assert a == b and a[0] == E_STATE
    ctx.close()
    for builder in (capi.BUILD_SAH, capi.BUILD_SAH_WATERTIGHT):
        ctx = host.Context(-1)
        ctx.build_scene(sc, builder)
        a, b = _both(ctx, None, n)
        assert a == b and a[0] == E_INVALID and "null transforms" in a[1]
        a, b = _both(ctx, t12, n - 1)
        assert a == b and a[0] == E_INVALID and "one transform per instance" in a[1]
        a, b = _both(ctx, t12, n)
        assert a == b and a[0] == E_DEVICE and "host-only" in a[1]
        ctx.update_tlas()   # the host's copy of the scene stays usable (nothing ran)
        ctx.close()
    assert capi.lib().jpt_scene_rebuild_tlas(None, None, 0) == E_INVALID
    assert capi.lib().jpt_multi_rebuild_tlas(None, None, 0) == E_INVALID
    assert capi.lib().jpt_debug_tlas_records(None, None, None, 0, None, None, None, None) == E_INVALID


def test_python_wrappers_reach_the_calls(hiplib):
    sc = scenes.demo_scene(n_tris=256)
    ctx = host.Context(-1)
    ctx.build_scene(sc, capi.BUILD_SAH)
    t12 = np.stack([np.asarray(i.transform, np.float32).reshape(12) for i in sc.instances])
    with pytest.raises(capi.JptError, match="jpt_scene_rebuild_tlas failed .*host-only"):
        ctx.rebuild_tlas(t12)
    with pytest.raises(capi.JptError, match="jpt_debug_tlas_records failed .*host-only"):
        ctx.debug_tlas_records(len(sc.instances))
    assert hasattr(host.MultiContext, "rebuild_tlas")
    ctx.close()
