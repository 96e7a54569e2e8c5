"""Encoded outputs on the host (jpt_encode; CPU): the host's copy of the three encoders (jpt_debug_encode with JPT_DEVICE_HOST_ONLY)
against tests/np_encode.py byte for byte, and the restatement itself against oracles it does not share code with -- numpy's float16
conversion, gdpathtracing_amd.hdrio.encode_rgbe, the float64 formula of the RGB9E5 specification and the format's derived error bound
-- then hdrio.save_hdr_rgbe, the refusals that need no device, and the header and bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, hdrio, host

import np_encode as ne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # JPT_E_*
FORMATS = (ne.RGBA16F, ne.RGB9E5, ne.RGBE8)
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099)


@pytest.fixture(scope="module")
def L():
    return capi.lib()


@pytest.fixture(scope="module")
def seeded():
    """2 x 10^6 seeded texels spanning 1e-8 .. 1e6"""
    rng = np.random.default_rng(20251)
    return (10.0 ** rng.uniform(-8.0, 6.0, (2_000_000, 4))).astype(F)


def lib_bits(got, fmt):
    """the library's array as np_encode returns it (the halves as their bits)"""
    return got.view(np.uint16) if fmt == ne.RGBA16F else got


# ---- 1. the host's copy equals the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_host_encode_equals_numpy_byte_for_byte(fmt):
    edge = ne.edge_texels()
    for divisor, alpha_one in ((1.0, False), (3.0, True), (3.0, False)):
        got = host.debug_encode(HOST_ONLY, edge, fmt, divisor, alpha_one)
        assert ne.same_bytes(lib_bits(got, fmt), ne.encode(edge, fmt, divisor, alpha_one)), (divisor, alpha_one)
        assert got.nbytes == len(edge) * ne.TEXEL_BYTES[fmt]
    for n in LENGTHS:
        for divisor in (1.0, 3.0):
            t = ne.texels(n, seed=n)
            got = host.debug_encode(HOST_ONLY, t, fmt, divisor, divisor != 1.0)
            assert ne.same_bytes(lib_bits(got, fmt), ne.encode(t, fmt, divisor, divisor != 1.0)), (n, divisor)


def test_the_divisor_divides_rgb_once_and_alpha_one_writes_one():
    t = np.array([[3.0, 1.0, 7.0, 5.0], [0.1, 0.2, 0.3, 0.25]], F)
    h = host.debug_encode(HOST_ONLY, t, ne.RGBA16F, 3.0, False).astype(F)
    assert np.array_equal(h[:, :3], (t[:, :3] / F(3.0)).astype(np.float16).astype(F)) and np.array_equal(h[:, 3], t[:, 3])
    h1 = host.debug_encode(HOST_ONLY, t, ne.RGBA16F, 3.0, True).astype(F)
    assert np.array_equal(h1[:, 3], [1.0, 1.0]) and np.array_equal(h1[:, :3], h[:, :3])
    # a divisor of 1 touches nothing: a signalling pattern goes through the clamp alone
    assert np.array_equal(host.debug_encode(HOST_ONLY, t, ne.RGBA16F, 1.0, False).astype(F), t.astype(np.float16).astype(F))


# ---- 2. the restatement against independent oracles --------------------------------------------------------------------------------------

def test_half_equals_numpys_conversion_after_the_clamp(seeded):
    for t in (ne.edge_texels(), seeded[:500_000]):
        c = ne.clamp(t, -ne.HALF_MAX, ne.HALF_MAX)
        assert np.array_equal(ne.rgba16f(t), c.astype(np.float16).view(np.uint16))
    edge = ne.rgba16f(ne.edge_texels()[-len(ne.edge_values()):])[:, 0]          # (the rows that hold a value in every channel)
    by_value = dict(zip(ne.edge_values().view(np.uint32).tolist(), edge.tolist()))
    bits = lambda v: int(np.array([v], F).view(np.uint32)[0])
    assert by_value[bits(0.0)] == 0x0000 and by_value[bits(-0.0)] == 0x8000                   # -0 stays -0
    assert by_value[bits(np.nan)] == 0x0000                                                   # NaN -> +0
    assert by_value[bits(np.inf)] == 0x7bff and by_value[bits(-np.inf)] == 0xfbff             # +-inf saturate
    assert by_value[bits(2.0 ** -25)] == 0x0000 and by_value[bits(2.0 ** -25) + 1] == 0x0001   # the tie to even, then its successor
    assert by_value[bits(2.0 ** -24)] == 0x0001 and by_value[bits(2.0 ** -14)] == 0x0400       # subnormal halves are kept
    assert by_value[bits(1.0 + 2.0 ** -11)] == 0x3c00 and by_value[bits(1.0 + 3 * 2.0 ** -11)] == 0x3c02
    assert by_value[bits(65504.0)] == by_value[bits(65520.0)] == by_value[bits(65520.0) - 1] == 0x7bff
    assert by_value[bits(-70000.0)] == 0xfbff


def test_every_half_boundary_rounds_as_numpy_rounds_it():
    """for every finite half and its successor: the midpoint and the float32 just below and just above it"""
    t = half_boundaries()
    assert len(t) > 45_000
    c = ne.clamp(t, -ne.HALF_MAX, ne.HALF_MAX)
    want = c.astype(np.float16).view(np.uint16)
    assert np.array_equal(ne.rgba16f(t), want)
    got = host.debug_encode(HOST_ONLY, t, ne.RGBA16F)
    assert np.array_equal(got.view(np.uint16), want)


def half_boundaries():
    """float32 [n, 4]: for every finite non-negative half h and its successor (the first value past 65504 included: 65536) the
    midpoint, the float32 below it and the float32 above it, then the same negated, packed into channels -- about 1.9 x 10^5 values"""
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(F)
    nxt = np.concatenate([h[1:], np.array([65536.0], F)])
    mid = ((h.astype(np.float64) + nxt.astype(np.float64)) * 0.5).astype(F)                      # exact: 12 significant bits
    assert np.array_equal(mid.astype(np.float64), (h.astype(np.float64) + nxt.astype(np.float64)) * 0.5)
    u = mid.view(np.uint32)
    pos = np.concatenate([mid, (u - 1).view(F), (u + 1).view(F)])
    v = np.concatenate([pos, -pos])
    v = np.concatenate([v, np.zeros((-len(v)) % 4, F)])
    return v.reshape(-1, 4)


def test_rgbe8_equals_hdrio(seeded):
    for t in (ne.edge_texels(), seeded):
        c = ne.clamp(t[:, :3], F(0.0), ne.RGBE8_MAX)                    # (hdrio takes finite, >= 0 input)
        assert np.array_equal(ne.rgbe8(t), hdrio.encode_rgbe(c))
    # the threshold: 1e-32f is encoded, its predecessor is not; 2^127 saturates to its predecessor
    lo = np.zeros((2, 4), F)
    lo[0, 1] = ne.RGBE8_MIN
    lo[1, 1] = ne._next(ne.RGBE8_MIN, -1)
    b = ne.rgbe8(lo)
    assert b[0, 3] != 0 and b[0, 1] >= 128 and not b[1].any()
    hi = np.array([[2.0 ** 127, np.inf, 1.0, 0.0]], F)
    assert np.array_equal(ne.rgbe8(hi), [[255, 255, 0, 255]])
    # exact powers of two: mantissa 128 at exponent byte k + 129
    for k in (-100, -1, 0, 1, 8, 100):
        assert np.array_equal(ne.rgbe8(np.array([[2.0 ** k, 0, 0, 0]], F)), [[128, 0, 0, k + 129]]), k
    # decoding returns each channel to within its cell
    d = ne.decode_rgbe8(ne.rgbe8(seeded[:200_000]))
    c = seeded[:200_000, :3].astype(np.float64)
    step = np.ldexp(1.0, ne.rgbe8(seeded[:200_000])[:, 3].astype(np.int64) - 136)[:, None]
    assert ((d <= c) & (c < d + step)).all()


def test_rgb9e5_equals_the_float64_specification_and_decodes_within_half_a_step(seeded):
    w = ne.rgb9e5(seeded)
    q, e = ne.unpack_rgb9e5(w)
    q64, e64 = ne.rgb9e5_spec64(seeded)
    mismatches = int((q != q64).any(axis=1).sum() + (e != e64).sum())
    print("RGB9E5 float32 form against the float64 formula: %d mismatches of %d texels" % (mismatches, len(seeded)))
    assert mismatches == 0
    assert (q <= 511).all() and (e >= 0).all() and (e <= 31).all()
    # the derived bound, on the seeded set and on the edge list: half a step plus the one rounding of x + 0.5f for x < 512
    for t in (seeded, ne.edge_texels()):
        w = ne.rgb9e5(t)
        _, e = ne.unpack_rgb9e5(w)
        c = ne.clamp(t[:, :3], F(0.0), ne.RGB9E5_MAX).astype(np.float64)
        err = np.abs(ne.decode_rgb9e5(w) - c)
        bound = (0.5 + 2.0 ** -16) * np.ldexp(1.0, e - 24)[:, None]
        print("RGB9E5 decoded error: worst %.6f of a step" % float((err / np.ldexp(1.0, e - 24)[:, None]).max()))
        assert (err <= bound).all()
    # planted: the largest value and its successor, the carry, zero, NaN and negatives
    one = lambda *rgb: int(ne.rgb9e5(np.array([list(rgb) + [0.0]], F))[0])
    assert one(65408.0, 0, 0) == one(65409.0, 0, 0) == one(np.inf, 0, 0) == (31 << 27) | 511
    assert one(0.9995, 0, 0) == (16 << 27) | 256 and one(0.5, 0, 0) == (15 << 27) | 256
    assert one(0, 0, 0) == one(np.nan, -1.0, -np.inf) == 0
    assert one(2.0 ** -16, 0, 0) == (0 << 27) | 256 and one(2.0 ** -25 * 1.5, 0, 0) == 1 and one(2.0 ** -26, 0, 0) == 0
    assert one(1.0, 0.5, 0.25) == (16 << 27) | 256 | (128 << 9) | (64 << 18)


# ---- 3. hdrio.save_hdr_rgbe --------------------------------------------------------------------------------------------------------------

def test_save_hdr_rgbe_writes_encoded_texels_unchanged(tmp_path):
    rng = np.random.default_rng(3)
    rgb = (10.0 ** rng.uniform(-3.0, 3.0, (5, 12, 3))).astype(F)
    rgb[1, 2:9] = 0.25                                                   # a run for the run-length scanlines
    a, b = str(tmp_path / "a.hdr"), str(tmp_path / "b.hdr")
    for rle in (True, False):
        hdrio.save_hdr(a, rgb, rle)
        texels = np.concatenate([rgb, np.ones((5, 12, 1), F)], axis=2).reshape(-1, 4)
        enc = host.debug_encode(HOST_ONLY, texels, ne.RGBE8).reshape(5, 12, 4)        # what a JPT_ENCODE_RGBE8 read-back holds
        hdrio.save_hdr_rgbe(b, enc, rle)
        assert open(a, "rb").read() == open(b, "rb").read(), rle
        assert np.array_equal(hdrio.load_hdr(b), hdrio.decode_rgbe(enc))
    for bad in (rgb, np.zeros((5, 12, 4), F), np.zeros((60, 4), np.uint8)):
        with pytest.raises(ValueError):
            hdrio.save_hdr_rgbe(b, bad)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_the_debug_call_checks_its_arguments(L):
    t, out = np.ones((4, 4), F), np.zeros(32, np.uint8)
    D = L.jpt_debug_encode
    assert D(HOST_ONLY, t.ctypes.data, 4, 1.0, 0, 0, out.ctypes.data) == E_INVALID and b"format" in L.jpt_debug_last_error()
    assert D(HOST_ONLY, t.ctypes.data, 4, 1.0, 0, 4, out.ctypes.data) == E_INVALID
    for divisor in (0.0, -1.0, np.inf, np.nan):
        assert D(HOST_ONLY, t.ctypes.data, 4, divisor, 0, ne.RGBE8, out.ctypes.data) == E_INVALID
        assert b"jpt_debug_encode" in L.jpt_debug_last_error() and b"divisor" in L.jpt_debug_last_error()
    assert D(HOST_ONLY, None, 4, 1.0, 0, ne.RGBE8, out.ctypes.data) == E_INVALID
    assert D(HOST_ONLY, t.ctypes.data, 4, 1.0, 0, ne.RGBE8, None) == E_INVALID
    assert D(HOST_ONLY, t.ctypes.data, (1 << 30) + 1, 1.0, 0, ne.RGBE8, out.ctypes.data) == E_LIMIT
    assert D(HOST_ONLY, None, 0, 1.0, 0, ne.RGBE8, None) == capi.OK                       # no texels: nothing is touched
    out[:] = 0xee
    assert D(HOST_ONLY, t.ctypes.data, 4, 1.0, 0, ne.RGBE8, out.ctypes.data) == capi.OK
    assert (out[:16].reshape(4, 4) == [128, 128, 128, 129]).all() and (out[16:] == 0xee).all()   # 4 B per texel and no more
    with pytest.raises(capi.JptError, match="format"):
        host.debug_encode(HOST_ONLY, t, 7)
    assert host.debug_encode(HOST_ONLY, np.zeros((0, 4), F), ne.RGB9E5).shape == (0,)


def test_a_host_only_context_checks_the_arguments_and_then_has_no_device(L):
    ctx = host.Context(HOST_ONLY)
    try:
        def refused(rc, code, *words):
            assert rc == code, (rc, ctx.last_error())
            for w in words:
                assert w in ctx.last_error(), ctx.last_error()

        M, R, S = capi.ENCODE_SOURCE_MEAN, capi.ENCODE_SOURCE_REFLECTION, capi.ENCODE_SOURCE_PROBE_SH
        refused(L.jpt_encode(ctx.h, -1, 0, ne.RGBE8), E_INVALID, "jpt_encode", "source")
        refused(L.jpt_encode(ctx.h, 6, 0, ne.RGBE8), E_INVALID, "jpt_encode", "source")
        refused(L.jpt_encode(ctx.h, M, 0, 0), E_INVALID, "jpt_encode", "format")
        refused(L.jpt_encode(ctx.h, M, 0, 4), E_INVALID, "jpt_encode", "format")
        for fmt in (ne.RGB9E5, ne.RGBE8):
            refused(L.jpt_encode(ctx.h, S, 0, fmt), E_INVALID, "jpt_encode", "signed")
        for source in (M, capi.ENCODE_SOURCE_DENOISED, capi.ENCODE_SOURCE_DISPLAY, capi.ENCODE_SOURCE_LIGHTMAP, S):
            refused(L.jpt_encode(ctx.h, source, 1, ne.RGBA16F), E_INVALID, "jpt_encode", "level")
            refused(L.jpt_encode(ctx.h, source, capi.ENCODE_ALL_LEVELS, ne.RGBA16F), E_INVALID, "jpt_encode", "level")
        refused(L.jpt_encode(ctx.h, R, -2, ne.RGBA16F), E_INVALID, "jpt_encode", "level")
        for source in range(6):
            refused(L.jpt_encode(ctx.h, source, 0, ne.RGBA16F), E_DEVICE, "jpt_encode", "host-only")
        refused(L.jpt_encode(ctx.h, R, capi.ENCODE_ALL_LEVELS, ne.RGB9E5), E_DEVICE, "jpt_encode")
        info, out, n, ms = capi.EncodedInfo(), np.zeros(64, np.uint8), C.c_size_t(7), C.c_float(0)
        refused(L.jpt_get_encoded_info(ctx.h, None), E_INVALID, "jpt_get_encoded_info")
        refused(L.jpt_get_encoded_info(ctx.h, C.byref(info)), E_DEVICE, "jpt_get_encoded_info")
        refused(L.jpt_read_encoded(ctx.h, None, 64), E_INVALID, "jpt_read_encoded")
        refused(L.jpt_read_encoded(ctx.h, out.ctypes.data, 64), E_DEVICE, "jpt_read_encoded")
        refused(L.jpt_readback_encoded_begin(ctx.h), E_DEVICE, "jpt_readback_encoded_begin")
        refused(L.jpt_readback_encoded_end(ctx.h, None, 64), E_INVALID, "jpt_readback_encoded_end")
        refused(L.jpt_readback_encoded_end(ctx.h, out.ctypes.data, 64), E_STATE, "jpt_readback_encoded_end", "no read-back in flight")
        refused(L.jpt_get_encode_timing(ctx.h, None), E_INVALID, "jpt_get_encode_timing")
        refused(L.jpt_get_encode_timing(ctx.h, C.byref(ms)), E_DEVICE, "jpt_get_encode_timing")
        assert L.jpt_device_encoded(ctx.h, C.byref(n)) is None and n.value == 0
        with pytest.raises(capi.JptError, match="jpt_encode"):
            ctx.encode(M, ne.RGBE8)
        with pytest.raises(capi.JptError, match="jpt_get_encoded_info"):
            ctx.read_encoded()
    finally:
        ctx.close()
    assert L.jpt_encode(None, 0, 0, 1) == E_INVALID and L.jpt_get_encoded_info(None, None) == E_INVALID
    assert L.jpt_read_encoded(None, None, 0) == E_INVALID and L.jpt_readback_encoded_begin(None) == E_INVALID
    assert L.jpt_readback_encoded_end(None, None, 0) == E_INVALID and L.jpt_get_encode_timing(None, None) == E_INVALID
    assert L.jpt_device_encoded(None, None) is None


# ---- 5. the header and the bindings -----------------------------------------------------------------------------------------------------

def test_the_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for proto in (
            r"typedef enum \{ JPT_ENCODE_RGBA16F = 1, JPT_ENCODE_RGB9E5 = 2, JPT_ENCODE_RGBE8 = 3 \} jpt_encode_format;",
            r"typedef enum \{ JPT_ENCODE_SOURCE_MEAN = 0, JPT_ENCODE_SOURCE_DENOISED = 1, JPT_ENCODE_SOURCE_DISPLAY = 2,\s+JPT_ENCODE_SOURCE_LIGHTMAP = 3, "
            r"JPT_ENCODE_SOURCE_REFLECTION = 4, JPT_ENCODE_SOURCE_PROBE_SH = 5 \} jpt_encode_source;",
            r"#define JPT_ENCODE_ALL_LEVELS \(-1\)",
            r"typedef struct \{ int32_t source, format, level, width, height; uint64_t n_texels, bytes; \} jpt_encoded_info;",
            r"int\s+jpt_encode\(jpt_ctx \*ctx, int32_t source, int32_t level, int32_t format\);",
            r"int\s+jpt_get_encoded_info\(jpt_ctx \*ctx, jpt_encoded_info \*out\);",
            r"int\s+jpt_read_encoded\(jpt_ctx \*ctx, void \*out, size_t capacity\);",
            r"int\s+jpt_readback_encoded_begin\(jpt_ctx \*ctx\);",
            r"int\s+jpt_readback_encoded_end\(jpt_ctx \*ctx, void \*out, size_t capacity\);",
            r"void \*jpt_device_encoded\(jpt_ctx \*ctx, size_t \*bytes_out\);",
            r"int\s+jpt_get_encode_timing\(jpt_ctx \*ctx, float \*ms\);",
            r"int jpt_debug_encode\(int device_id, const float \*src4, uint64_t n_texels, float divisor, int32_t alpha_one, int32_t format, void \*out\);"):
        assert re.search(proto, text), proto
    assert re.search(r"#define JPT_ABI_VERSION 6\b", text) and capi.lib().jpt_abi_version() == 6
    assert C.sizeof(capi.EncodedInfo) == 40
    assert (capi.ENCODE_RGBA16F, capi.ENCODE_RGB9E5, capi.ENCODE_RGBE8) == (ne.RGBA16F, ne.RGB9E5, ne.RGBE8) == (1, 2, 3)
    assert (capi.ENCODE_SOURCE_MEAN, capi.ENCODE_SOURCE_DENOISED, capi.ENCODE_SOURCE_DISPLAY, capi.ENCODE_SOURCE_LIGHTMAP,
            capi.ENCODE_SOURCE_REFLECTION, capi.ENCODE_SOURCE_PROBE_SH) == tuple(range(6)) and capi.ENCODE_ALL_LEVELS == -1
    for name in ("jpt_encode", "jpt_get_encoded_info", "jpt_read_encoded", "jpt_readback_encoded_begin", "jpt_readback_encoded_end",
                 "jpt_device_encoded", "jpt_get_encode_timing", "jpt_debug_encode"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert not hasattr(capi.lib(), "jpt_multi_encode")
    hpp = open(os.path.join(ROOT, "include", "jpt_host.hpp")).read()
    for name in ("encode", "encoded_info", "read_encoded", "readback_encoded_begin", "readback_encoded_end", "device_encoded", "encode_timing"):
        assert hasattr(host.Context, name), name
        assert re.search(r"\b%s\(" % name, hpp), name
    assert hasattr(host, "debug_encode") and hasattr(hdrio, "save_hdr_rgbe")
    assert [capi.encoded_array(f, 3).dtype for f in FORMATS] == [np.float16, np.uint32, np.uint8]
    assert [capi.encoded_array(f, 3).nbytes for f in FORMATS] == [24, 12, 12]
    # the kernels and the host loop include the one header the arithmetic lives in
    csrc = os.path.join(ROOT, "gdpathtracing_amd", "csrc")
    for name in ("jpt_kernels_encode.hip", "jpt_debug.hip", "jpt_encode.cpp"):
        assert '#include "jpt_encode.h"' in open(os.path.join(csrc, name)).read(), name
    assert "cvt_pkrtz" not in open(os.path.join(csrc, "jpt_encode.h")).read() + open(os.path.join(csrc, "jpt_kernels_encode.hip")).read()
