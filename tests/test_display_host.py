"""jpt_display without a GPU: the C ABI's refusals on a host-only context, the host form of the transform (jpt_debug_display, device
-1) against the float32 numpy restatement bit for bit, the sRGB table, properties of the restatement itself, and the register
budgets of the new kernels in the cross-compiled ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_denoise as ndn
import np_display as nd

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def debug_display(L, device, image, want_f32=True, want_rgba8=True, **fields):
    h, w = image.shape[:2]
    image = np.ascontiguousarray(image, F)
    out = np.zeros((h, w, 4), F) if want_f32 else None
    ldr = np.zeros((h, w, 4), np.uint8) if want_rgba8 else None
    rc = L.jpt_debug_display(device, w, h, C.byref(capi.DisplayParams(**fields)) if fields else None, image.ctypes.data,
                             None if out is None else out.ctypes.data, None if ldr is None else ldr.ctypes.data)
    assert rc == 0, "jpt_debug_display(device %d) = %d" % (device, rc)
    return out, ldr


def library_table(L):
    t = np.zeros(255, F)
    assert L.jpt_debug_display_srgb_table(t.ctypes.data) == 0
    return t


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

BAD = [("source", -1), ("source", 2), ("tonemap", -1), ("tonemap", 3), ("transfer", -1), ("transfer", 2), ("bloom_levels", -1), ("bloom_levels", 7),
       ("exposure", -0.5), ("exposure", float("nan")), ("exposure", float("inf")), ("white", 0.0), ("white", -1.0), ("white", float("nan")),
       ("white", float("inf")), ("bloom_threshold", -1.0), ("bloom_threshold", float("nan")), ("bloom_threshold", float("inf")),
       ("bloom_strength", -1.0), ("bloom_strength", float("nan")), ("bloom_strength", float("inf"))]


def test_refusals_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_display_params
        for field, value in BAD:
            assert S(ctx.h, C.byref(capi.DisplayParams(**{field: value}))) == E_INVALID, (field, value)
            msg = L.jpt_last_error(ctx.h)
            assert b"jpt_display_params" in msg and field.encode() in msg, msg     # each bad parameter is named
        for good in (dict(exposure=0.0), dict(bloom_threshold=0.0), dict(bloom_strength=0.0), dict(bloom_levels=6), dict()):
            assert S(ctx.h, C.byref(capi.DisplayParams(**good))) == E_DEVICE, good    # checks passed: no device
        assert S(ctx.h, None) == E_DEVICE
        assert S(None, None) == E_INVALID and L.jpt_display(None) == E_INVALID
        # the state errors that need no device come before the device is asked for, in jpt_denoise's order
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        ctx.set_debug_steps(True)
        ctx.set_partition(1, 2)
        assert L.jpt_display(ctx.h) == E_STATE and b"JPT_DENOISE_PROGRESSIVE" in L.jpt_last_error(ctx.h)
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        assert L.jpt_display(ctx.h) == E_STATE and b"DEBUG_STEPS" in L.jpt_last_error(ctx.h)
        ctx.set_debug_steps(False)
        assert L.jpt_display(ctx.h) == E_STATE and b"whole image on one context" in L.jpt_last_error(ctx.h)
        ctx.set_partition(0, 1)
        assert L.jpt_display(ctx.h) == E_DEVICE and b"host-only" in L.jpt_last_error(ctx.h)
        out = np.zeros(4, F)
        assert L.jpt_read_display_f32(ctx.h, None) == E_INVALID and L.jpt_read_display_rgba8(ctx.h, None) == E_INVALID
        assert L.jpt_read_display_f32(ctx.h, out.ctypes.data) == E_DEVICE
        assert L.jpt_read_display_rgba8(ctx.h, out.ctypes.data) == E_DEVICE
        with pytest.raises(capi.JptError, match="host-only"):
            ctx.display()
    finally:
        ctx.close()


def test_debug_display_checks_its_arguments(L):
    img = nd.synthetic_image(8, 8)
    out, ldr = np.zeros((8, 8, 4), F), np.zeros((8, 8, 4), np.uint8)
    D = L.jpt_debug_display
    assert D(HOST_ONLY, 0, 8, None, img.ctypes.data, out.ctypes.data, ldr.ctypes.data) == E_INVALID
    assert D(HOST_ONLY, 8, 65537, None, img.ctypes.data, out.ctypes.data, ldr.ctypes.data) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, None, out.ctypes.data, ldr.ctypes.data) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, img.ctypes.data, None, None) == E_INVALID
    for field, value in BAD:
        assert D(HOST_ONLY, 8, 8, C.byref(capi.DisplayParams(**{field: value})), img.ctypes.data, out.ctypes.data, ldr.ctypes.data) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, img.ctypes.data, out.ctypes.data, ldr.ctypes.data) == 0
    assert L.jpt_debug_display_srgb_table(None) == E_INVALID
    # either output alone
    both = debug_display(L, HOST_ONLY, img, bloom_levels=2)
    assert nd.same_bits(debug_display(L, HOST_ONLY, img, want_rgba8=False, bloom_levels=2)[0], both[0]).all()
    assert np.array_equal(debug_display(L, HOST_ONLY, img, want_f32=False, bloom_levels=2)[1], both[1])


# ---- 2. the host form equals the restatement -----------------------------------------------------------------------------------

SIZES = [(1, 1), (2, 3), (97, 61), (256, 144)]
GRADE = dict(exposure=1.7, white=3.0, bloom_threshold=0.8, bloom_strength=0.6)


def check_against_restatement(L, device, w, h, seed, **fields):
    img = nd.synthetic_image(w, h, seed)
    got = debug_display(L, device, img, **fields)
    want = nd.display(img, 1, **fields)
    bad = ~nd.same_bits(got[0], want[0])
    assert not bad.any(), "%dx%d %s: %d values differ, first %s" % (w, h, fields, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    bad = got[1] != want[1]
    assert not bad.any(), "%dx%d %s: %d codes differ, first %s" % (w, h, fields, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (got[0][..., 3] == 1).all() and (got[1][..., 3] == 255).all()


@pytest.mark.parametrize("levels", range(7))
def test_host_transform_equals_the_numpy_restatement_bit_for_bit(L, levels):
    """every size, tone map and transfer with N levels, on seeded images with NaN, +-inf, zeros, negative values and values up to 1e6"""
    for w, h in SIZES:
        for tonemap in (nd.ACES_REF, nd.REINHARD, nd.CLAMP):
            for transfer in (nd.LINEAR, nd.SRGB):
                check_against_restatement(L, HOST_ONLY, w, h, w + levels, bloom_levels=levels, tonemap=tonemap, transfer=transfer, **GRADE)


def test_host_transform_with_the_defaults_and_the_parameter_extremes(L):
    img = nd.synthetic_image(40, 30, 9)
    got = debug_display(L, HOST_ONLY, img)                  # NULL parameters: the defaults are the library's
    want = nd.display(img, 1)
    assert nd.same_bits(got[0], want[0]).all() and np.array_equal(got[1], want[1])
    for fields in (dict(exposure=0.0, bloom_levels=3), dict(bloom_threshold=0.0, bloom_levels=6, bloom_strength=0.0),
                   dict(exposure=1e30, tonemap=nd.REINHARD, white=1e30, bloom_levels=2, transfer=nd.SRGB),
                   dict(exposure=1e-30, white=1e-30, tonemap=nd.REINHARD, transfer=nd.SRGB, bloom_levels=1, bloom_threshold=1e-35),
                   dict(source=capi.DISPLAY_SOURCE_DENOISED, bloom_levels=4)):
        check_against_restatement(L, HOST_ONLY, 67, 45, 3, **fields)


# ---- 3. the sRGB table ----------------------------------------------------------------------------------------------------------

def test_srgb_table_is_the_definition_and_codes_are_its_search(L):
    t = library_table(L)
    assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] < 1
    e = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    exact = np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)
    ulp = np.spacing(exact.astype(F)).astype(np.float64)
    assert (np.abs(t.astype(np.float64) - exact) <= ulp).all()
    # the codes of values at, just under and just over every entry, of 0, 1 and a ramp: np.searchsorted on the library's own table
    v = np.concatenate([t, np.nextafter(t, F(0)), np.nextafter(t, F(2)), np.array([0.0, 1.0], F), np.linspace(0, 1, 4001).astype(F)]).astype(F)
    img = np.zeros((1, len(v), 4), F)
    img[0, :, 0] = img[0, :, 1] = img[0, :, 2] = v
    out, ldr = debug_display(L, HOST_ONLY, img, tonemap=nd.CLAMP, transfer=nd.SRGB)
    assert nd.same_bits(out[0, :, 0], v).all()
    want = np.searchsorted(t, v, side="right")
    assert np.array_equal(ldr[0, :, 0], want) and np.array_equal(ldr[0, :, 2], want)
    assert ldr[0, len(t) * 3, 0] == 0 and ldr[0, len(t) * 3 + 1, 0] == 255
    # ... which is the nearest code of the encoded value: |oetf(v) * 255 - code| <= 0.5 (+ float64 rounding)
    v64 = v.astype(np.float64)
    enc = np.where(v64 <= 0.0031308, v64 * 12.92, 1.055 * v64 ** (1 / 2.4) - 0.055) * 255.0
    assert (np.abs(enc - want) <= 0.5 + 1e-3).all()


# ---- 4. properties of the restatement -------------------------------------------------------------------------------------------

def test_defaults_reproduce_the_reference_display_function():
    """with the default parameters the codes are np_denoise's unorm8(ACES(.)) of the same means"""
    rng = np.random.default_rng(5)
    mean = np.zeros((64, 96, 4), F)
    mean[..., :3] = (rng.random((64, 96, 3)) * 10.0 ** rng.uniform(-3, 2, (64, 96, 1))).astype(F)
    mean[3, 4, 0], mean[5, 6, 1], mean[7, 8, 2], mean[9, 9, :3] = np.nan, np.inf, -np.inf, 0.0
    assert np.array_equal(nd.display(mean, 1)[1], ndn.display(mean))
    acc = (mean * F(7)).astype(F)
    with np.errstate(all="ignore"):
        m7 = (acc / F(7)).astype(F)
    assert np.array_equal(nd.display(acc, 7)[1], ndn.display(m7))


@pytest.mark.parametrize("levels", range(1, 7))
def test_a_uniform_image_blooms_by_exactly_the_strength(levels):
    """2.0 everywhere, threshold 1: the luminance is exactly 2, B = 2 * ((2 - 1) / 2) = 1, every level of the pyramid is exactly 1
    (the weights are dyadic and sum to 1, clamped taps included), U_1 = N and bloom * (strength / N) = strength: o = 2 + strength
    at every pixel and every N, border pixels included.  Strengths s with s / N exact, i.e. the composite scale s / N times the N
    levels gives s back."""
    img = np.full((37, 53, 4), 2.0, F)
    for s in (0.25, 1.0):
        strength = F(s) * F(levels)           # (so the composite scale strength / N is s exactly)
        o = nd.composite(img, 1, bloom_levels=levels, bloom_threshold=1.0, bloom_strength=strength)
        assert (o == F(2.0) + strength).all()
        o = nd.composite(img, 1, bloom_levels=levels, bloom_threshold=1.0, bloom_strength=s * 0.5)
        if levels in (1, 2, 4):               # s / N exact
            assert (o == F(2.0) + F(s * 0.5)).all()


def test_a_single_bright_pixel_blooms_symmetrically_and_keeps_its_energy():
    n, levels = 255, 4                      # odd: the pixel sits on the centre; 4 levels reach +-47 pixels, far from the border
    img = np.zeros((n, n, 4), F)
    img[n // 2, n // 2, :3] = (40.0, 20.0, 10.0)
    c = nd.base(img, 1, 1.0)
    b = nd.bright(c, 1.0)[n // 2, n // 2]
    assert (b > 0).all()
    bl = nd.bloom(c, levels, 1.0)
    assert (bl >= 0).all()
    # every level conserves the sum (the down weights sum to 1 per source pixel over the outputs it feeds, up to the factor 4 of the
    # halving, the tent's likewise): the bloom sums to N times B's sum, each of the N levels carrying it once
    total = bl.astype(np.float64).sum((0, 1))
    assert np.allclose(total, levels * b.astype(np.float64), rtol=1e-5, atol=0)
    assert (bl[0] == 0).all() and (bl[-1] == 0).all() and (bl[:, 0] == 0).all() and (bl[:, -1] == 0).all()     # no tap clamped
    # a pixel on the diagonal of a square canvas: symmetric under transposition (rows and columns are summed in another order, so
    # to float rounding; where one side is 0 the other is)
    assert np.allclose(bl, bl.transpose(1, 0, 2), rtol=1e-5, atol=0)
    # a pixel is not centred on the coarser grids; the 2 x 2 block about the centre of a 256 x 256 canvas is, at every level: its
    # bloom is symmetric under both mirrors and the transposition
    img = np.zeros((256, 256, 4), F)
    img[127:129, 127:129, :3] = (40.0, 20.0, 10.0)
    bl = nd.bloom(nd.base(img, 1, 1.0), levels, 1.0)
    assert (bl >= 0).all() and (bl[0] == 0).all() and (bl[:, 0] == 0).all()
    for other in (bl[::-1], bl[:, ::-1], bl.transpose(1, 0, 2)):
        assert np.allclose(bl, other, rtol=1e-5, atol=0)


def test_one_nan_pixel_leaves_every_other_pixel_finite():
    rng = np.random.default_rng(11)
    img = np.zeros((48, 64, 4), F)
    img[..., :3] = (rng.random((48, 64, 3)) * 4.0).astype(F)
    clean = nd.composite(img, 1, bloom_levels=5, bloom_threshold=0.5, bloom_strength=1.0)
    for bad in (np.nan, np.inf, -np.inf):
        dirty_img = img.copy()
        dirty_img[20, 30, 1] = bad
        dirty = nd.composite(dirty_img, 1, bloom_levels=5, bloom_threshold=0.5, bloom_strength=1.0)
        mask = np.ones((48, 64), bool)
        mask[20, 30] = False
        assert np.isfinite(dirty[mask]).all()
        # ... and what reaches them is what a black pixel in its place would have sent
        black = img.copy()
        black[20, 30, :3] = 0.0
        assert np.array_equal(dirty[mask], nd.composite(black, 1, bloom_levels=5, bloom_threshold=0.5, bloom_strength=1.0)[mask])
        out, ldr = nd.display(dirty_img, 1, bloom_levels=5, bloom_threshold=0.5, bloom_strength=1.0, tonemap=nd.REINHARD, transfer=nd.SRGB)
        assert np.isfinite(out).all()
    assert np.isfinite(clean).all()


# ---- 5. register budgets ---------------------------------------------------------------------------------------------------------

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body).  The budget is
# eight waves per SIMD: at most 64 VGPRs, no scratch.  First compile: down0 19, down 62 (two rows of four 16-byte gathers in flight;
# with all sixteen unrolled it took 68), up 28, resolve with bloom 28, resolve without 13.  The four small ones get their first
# figure plus a quarter; the down kernel gets the limit itself.
BUDGETS = {
    "20display_down0_kernelE": (24, 0, 0),
    "19display_down_kernelE": (64, 0, 0),
    "17display_up_kernelE": (35, 0, 0),
    "22display_resolve_kernelILb1EE": (35, 0, 0),
    "22display_resolve_kernelILb0EE": (17, 0, 0),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "display.s")
    src = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_display.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_display_kernels_keep_their_budgets(isa, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    got = int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions" % (kernel, got[1], got[2])
