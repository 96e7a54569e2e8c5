"""jpt_meter without a GPU: the host form of the pass (jpt_debug_meter, device -1) against the restatement (np_meter) in every bin and
every bit of the result, the C ABI's refusals on a host-only context, the header, and the register budgets of the new kernels in the
cross-compiled ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_meter as nm

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (33, 9), (257, 131)]
CLIPS = [(0, 1000), (100, 900), (499, 500)]
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def debug_meter(L, device, image, prev=None, want_hist=True, **fields):
    h, w = image.shape[:2]
    image = np.ascontiguousarray(image, F)
    hist = np.zeros(256, np.uint32) if want_hist else None
    res = capi.MeterResult()
    rc = L.jpt_debug_meter(device, w, h, C.byref(capi.MeterParams(**fields)) if fields else None, image.ctypes.data,
                           NAN if prev is None else float(prev), None if hist is None else hist.ctypes.data, C.byref(res))
    assert rc == 0, "jpt_debug_meter(device %d) = %d" % (device, rc)
    return hist, res.as_dict()


def same_result(got, want, what):
    """every bit of the six fields"""
    for name in ("exposure", "target", "luminance"):
        assert nm.bits(got[name]) == nm.bits(want[name]), "%s: %s is %r (0x%08x), the restatement gives %r (0x%08x)" % (
            what, name, got[name], nm.bits(got[name]), float(want[name]), nm.bits(want[name]))
    for name in ("flags", "weight", "used"):
        assert int(got[name]) == int(want[name]), "%s: %s is %d, the restatement gives %d" % (what, name, got[name], want[name])


def check_against_restatement(L, device, img, prev=None, **fields):
    what = "%dx%d %s prev %r" % (img.shape[1], img.shape[0], fields, prev)
    hist, res = debug_meter(L, device, img, prev, **fields)
    want_hist, want = nm.meter(img, 1, prev, **fields)
    bad = np.flatnonzero(hist.astype(np.int64) != np.array(want_hist, np.int64))
    assert not len(bad), "%s: %d bins differ, first %s" % (what, len(bad), [(int(b), int(hist[b]), want_hist[b]) for b in bad[:4]])
    same_result(res, want, what)
    return hist, res


# ---- 1. the host form equals the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [nm.AVERAGE, nm.CENTER_WEIGHTED])
@pytest.mark.parametrize("size", SIZES)
def test_host_form_equals_the_restatement_in_every_bin_and_bit(L, size, mode):
    """images with NaN, +-inf, negatives, zeros, denormals, values below 2^-20 and at and above 2^12 and the bounds of a sweep of bins"""
    img = nm.edge_image(size[0], size[1], seed=size[0])
    for low, high in CLIPS:
        check_against_restatement(L, HOST_ONLY, img, mode=mode, low_permille=low, high_permille=high)
        for adapt in (0.0, 0.25, 1.0):
            check_against_restatement(L, HOST_ONLY, img, prev=0.75, mode=mode, low_permille=low, high_permille=high, adapt=adapt)


def test_the_edge_image_reaches_what_it_is_meant_to(L):
    """the fixture spans what the pin names, and the library bins single pixels of each kind where the pin says"""
    img = nm.edge_image(257, 131, seed=257)
    b = nm.bins_of(img)
    assert (b == -1).sum() >= 10 and (b == 0).sum() >= 4 and (b == 255).sum() >= 5
    assert len(np.unique(b)) > 200
    for k in (1, 8, 100, 255):
        assert nm.bits(nm.bin_lower_bound(k)) == (k + 856) << 20

    def library_bin(rgb):
        """the bin the library's host form puts one pixel in, -1 for a skipped one"""
        hist, res = debug_meter(L, HOST_ONLY, np.array([[list(rgb) + [0]]], F), low_permille=0, high_permille=1000)
        assert int(hist.sum()) == res["weight"] <= 1
        return int(np.flatnonzero(hist)[0]) if res["weight"] else -1

    for v in (1e-45, 2.0 ** -25):                       # a denormal, and below 2^-20
        assert library_bin((v, v, v)) == 0
    for v in (4096.0, 1e30):                            # at and above 2^12
        assert library_bin((v, v, v)) == 255
    assert library_bin((1.0, 1.0, 1.0)) == 160          # 2^0: (0 + 20) * 8
    for v in (np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0):
        assert library_bin((v, v, v)) == -1
    assert library_bin((1.0, 1.0, np.inf)) == -1


def test_every_bin_bound(L):
    """grey pixels on, just below and just above the lower bound of every bin: the luminance of a grey v is v up to an ulp, so these
    fall on either side of the bounds, and the library must put each where the restatement puts it"""
    vals = []
    for b in range(1, 256):
        v = nm.bin_lower_bound(b)
        vals += [v, np.nextafter(v, F(0)), np.nextafter(v, F(np.inf))]
    img = np.zeros((3, 255, 4), F)
    img[..., 0] = img[..., 1] = img[..., 2] = np.array(vals, F).reshape(255, 3).T
    hist, _ = check_against_restatement(L, HOST_ONLY, img, low_permille=0, high_permille=1000)
    assert int(hist.sum()) == 3 * 255


def test_the_resolve_by_hand(L):
    """64 x 64 of 0.18 = 2^-3 * 1.44: the octave from 2^-3 is bins 136..143 and 0.44 * 8 = 3.52, so bin 139 = [0.171875, 0.1875); with
    all the weight in one bin p = (2 * 139 + 1) * 32768 and L_avg is the bin's middle in the bits, 2^-3 * (1 + 3.5 / 8) = 0.1796875"""
    img = np.full((64, 64, 4), 0.18, F)
    hist, res = check_against_restatement(L, HOST_ONLY, img)
    assert int(hist[139]) == 4096 and int(hist.sum()) == 4096
    assert res["weight"] == 4096 and res["used"] == 4096 * 900 // 1000 - 4096 * 100 // 1000 and res["flags"] == nm.FIRST
    assert res["luminance"] == 0.1796875 and nm.bits(res["exposure"]) == nm.bits(F(0.18) / F(0.1796875)) == nm.bits(res["target"])
    # center-weighted: the middle 32 x 32 counts four times
    hist, res = check_against_restatement(L, HOST_ONLY, img, mode=nm.CENTER_WEIGHTED)
    assert int(hist[139]) == 4096 + 3 * 1024 and res["weight"] == 4096 + 3 * 1024


def test_empty_histograms_keep_the_exposure(L):
    black = np.zeros((9, 33, 4), F)
    skipped = np.full((9, 33, 4), np.nan, F)
    skipped[::2] = -1.0
    for img in (black, skipped):
        hist, res = check_against_restatement(L, HOST_ONLY, img)
        assert int(hist.sum()) == 0 and res["flags"] == nm.EMPTY | nm.FIRST and res["exposure"] == 1.0 and res["target"] == 1.0
        assert res["luminance"] == 0.0 and res["used"] == 0 and res["weight"] == 0
        _, res = check_against_restatement(L, HOST_ONLY, img, min_exposure=2.0, max_exposure=8.0)
        assert res["exposure"] == 2.0                       # a FIRST and EMPTY call: clamp(1, min, max)
        _, res = check_against_restatement(L, HOST_ONLY, img, prev=3.5, adapt=0.25)
        assert res["flags"] == nm.EMPTY and res["exposure"] == 3.5 and res["target"] == 3.5
    # one counted pixel and a clip that leaves nothing of it: used == 0 although the weight is not
    one = np.zeros((1, 1, 4), F)
    one[..., :3] = 0.5
    _, res = check_against_restatement(L, HOST_ONLY, one, low_permille=499, high_permille=500)
    assert res["weight"] == 1 and res["used"] == 0 and res["flags"] == nm.EMPTY | nm.FIRST


def test_adaptation_and_clamping(L):
    img = np.full((9, 33, 4), 0.18, F)
    target = F(0.18) / F(0.1796875)
    for prev in (0.25, 4.0):
        for adapt in (0.0, 0.25, 1.0):
            _, res = check_against_restatement(L, HOST_ONLY, img, prev=prev, adapt=adapt)
            assert res["flags"] == 0 and nm.bits(res["target"]) == nm.bits(target)
            assert nm.bits(res["exposure"]) == nm.bits(F(prev) + F(F(target - F(prev)) * F(adapt)))
    _, res = check_against_restatement(L, HOST_ONLY, img, prev=0.25, adapt=0.0)
    assert res["exposure"] == 0.25
    # both ends of the clamp: a dark image wants more than max, a bright one less than min
    dark, bright = np.full((9, 33, 4), 1e-4, F), np.full((9, 33, 4), 500.0, F)
    _, res = check_against_restatement(L, HOST_ONLY, dark)
    assert res["exposure"] == 64.0 and res["target"] == 64.0
    _, res = check_against_restatement(L, HOST_ONLY, bright)
    assert res["exposure"] == 1.0 / 64.0
    _, res = check_against_restatement(L, HOST_ONLY, dark, min_exposure=0.5, max_exposure=2.0, key=0.36)
    assert res["exposure"] == 2.0
    _, res = check_against_restatement(L, HOST_ONLY, bright, min_exposure=0.5, max_exposure=0.5)
    assert res["exposure"] == 0.5
    # the steady state of the recurrence is the target
    e = 4.0
    for _ in range(80):
        _, res = debug_meter(L, HOST_ONLY, img, prev=e, adapt=0.25)
        e = res["exposure"]
    assert abs(e - float(target)) < 1e-5


def test_the_clipping_ignores_the_ends(L):
    """a tenth of the pixels at 100, a tenth at 1e-3, the rest at 0.18: the default 100 / 900 clip meters the 0.18 alone"""
    img = np.full((10, 100, 4), 0.18, F)
    img[0] = 100.0
    img[9] = 1e-3
    _, res = check_against_restatement(L, HOST_ONLY, img)
    assert res["luminance"] == 0.1796875 and res["used"] == 800
    _, res = check_against_restatement(L, HOST_ONLY, img, low_permille=0, high_permille=1000)
    assert res["luminance"] != 0.1796875 and res["used"] == 1000


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------------------

BAD = [("source", -1), ("source", 2), ("mode", -1), ("mode", 2), ("low_permille", -1), ("low_permille", 1001), ("high_permille", 100),
       ("high_permille", 50), ("high_permille", 1001), ("key", 0.0), ("key", -1.0), ("key", NAN), ("key", float("inf")),
       ("min_exposure", 0.0), ("min_exposure", NAN), ("min_exposure", float("inf")), ("max_exposure", 0.001), ("max_exposure", NAN),
       ("max_exposure", float("inf")), ("adapt", -0.1), ("adapt", 1.5), ("adapt", NAN)]


def test_refusals_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_meter_params
        for field, value in BAD:
            assert S(ctx.h, C.byref(capi.MeterParams(**{field: value}))) == E_INVALID, (field, value)
            msg = L.jpt_last_error(ctx.h)
            assert b"jpt_meter_params" in msg and field.encode() in msg, msg      # each bad parameter is named
        for good in (dict(low_permille=0, high_permille=1), dict(high_permille=1000), dict(adapt=0.0), dict(min_exposure=2.0, max_exposure=2.0), dict()):
            assert S(ctx.h, C.byref(capi.MeterParams(**good))) == E_DEVICE, good     # checks passed: no device
        assert S(ctx.h, None) == E_DEVICE
        assert S(None, None) == E_INVALID and L.jpt_meter(None) == E_INVALID and L.jpt_meter_reset(None) == E_INVALID
        assert L.jpt_set_auto_exposure(None, 1) == E_INVALID and L.jpt_read_meter(None, None, None) == E_INVALID
        assert L.jpt_set_auto_exposure(ctx.h, 2) == E_INVALID and L.jpt_set_auto_exposure(ctx.h, -1) == E_INVALID
        assert L.jpt_set_auto_exposure(ctx.h, 1) == E_DEVICE and L.jpt_set_auto_exposure(ctx.h, 0) == E_DEVICE
        assert L.jpt_meter_reset(ctx.h) == E_DEVICE
        # the state errors that need no device come before the device is asked for, in jpt_display's order
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        ctx.set_debug_steps(True)
        ctx.set_partition(1, 2)
        assert L.jpt_meter(ctx.h) == E_STATE and b"JPT_DENOISE_PROGRESSIVE" in L.jpt_last_error(ctx.h)
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        assert L.jpt_meter(ctx.h) == E_STATE and b"DEBUG_STEPS" in L.jpt_last_error(ctx.h)
        ctx.set_debug_steps(False)
        assert L.jpt_meter(ctx.h) == E_STATE and b"whole image on one context" in L.jpt_last_error(ctx.h)
        ctx.set_partition(0, 1)
        assert L.jpt_meter(ctx.h) == E_DEVICE and b"host-only" in L.jpt_last_error(ctx.h)
        res = capi.MeterResult()
        assert L.jpt_read_meter(ctx.h, None, None) == E_INVALID
        assert L.jpt_read_meter(ctx.h, C.byref(res), None) == E_DEVICE
        with pytest.raises(capi.JptError, match="host-only"):
            ctx.meter()
    finally:
        ctx.close()


def test_debug_meter_checks_its_arguments(L):
    img = nm.edge_image(8, 8)
    hist, res = np.zeros(256, np.uint32), capi.MeterResult()
    D = L.jpt_debug_meter
    assert D(HOST_ONLY, 0, 8, None, img.ctypes.data, NAN, hist.ctypes.data, C.byref(res)) == E_INVALID
    assert D(HOST_ONLY, 8, 65537, None, img.ctypes.data, NAN, hist.ctypes.data, C.byref(res)) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, None, NAN, hist.ctypes.data, C.byref(res)) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, img.ctypes.data, NAN, hist.ctypes.data, None) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, img.ctypes.data, float("inf"), hist.ctypes.data, C.byref(res)) == E_INVALID
    assert D(HOST_ONLY, 65536, 32768, None, img.ctypes.data, NAN, hist.ctypes.data, C.byref(res)) == E_LIMIT      # 2^31 pixels: refused before a read
    for field, value in BAD:
        assert D(HOST_ONLY, 8, 8, C.byref(capi.MeterParams(**{field: value})), img.ctypes.data, NAN, hist.ctypes.data, C.byref(res)) == E_INVALID
    assert D(HOST_ONLY, 8, 8, None, img.ctypes.data, NAN, hist.ctypes.data, C.byref(res)) == 0
    # NULL parameters are the defaults; the histogram is optional
    want_hist, want = nm.meter(img)
    assert [int(v) for v in hist] == want_hist
    same_result(res.as_dict(), want, "defaults")
    _, alone = debug_meter(L, HOST_ONLY, img, want_hist=False)
    same_result(alone, want, "without the histogram")
    assert C.sizeof(capi.MeterResult) == 32 and C.sizeof(capi.MeterParams) == 32


def test_the_header_declares_the_calls_and_keeps_the_abi(L):
    hdr = open(os.path.join(ROOT, "include", "jpt.h")).read()
    assert re.search(r"#define\s+JPT_ABI_VERSION\s+6\b", hdr) and L.jpt_abi_version() == 6
    names = ("jpt_set_meter_params", "jpt_meter", "jpt_meter_reset", "jpt_read_meter", "jpt_set_auto_exposure", "jpt_debug_meter")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    for token in ("JPT_METER_AVERAGE = 0", "JPT_METER_CENTER_WEIGHTED = 1", "JPT_METER_EMPTY = 1", "JPT_METER_FIRST = 2", "jpt_meter_params;",
                  "jpt_meter_result;"):
        assert token in hdr, token


# ---- 3. register budgets -----------------------------------------------------------------------------------------------------------

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane).  The histogram runs eight blocks per CU, eight
# waves per SIMD: at most 64 VGPRs, no scratch.  First compile: histogram 26, center-weighted 36; each gets its first figure plus a
# quarter.  The resolve is one wave (its 16 sets' loads are all in flight: 60 at first compile): 64.
BUDGETS = {
    "22meter_histogram_kernelILb0EE": (32, 0),
    "22meter_histogram_kernelILb1EE": (45, 0),
    "20meter_resolve_kernelE": (64, 0),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "meter.s")
    src = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_meter.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_meter_kernels_keep_their_budgets(isa, kernel):
    vgprs, scratch = BUDGETS[kernel]
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    got = int(m.group(2)), int(m.group(1))
    print(kernel, "vgprs %d scratch %d B" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d" % (kernel, got[0], vgprs)
    assert got[1] <= scratch, "%s: scratch %d B" % (kernel, got[1])
