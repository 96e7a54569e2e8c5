"""jpt_denoise without a GPU: the C ABI's refusals on a host-only context, the host form of the filter (jpt_debug_atrous, device -1)
against the float32 numpy restatement bit for bit, properties of the restatement itself, what the filter gains on 4-frame renders
of the oracle, and the register budgets of the new kernels in the cross-compiled ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_denoise as nd

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def debug_atrous(L, device, mean, position_t, normal, albedo, params=None):
    h, w = mean.shape[:2]
    arrays = [np.ascontiguousarray(a, F) for a in (mean, position_t, normal, albedo)]
    out = np.zeros((h, w, 4), F)
    rc = L.jpt_debug_atrous(device, w, h, None if params is None else C.byref(params), *[a.ctypes.data for a in arrays], out.ctypes.data)
    assert rc == 0, rc
    return out


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_denoise_params
        bad = [dict(passes=0), dict(passes=7), dict(normal_power_log2=-1), dict(normal_power_log2=9), dict(sigma_plane=0.0),
               dict(sigma_plane=-1.0), dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")), dict(sigma_color=0.0),
               dict(sigma_color=float("nan")), dict(sigma_color=float("inf"))]
        for fields in bad:
            assert S(ctx.h, C.byref(capi.DenoiseParams(**fields))) == E_INVALID, fields
            assert b"jpt_denoise_params" in L.jpt_last_error(ctx.h)
        assert S(ctx.h, None) == E_DEVICE and S(ctx.h, C.byref(capi.DenoiseParams())) == E_DEVICE   # checks passed: no device
        assert S(None, None) == E_INVALID and L.jpt_denoise(None) == E_INVALID
        # the state errors that need no device come before the device is asked for
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
        assert L.jpt_denoise(ctx.h) == E_STATE and b"JPT_DENOISE_PROGRESSIVE" in L.jpt_last_error(ctx.h)
        ctx.set_denoising_mode(capi.DENOISE_PROGRESSIVE)
        ctx.set_debug_steps(True)
        assert L.jpt_denoise(ctx.h) == E_STATE and b"DEBUG_STEPS" in L.jpt_last_error(ctx.h)
        ctx.set_debug_steps(False)
        ctx.set_partition(1, 2)
        assert L.jpt_denoise(ctx.h) == E_STATE and b"whole image on one context" in L.jpt_last_error(ctx.h)
        ctx.set_partition(0, 1)
        assert L.jpt_denoise(ctx.h) == E_DEVICE and b"host-only" in L.jpt_last_error(ctx.h)
        out = np.zeros(4, F)
        assert L.jpt_read_denoised_f32(ctx.h, None) == E_INVALID and L.jpt_read_denoised_rgba8(ctx.h, None) == E_INVALID
        assert L.jpt_read_denoised_f32(ctx.h, out.ctypes.data) == E_DEVICE
        assert L.jpt_read_denoised_rgba8(ctx.h, out.ctypes.data) == E_DEVICE
        assert L.jpt_read_guides_f32(ctx.h, None, None, None) == E_DEVICE
        with pytest.raises(capi.JptError, match="host-only"):
            ctx.denoise()
    finally:
        ctx.close()


def test_debug_atrous_checks_its_arguments(L):
    case = nd.synthetic_case(8, 8)
    out = np.zeros((8, 8, 4), F)
    ptrs = [a.ctypes.data for a in case]
    assert L.jpt_debug_atrous(HOST_ONLY, 0, 8, None, *ptrs, out.ctypes.data) == E_INVALID
    assert L.jpt_debug_atrous(HOST_ONLY, 8, 8, None, None, *ptrs[1:], out.ctypes.data) == E_INVALID
    assert L.jpt_debug_atrous(HOST_ONLY, 8, 8, C.byref(capi.DenoiseParams(passes=9)), *ptrs, out.ctypes.data) == E_INVALID
    assert L.jpt_debug_atrous(HOST_ONLY, 8, 8, None, *ptrs, out.ctypes.data) == 0


# ---- 3. the host form equals the restatement -----------------------------------------------------------------------------------

PARAM_SETS = [dict(passes=p) for p in range(1, 7)] + [dict(passes=4, normal_power_log2=0, sigma_plane=0.5, sigma_color=0.25),
                                                      dict(passes=6, normal_power_log2=8, sigma_plane=0.003, sigma_color=64.0)]


@pytest.mark.parametrize("prm", PARAM_SETS, ids=lambda p: "-".join("%s" % v for v in p.values()))
def test_host_filter_equals_the_numpy_restatement_bit_for_bit(L, prm):
    """seeded random colour with planted NaN / inf pixels over guides with a depth step, a crease, a miss region and the borders"""
    for w, h, seed in ((67, 45, 1), (96, 64, 2), (1, 1, 3), (5, 40, 4)):
        case = nd.synthetic_case(w, h, seed)
        got = debug_atrous(L, HOST_ONLY, *case, params=capi.DenoiseParams(**prm))
        want = nd.atrous(*case, **prm)
        bad = ~nd.same_bits(got, want)
        assert not bad.any(), "%dx%d: %d values differ, first %s" % (w, h, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (got[..., 3] == 1).all()
    # the defaults are the library's
    case = nd.synthetic_case(40, 30, 9)
    assert nd.same_bits(debug_atrous(L, HOST_ONLY, *case), nd.atrous(*case, **nd.DEFAULTS)).all()


# ---- 4. properties of the restatement -------------------------------------------------------------------------------------------

def test_a_constant_image_is_a_fixed_point():
    """i_0 is constant where mean = c * amod: every pass averages equal values with weights that sum to the divisor -- exactly,
    when the demodulated constant is a power of two (every partial sum of the binomial weights times it is exact)"""
    _, pos, nrm, alb = nd.synthetic_case(67, 45, 5)
    mean = np.zeros((45, 67, 4), F)
    mean[..., :3] = nd.amod(alb) * F(0.5)
    out = nd.atrous(mean, pos, nrm, alb, passes=6)
    assert np.array_equal(out[..., :3], mean[..., :3])


def test_a_colour_step_on_a_crease_or_a_plane_step_is_preserved_exactly():
    h, w = 32, 64
    ys, xs = np.mgrid[0:h, 0:w]
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = 1.0
    for kind in ("crease", "plane"):
        pos = np.zeros((h, w, 4), F)
        pos[..., 0], pos[..., 1], pos[..., 2] = (xs - w / 2) * 0.05, (ys - h / 2) * 0.05, -5.0
        nrm = np.zeros((h, w, 4), F)
        nrm[..., 2] = 1.0
        right = xs >= w // 2
        if kind == "crease":
            nrm[right] = np.array([1.0, 0.0, 0.0, 0.0], F)      # perpendicular normals: dot = 0, the normal weight is 0
            pos[right, 0] = pos[0, w // 2, 0]                   # ... and the right half lies in the plane x = const of its normal
            pos[right, 2] = -5.0 - (xs[right] - w // 2) * 0.05
        else:
            pos[right, 2] = -5.0 - 2.0                          # a step of 2 >> sigma_plane * t = 0.02 * ~5.4 along the normal
        pos[..., 3] = np.sqrt((pos[..., :3].astype(np.float64) ** 2).sum(-1))
        mean = np.zeros((h, w, 4), F)
        mean[..., :3] = np.where(right[..., None], F(0.25), F(2.0))
        out = nd.atrous(mean, pos, nrm, alb, passes=5)
        assert np.array_equal(out[..., :3], mean[..., :3]), kind


def test_white_noise_on_a_flat_region_loses_variance_with_every_pass():
    h, w = 96, 96
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:h, 0:w]
    pos = np.zeros((h, w, 4), F)
    pos[..., 0], pos[..., 1], pos[..., 2] = (xs - w / 2) * 0.02, (ys - h / 2) * 0.02, -4.0
    pos[..., 3] = np.sqrt((pos[..., :3].astype(np.float64) ** 2).sum(-1))
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = 1.0
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = 0.5
    mean = np.zeros((h, w, 4), F)
    mean[..., :3] = (0.5 + 0.2 * rng.standard_normal((h, w, 3))).astype(F)
    var = [float(np.var(mean[24:72, 24:72, :3].astype(np.float64)))]
    for passes in range(1, 7):
        out = nd.atrous(mean, pos, nrm, alb, passes=passes)
        var.append(float(np.var(out[24:72, 24:72, :3].astype(np.float64))))
    print("variance by passes:", ["%.3g" % v for v in var])
    assert all(b < a for a, b in zip(var, var[1:])), var


# ---- 5. quality ----------------------------------------------------------------------------------------------------------------

# measured ratio RMSE(np_denoise(4 frames)) / RMSE(raw 4-frame mean) against a 1024-frame oracle render, defaults, 96 x 64
MEASURED = {"cornell": 0.5358, "demo800": 0.5880}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_four_frames_denoised_are_closer_to_a_long_render_than_the_raw_mean(oracle, name):
    """Cornell and demo_scene(800) at 96 x 64, ACCUM_HDR_F32, 4 bounces: frames 1..4 of the oracle, denoised by the restatement
    with the default parameters, against the mean of 1024 other oracle frames (1000..2023), RMSE on the linear image.  Measured
    ratios denoised / raw: Cornell 0.5358, demo_scene(800) 0.5880 (deterministic).  The condition is a ratio below 1; asserted
    is the midpoint between the measured value and 1, so that a later change that gives half the benefit back fails."""
    sc = scenes.cornell_scene() if name == "cornell" else scenes.demo_scene(800)
    w, h, truth_frames = 96, 64, 1024
    cam = scenes.camera_block(sc.camera, w, h)
    ref = oracle.build_scene(sc)
    truth = oracle.render(ref, cam, w, h, max_bounces=4, n_frames=truth_frames, first_frame_index=1000, accum_mode=wire.ACCUM_HDR_F32)[0]
    truth = truth[..., :3].astype(np.float64) / truth_frames
    acc = oracle.render(ref, cam, w, h, max_bounces=4, n_frames=4, first_frame_index=1, accum_mode=wire.ACCUM_HDR_F32)[0]
    den = nd.denoise(acc, 4, *nd.guides(ref, cam, w, h))[..., :3]
    raw = acc[..., :3] / F(4)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))

    ratio = rmse(den) / rmse(raw)
    print("%s: RMSE raw %.4f, denoised %.4f, ratio %.4f (measured %.4f)" % (name, rmse(raw), rmse(den), ratio, MEASURED[name]))
    assert ratio < 1.0
    assert ratio <= (MEASURED[name] + 1.0) / 2


# ---- 6. register budgets ---------------------------------------------------------------------------------------------------------

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body).  Every one
# of them stays at eight waves per SIMD (at most 64 VGPRs) except guide_kernel, whose launch is one wave per block with 24 KB of LDS
# for the traversal stack (wf2_occlude's arrangement): six blocks per CU, under two waves per SIMD whatever its registers -- it runs
# once per jpt_denoise, one ray per pixel.
BUDGETS = {
    "12guide_kernelILb1EE": (75, 0, 0),
    "12guide_kernelILb0EE": (67, 0, 0),
    "13atrous_kernelILi2ELb1ELb1EE": (33, 0, 0),
    "13atrous_kernelILi2ELb1ELb0EE": (33, 0, 0),
    "13atrous_kernelILi4ELb0ELb1EE": (29, 0, 0),
    "13atrous_kernelILi4ELb0ELb0EE": (31, 0, 0),
    "13atrous_kernelILi0ELb0ELb1EE": (52, 0, 0),
    "13atrous_kernelILi0ELb0ELb0EE": (50, 0, 0),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "denoise.s")
    src = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_denoise.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_denoise_kernels_keep_their_budgets(isa, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    got = int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions" % (kernel, got[1], got[2])
