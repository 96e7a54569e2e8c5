"""Importance sampling of the emissive triangles (jpt_set_light_sampling) without a GPU: the C ABI's refusals, the density p_L of
tests/np_light_sampling.py in float64 (it integrates to 1 over the emitters; w_L + w_brdf = 1 on sampled directions), the numpy
estimator against BRDF sampling alone, and the register budgets of the new kernels in the cross-compiled ISA."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_light_sampling as nls
import np_path

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE = -1, -2   # include/jpt.h


@pytest.fixture(scope="module")
def L():
    return capi.lib()


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------

def test_refusals(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_light_sampling
        assert S(ctx.h, 2) == E_INVALID and S(ctx.h, -1) == E_INVALID
        assert S(ctx.h, capi.LIGHT_SAMPLING_MIS) == E_DEVICE   # checks passed: no device
        assert S(ctx.h, capi.LIGHT_SAMPLING_BRDF) == E_DEVICE
        assert S(None, capi.LIGHT_SAMPLING_MIS) == E_INVALID
        assert L.jpt_multi_set_light_sampling(None, 1) == E_INVALID
        n = np.zeros(2, np.uint32)
        assert L.jpt_debug_light_tables(ctx.h, 0, n.ctypes.data, None, None, None, None) == E_DEVICE
        with pytest.raises(RuntimeError):
            ctx.set_light_sampling(7)
    finally:
        ctx.close()


# ---- 2. the density in float64 -----------------------------------------------------------------------------------------------------

def _emitter_set(ref):
    pairs = nls.emitters(ref)
    le = nls.emission(ref, pairs[:, 0], pairs[:, 1]).astype(np.float64)
    p0, e1, e2 = (a.astype(np.float64) for a in nls._world_edges(ref, pairs[:, 0], pairs[:, 1]))
    g = np.cross(e1, e2)
    area = 0.5 * np.linalg.norm(g, axis=1)
    lum = le @ np.array([0.2126, 0.7152, 0.0722])
    return p0, e1, e2, g, area, lum


def test_the_density_integrates_to_one_over_the_emitters(oracle):
    """p_L(y) = lum * d^2 / (total |cos_y|) per unit solid angle is, per unit area, lum / total: summed over every emitter's
    area it is 1.  Checked by Monte Carlo over solid angle from a point inside the box, with the visibility left out."""
    sc = scenes.demo_scene(n_tris=256)
    ref = oracle.build_scene(sc)
    p0, e1, e2, g, area, lum = _emitter_set(ref)
    total = float((lum * area).sum())
    assert np.isclose(float((lum * area / total).sum()), 1.0, rtol=1e-12)
    # uniform points on the emitters, weighted by area: E[p_L * |cos| / d^2 * total_area] = sum lum*area/total = 1
    rng = np.random.default_rng(3)
    n = 200000
    k = rng.choice(len(area), n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    s = np.sqrt(u)
    y = p0[k] + e1[k] * (s * (1 - v))[:, None] + e2[k] * (s * v)[:, None]
    o = np.array([0.1, -0.5, 0.3])
    dv = y - o
    d2 = (dv * dv).sum(1)
    l = dv / np.sqrt(d2)[:, None]
    c = np.abs((g[k] / np.linalg.norm(g[k], axis=1)[:, None] * l).sum(1))
    p_sa = lum[k] * d2 / (total * c)
    est = (p_sa * c / d2).mean() * area.sum()
    assert abs(est - 1.0) < 0.01, est


def test_weights_sum_to_one_on_sampled_directions(oracle):
    sc = scenes.cornell_scene()
    ref = oracle.build_scene(sc)
    tabs = nls.tables(ref)
    rng = np.random.default_rng(5)
    xi = rng.random((4096, 4)).astype(F)
    origins = rng.uniform(-2.5, 2.5, (4096, 3)).astype(F)
    y, l, pl = nls.sample_seen_from(tabs, xi, origins)
    pb = rng.uniform(0.0, 3.0, 4096)
    pl = pl.astype(np.float64)
    ok = pl > 0
    assert ok.mean() > 0.9
    wl = pl[ok] ** 2 / (pl[ok] ** 2 + pb[ok] ** 2)
    wb = pb[ok] ** 2 / (pb[ok] ** 2 + pl[ok] ** 2)
    assert np.allclose(wl + wb, 1.0, rtol=1e-12)


def test_light_estimator_is_unbiased_in_numpy(oracle):
    """trace_lights against the same function with the emitter total forced to 0 (BRDF sampling alone): the mean of many frames of
    a small scene with emitters agrees within stated sigmas"""
    sc = scenes.cornell_scene()
    ref = oracle.build_scene(sc)
    w = h = 8
    frames = 48
    cam = scenes.camera_block(sc.camera, w, h).copy()
    tabs = nls.tables(ref)
    off = dict(tabs, total=F(0))
    est = {}
    for mode, t in (("lights", tabs), ("brdf", off)):
        vals = []
        for f in range(frames):
            cam["frame_index"] = 1 + f
            vals.append(nls.trace_lights(ref, cam, w, h, 2, tabs=t).astype(np.float64).sum(-1))
        est[mode] = np.array(vals)
    ok = np.isfinite(est["lights"]).all(axis=0) & np.isfinite(est["brdf"]).all(axis=0)
    assert ok.mean() > 0.9
    for mode in ("lights", "brdf"):
        v = est[mode][:, ok]
        est[mode] = (v.mean(), v.mean(axis=1).std(ddof=1) / np.sqrt(frames))
    diff = abs(est["lights"][0] - est["brdf"][0])
    se = np.hypot(est["lights"][1], est["brdf"][1])
    assert diff <= 4.0 * se + 1e-6, (est, diff / se)


# ---- 3. register budgets of the new kernels ------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc")

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body)
# Pinned at what the build takes.  The filtered wf2_shade_lt forms take 81 VGPRs (the map's MIS kernels 73): the emitter sample,
# its gathers and the second shadow-queue store; still five waves per SIMD under the kernel's launch bounds.  The form without
# textures is held to 72 VGPRs by its seven-wave bound and spills 20 bytes.  wf2_occlude_lt keeps its stack in LDS: no scratch.
BUDGETS = {
    "jpt_kernels_wf2.hip": {
        "12wf2_shade_ltILb0ELb0ELi0E": (72, 20, 4),
        "12wf2_shade_ltILb0ELb0ELi1E": (81, 0, 0),
        "12wf2_shade_ltILb0ELb0ELi2E": (81, 0, 0),
        "12wf2_shade_ltILb0ELb1ELi0E": (55, 0, 0),   # the paths' last vertices (no emitter sample)
        "14wf2_occlude_ltILb0ELb0EE": (53, 0, 0),
        "14wf2_occlude_ltILb0ELb1EE": (76, 0, 0),
    },
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = {}
    for src in BUDGETS:
        path = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
        flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
        r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", path, os.path.join(CSRC, src)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        out[src] = open(path).read()
    return out


def usage(isa, kernel):
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    return int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))


@pytest.mark.parametrize("src,kernel", sorted((s, k) for s in BUDGETS for k in BUDGETS[s]))
def test_light_sampling_kernels_keep_their_budgets(isa, src, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[src][kernel]
    got = usage(isa[src], kernel)
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d" % (
        kernel, got[1], got[2], scratch, scratch_ops)
