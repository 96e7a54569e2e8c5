"""The procedural sky on the host (jpt_set_sky; CPU): the host's copy of the pinned arithmetic (jpt_debug_sky with
JPT_DEVICE_HOST_ONLY, jpt_debug_sky_radiance, jpt_debug_pow01) against tests/np_sky.py bit for bit; pow01_ and sky_radiance against
float64 within derived bounds; the energy a supersampled sun disk carries; the orientation against np_env's lookup; the refusals that
need no device; the header and the bindings."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_env
import np_sky as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_LIMIT, E_STATE = -1, -2, -3, -4   # JPT_E_*

# one sun at +y, one below the horizon, one straddling it, one in the open sky (the halos of the first and the last overlap)
SUNS = [dict(direction=(0.0, 1.0, 0.0), angular_radius=0.1, color=(5.0, 4.0, 3.0), energy=2.0),
        dict(direction=(0.3, -0.5, 0.2), angular_radius=0.2, color=(9.0, 1.0, 1.0)),
        dict(direction=(2.0, 0.04, 0.2), angular_radius=0.15, color=(1.0, 0.9, 0.8), energy=3.0, mode=ns.SUN_IRRADIANCE),
        dict(direction=(0.3, 0.8, 0.52), angular_radius=0.05, color=(1.0, 1.0, 0.5), energy=40.0)]
SUN_SETS = {0: [], 1: SUNS[:1], 4: SUNS}
SIZES = ((64, 32, 1), (64, 32, 3), (64, 32, 8), (37, 19, 2))


def hard_params():
    """all curves 1/64, colours of different hue, energies 2 and 0.5, exposure 1.5, a sun of radius 0.05 with a halo out to 0.3, radiance 1000"""
    return ns.params(sky_top_color=(0.1, 0.3, 0.9), sky_horizon_color=(0.9, 0.6, 0.2), ground_bottom_color=(0.05, 0.4, 0.1),
                     ground_horizon_color=(0.5, 0.1, 0.6), sky_curve=1.0 / 64, ground_curve=1.0 / 64, sun_curve=1.0 / 64, sky_energy=2.0,
                     ground_energy=0.5, exposure=1.5, sun_angle_max=0.3,
                     suns=[dict(direction=(0.3, 0.8, 0.52), angular_radius=0.05, color=(1.0, 0.8, 0.6), energy=1000.0)])


@pytest.fixture(scope="module")
def L():
    return capi.lib()


# ---- 1. the host equals the restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_suns", sorted(SUN_SETS))
def test_host_sky_equals_numpy_bit_for_bit(n_suns):
    p = ns.params(suns=SUN_SETS[n_suns])
    for w, h, n in SIZES:
        got = host.debug_sky(HOST_ONLY, ns.lib_params(p), w, h, n)
        assert got.shape == (h, w, 3) and ns.same_bits(got, ns.sky_map(p, w, h, n)), (w, h, n)
    assert ns.same_bits(host.debug_sky(HOST_ONLY, ns.lib_params(hard_params()), 37, 19, 2), ns.sky_map(hard_params(), 37, 19, 2))


def test_host_sky_radiance_and_pow01_equal_numpy_bit_for_bit():
    d = np_env.directions(20000, seed=5)
    for p in (ns.params(), ns.params(suns=SUNS), hard_params()):
        assert ns.same_bits(host.debug_sky_radiance(ns.lib_params(p), d), ns.sky_radiance(p, d))
    b, e = pow_pairs(200_000, seed=9)
    edge = np.array([0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 0.5, 2.0 ** -0.5, 1.5, -1.0], F)
    for ev in (0.125, 1.0, 6.6666665, 64.0):
        assert ns.same_bits(host.debug_pow01(edge, ev), ns.pow01_(edge, F(ev))), ev
    assert ns.same_bits(host.debug_pow01(b, e), ns.pow01_(b, e))


# ---- 2. pow01_ against float64 ------------------------------------------------------------------------------------------------------------

def pow_pairs(n, seed):
    """b: half uniform in (0, 1), half log-uniform down to 2^-24; e log-uniform in [1/8, 64]"""
    rng = np.random.default_rng(seed)
    b = np.concatenate([rng.uniform(0.0, 1.0, n // 2), 2.0 ** rng.uniform(-24.0, 0.0, n - n // 2)]).astype(F)
    e = (2.0 ** rng.uniform(-3.0, 6.0, n)).astype(F)
    return np.clip(b, F(2.0 ** -24), F(1.0 - 2.0 ** -24)), e


def test_pow01_is_within_2_to_minus_21_of_float64():
    b, e = pow_pairs(2_000_000, seed=20261)
    got = host.debug_pow01(b, e)
    err = np.abs(got.astype(np.float64) - b.astype(np.float64) ** e.astype(np.float64))
    print("pow01_: worst |error| %.3e (bound 2^-21 = %.3e), largest value %.9g" % (err.max(), 2.0 ** -21, got.max()))
    assert err.max() <= 2.0 ** -21
    assert got.max() <= 1.0 and got.min() >= 0.0
    ends = host.debug_pow01(np.array([0.0, 1.0] * 4, F), np.array([0.125, 0.125, 1.0, 1.0, 7.0, 7.0, 64.0, 64.0], F))
    assert np.array_equal(ends.view(np.uint32), np.array([0.0, 1.0] * 4, F).view(np.uint32))      # exactly 0 and exactly 1
    # a result below 2^-126 is 0
    tiny = host.debug_pow01(np.array([2.0 ** -2, 2.0 ** -1.99], F), np.array([63.5, 64.0], F))
    assert tiny[0] == 0.0 and (tiny[1] == 0.0 or tiny[1] >= 2.0 ** -126)


# ---- 3. sky_radiance against the float64 formula ---------------------------------------------------------------------------------------

def unit_directions(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def near(L, n, spread, seed):
    rng = np.random.default_rng(seed)
    L = np.asarray(L, np.float64) / np.linalg.norm(L)
    v = L + rng.standard_normal((n, 3)) * spread / math.sqrt(2.0)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("which", ("defaults", "hard"))
def test_sky_radiance_is_within_the_derived_bound_of_the_float64_formula(which):
    if which == "defaults":
        p = ns.params(suns=[dict(direction=(0.3, 0.8, 0.52), angular_radius=0.05, color=(1.0, 0.95, 0.9), energy=8.0)])
    else:
        p = hard_params()
    sun = p["suns"][0]
    d = np.concatenate([unit_directions(1_000_000, 31), near(sun["direction"], 250_000, 0.05, 32)])
    keep = np.abs(d[:, 1]) >= F(1e-6)                      # at the horizon the step picks a branch, and the horizon colours may differ
    assert (~keep).sum() <= len(d) // 1000
    d = d[keep]
    # the float64 formula takes the directions as the library does: float32 values, renormalised (the library assumes unit length)
    d64 = d.astype(np.float64)
    got = host.debug_sky_radiance(ns.lib_params(p), d).astype(np.float64)
    want = ns.sky_radiance64(p, d64)
    M = max(max(p["sky_top_color"] + p["sky_horizon_color"]) * p["sky_energy"], max(p["ground_bottom_color"] + p["ground_horizon_color"]) * p["ground_energy"],
            float(ns.sun_radiance64(sun).max())) * p["exposure"]
    err = np.abs(got - want).max()
    print("sky_radiance (%s): worst |error| %.3e = %.3e M (M = %g), %d of %d directions left out" % (which, err, err / M, M, int((~keep).sum()), len(keep)))
    assert err <= 3e-5 * M


# ---- 4. energy ------------------------------------------------------------------------------------------------------------------------------

def disk_params(direction, mode=ns.SUN_RADIANCE, color=(1.0, 1.0, 1.0), energy=1.0):
    black = (0.0, 0.0, 0.0)
    return ns.params(sky_top_color=black, sky_horizon_color=black, ground_bottom_color=black, ground_horizon_color=black, sun_angle_max=0.0,
                     suns=[dict(direction=direction, angular_radius=0.1, color=color, energy=energy, mode=mode)])


def map_flux(m):
    h, w = m.shape[:2]
    return float((m[:, :, 0].astype(np.float64).sum(axis=1) * ns.row_solid_angles(w, h)).sum())


def test_a_supersampled_disk_carries_its_energy():
    """Sum of texel * (row's exact solid angle) against R * 2 pi (1 - cos 0.1) at 64 x 32.  The float64 formula gives 1.0065 of it towards
    normalize(0.3, 0.8, 0.52) with samples = 8 and 0.755 with samples = 1: the supersampling is what the test shows.  A sun within a texel
    row of a pole loses about 4 % (0.964 with the float64 formula): the subsamples are not weighted by sin theta."""
    cap = 2.0 * math.pi * (1.0 - math.cos(float(F(0.1))))
    L = (0.3, 0.8, 0.52)
    p = disk_params(L)
    fine = map_flux(host.debug_sky(HOST_ONLY, ns.lib_params(p), 64, 32, 8)) / cap
    coarse = map_flux(host.debug_sky(HOST_ONLY, ns.lib_params(p), 64, 32, 1)) / cap
    print("disk energy / exact: samples 8 %.4f, samples 1 %.4f; float64 formula %.4f, %.4f" % (
        fine, coarse, map_flux(ns.sky_map64(p, 64, 32, 8)) / cap, map_flux(ns.sky_map64(p, 64, 32, 1)) / cap))
    assert abs(fine - 1.0) <= 0.02
    assert abs(coarse - 1.0) > 0.10
    # other places, against the float64 formula's own sum (the float32 arithmetic moves a disk's edge by less than 1e-6 rad): low in the
    # sky but clear of the horizon; straddling the horizon, where the part below does not show (elevation 0.05 of a radius of 0.1: a
    # segment of 19.6 % is cut off); and at the pole, where the unweighted subsamples lose about 4 %
    for Lk, lo, hi in (((0.9, 0.25, -0.43), 0.98, 1.02), ((0.9, 0.05, -0.43), 0.78, 0.82), ((0.0, 1.0, 0.0), 0.94, 0.99)):
        pk = disk_params(Lk)
        got, want = map_flux(host.debug_sky(HOST_ONLY, ns.lib_params(pk), 64, 32, 8)) / cap, map_flux(ns.sky_map64(pk, 64, 32, 8)) / cap
        print("towards normalize%r: %.4f, float64 formula %.4f" % (Lk, got, want))
        assert lo <= got <= hi and abs(got - want) <= 0.002
    # JPT_SUN_IRRADIANCE: the disk alone sends color * energy of irradiance onto a surface that faces it (to first order in its size)
    irr = map_flux(host.debug_sky(HOST_ONLY, ns.lib_params(disk_params(L, ns.SUN_IRRADIANCE, (1.0, 1.0, 1.0), 3.0)), 64, 32, 8))
    print("JPT_SUN_IRRADIANCE, energy 3: %.4f" % irr)
    assert abs(irr - 3.0) <= 0.02 * 3.0


# ---- 5. orientation ------------------------------------------------------------------------------------------------------------------------

def test_the_sun_lands_where_the_lookup_looks_for_it():
    for L in ((0.3, 0.8, 0.52), (-0.7, 0.3, -0.2), (0.1, 0.5, 0.9), (0.9, 0.2, -0.43)):
        p = disk_params(L, color=(7.0, 5.0, 3.0))
        p["sky_top_color"] = p["sky_horizon_color"] = (0.1, 0.1, 0.1)
        w, h = 64, 32
        m = host.debug_sky(HOST_ONLY, ns.lib_params(p), w, h, 4)         # radius 0.1: a disk two texels wide
        Ln = (np.asarray(L, np.float64) / np.linalg.norm(L)).astype(F)
        phi, theta = math.atan2(Ln[0], -Ln[2]), math.atan2(math.hypot(Ln[0], Ln[2]), Ln[1])
        i, j = int((phi / (2 * math.pi) + 0.5) * w), int(theta / math.pi * h)          # the texel np_env's mapping puts L in
        assert m[j, i, 0] == m[:, :, 0].max(), (L, i, j, np.unravel_index(m[:, :, 0].argmax(), (h, w)))
    # a disk wider than two texels: the bilinear lookup at L returns the disk's radiance
    p = disk_params((0.3, 0.8, 0.52), color=(7.0, 5.0, 3.0))
    m = host.debug_sky(HOST_ONLY, ns.lib_params(p), 256, 128, 4)           # texels of 0.0245 rad, radius 0.1
    Ln = (np.asarray((0.3, 0.8, 0.52), np.float64) / np.linalg.norm((0.3, 0.8, 0.52))).astype(F)
    assert np.array_equal(np_env.env_radiance(m, Ln[None, :])[0], np.array([7.0, 5.0, 3.0], F))


# ---- 6. checks, defaults, the header and the bindings -------------------------------------------------------------------------------------

def test_defaults_and_null_params(L):
    p = capi.SkyParams()
    L.jpt_sky_defaults(C.byref(p))
    want = ns.params()
    for k, v in want.items():
        if k == "suns":
            continue
        got = getattr(p, k)
        if k.endswith("_color"):
            assert np.array_equal(np.array(list(got), F), np.asarray(v, F)), k
        else:
            assert F(got) == F(v), k
    assert p.n_suns == 0 and F(p.sun_angle_max) == F(math.radians(30.0))
    assert (p.sky_curve, p.ground_curve, p.sun_curve) == (F(0.15), F(0.02), F(0.15))
    L.jpt_sky_defaults(None)                                                  # (a null pointer is ignored)
    a = np.zeros((19, 37, 3), F)
    assert L.jpt_debug_sky(HOST_ONLY, None, 37, 19, 2, a.ctypes.data) == capi.OK
    assert ns.same_bits(a, host.debug_sky(HOST_ONLY, p, 37, 19, 2)) and ns.same_bits(a, ns.sky_map(ns.params(), 37, 19, 2))
    assert ns.same_bits(host.debug_sky(HOST_ONLY, None, 8, 4, 1), host.debug_sky(HOST_ONLY, capi.sky_params(), 8, 4, 1))
    d = np_env.directions(100)
    assert ns.same_bits(host.debug_sky_radiance(None, d), host.debug_sky_radiance(p, d))


def bad_params():
    """(field named in the message, SkyParams) for every refusal of the parameter block"""
    sun = dict(direction=(0.0, 1.0, 0.0), angular_radius=0.1)
    out = []
    for name in ("sky_top_color", "sky_horizon_color", "ground_bottom_color", "ground_horizon_color"):
        for v in (-0.5, np.inf, np.nan):
            out.append((name, capi.sky_params(**{name: (0.5, v, 0.5)})))
    for name in ("sky_energy", "ground_energy", "exposure"):
        for v in (-1.0, np.inf, np.nan):
            out.append((name, capi.sky_params(**{name: v})))
    for name in ("sky_curve", "ground_curve", "sun_curve"):
        for v in (0.0, 1.0 / 65, 8.5, -1.0, np.nan, np.inf):
            out.append((name, capi.sky_params(**{name: v})))
    for v in (-0.1, 3.2, np.nan):
        out.append(("sun_angle_max", capi.sky_params(sun_angle_max=v)))
    for v in (-1, 5):
        out.append(("n_suns", capi.sky_params(n_suns=v)))
    for v in ((0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0)):
        out.append(("suns[1].direction", capi.sky_params(suns=[sun, dict(sun, direction=v)])))
    for v in (0.0, -0.1, 1.6, np.nan):
        out.append(("suns[0].angular_radius", capi.sky_params(suns=[dict(sun, angular_radius=v)])))
    for v in (-1.0, np.nan, np.inf):
        out.append(("suns[0].color", capi.sky_params(suns=[dict(sun, color=(1.0, v, 1.0))])))
        out.append(("suns[0].energy", capi.sky_params(suns=[dict(sun, energy=v)])))
    for v in (-1, 2):
        out.append(("suns[3].mode", capi.sky_params(suns=[sun, sun, sun, dict(sun, mode=v)])))
    return out


def test_every_check_names_its_field(L):
    ctx = host.Context(HOST_ONLY)
    out = np.zeros((4, 8, 3), F)
    d = np.array([[0.0, 1.0, 0.0]], F)
    try:
        for name, p in bad_params():
            assert L.jpt_set_sky(ctx.h, C.byref(p), 8, 4, 1) == E_INVALID, name
            assert name in ctx.last_error() and "jpt_set_sky" in ctx.last_error(), (name, ctx.last_error())
            assert L.jpt_debug_sky(HOST_ONLY, C.byref(p), 8, 4, 1, out.ctypes.data) == E_INVALID and name.encode() in L.jpt_debug_last_error(), name
            assert L.jpt_debug_sky_radiance(C.byref(p), d.ctypes.data, 1, out.ctypes.data) == E_INVALID and name.encode() in L.jpt_debug_last_error(), name
        ok = capi.sky_params(suns=[dict(direction=(0.0, 3.0, 0.0), angular_radius=float(F(math.pi / 2)))], sun_angle_max=float(F(math.pi)),
                             sky_curve=1.0 / 64, ground_curve=8.0, exposure=0.0, sky_energy=0.0)
        for w, h, n, code, word in ((0, 4, 1, E_INVALID, "width"), (8, -1, 1, E_INVALID, "height"), (8, 4, 0, E_INVALID, "samples"),
                                    (8, 4, 9, E_INVALID, "samples"), (16385, 4, 1, E_LIMIT, "16384"), (8, 8193, 1, E_LIMIT, "8192")):
            assert L.jpt_set_sky(ctx.h, C.byref(ok), w, h, n) == code and word in ctx.last_error(), (w, h, n, ctx.last_error())
            assert L.jpt_debug_sky(HOST_ONLY, C.byref(ok), w, h, n, out.ctypes.data) == code and word.encode() in L.jpt_debug_last_error()
        # after the checks a host-only context has no device
        for p in (C.byref(ok), None):
            assert L.jpt_set_sky(ctx.h, p, 8, 4, 1) == E_DEVICE and "host-only" in ctx.last_error()
        assert L.jpt_set_sky(ctx.h, None, 16384, 8192, 8) == E_DEVICE
        w, h = C.c_int32(), C.c_int32()
        assert L.jpt_read_environment_f32(ctx.h, None, C.byref(w), C.byref(h)) == E_DEVICE and "jpt_read_environment_f32" in ctx.last_error()
        with pytest.raises(capi.JptError, match="jpt_set_sky"):
            ctx.set_sky()
        with pytest.raises(capi.JptError, match="jpt_read_environment_f32"):
            ctx.read_environment()
    finally:
        ctx.close()
    assert L.jpt_set_sky(None, None, 8, 4, 1) == E_INVALID and L.jpt_read_environment_f32(None, None, None, None) == E_INVALID
    assert L.jpt_multi_set_sky(None, None, 8, 4, 1) == E_INVALID
    assert L.jpt_debug_sky(HOST_ONLY, None, 8, 4, 1, None) == E_INVALID and b"null" in L.jpt_debug_last_error()
    assert L.jpt_debug_sky_radiance(None, None, 1, out.ctypes.data) == E_INVALID and L.jpt_debug_sky_radiance(None, None, 0, None) == capi.OK
    assert L.jpt_debug_pow01(None, None, 1, None) == E_INVALID and L.jpt_debug_pow01(None, None, 0, None) == capi.OK
    with pytest.raises(capi.JptError, match="sky_curve"):
        host.debug_sky(HOST_ONLY, capi.sky_params(sky_curve=9.0), 8, 4, 1)


def test_the_header_the_structs_and_the_wrappers(L, tmp_path):
    offs = lambda S: " && ".join("offsetof(%s, %s) == %d" % (S[0], n, getattr(S[1], n).offset) for n, _ in S[1]._fields_)
    sun, sky = ("jpt_sky_sun", capi.SkySun), ("jpt_sky_params", capi.SkyParams)
    src = tmp_path / "sky.cpp"
    src.write_text('#include "jpt.h"\n#include "jpt_host.hpp"\n#include <cstddef>\n'
                   'static_assert(sizeof(jpt_sky_sun) == %d && sizeof(jpt_sky_params) == %d, "sizes");\n' % (C.sizeof(capi.SkySun), C.sizeof(capi.SkyParams)) +
                   'static_assert(%s, "jpt_sky_sun");\nstatic_assert(%s, "jpt_sky_params");\n' % (offs(sun), offs(sky)) +
                   'static_assert(JPT_SUN_RADIANCE == 0 && JPT_SUN_IRRADIANCE == 1 && JPT_ABI_VERSION == 6, "enums");\n'
                   'void use(jpt_host::PathTracingCamera& cam, const jpt_sky_params& p) { cam.set_sky(); cam.set_sky(&p, 512, 256, 2); int32_t w, h; '
                   'std::vector<float> rgb = cam.read_environment(w, h); (void)rgb; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
    assert C.sizeof(capi.SkySun) == 36 and C.sizeof(capi.SkyParams) == 80 + 4 * 36
    assert capi.SkyParams.suns.offset == 80 and capi.SkyParams.n_suns.offset == 76
    assert (capi.SUN_RADIANCE, capi.SUN_IRRADIANCE) == (ns.SUN_RADIANCE, ns.SUN_IRRADIANCE) == (0, 1)
    assert L.jpt_abi_version() == 6
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for proto in (r"enum \{ JPT_SUN_RADIANCE = 0, JPT_SUN_IRRADIANCE = 1 \};",
                  r"void jpt_sky_defaults\(jpt_sky_params \*out\);",
                  r"int jpt_set_sky\(jpt_ctx \*ctx, const jpt_sky_params \*params[^,]*, int32_t width, int32_t height, int32_t samples\);",
                  r"int jpt_read_environment_f32\(jpt_ctx \*ctx, float \*rgb[^,]*, int32_t \*width, int32_t \*height\);",
                  r"int jpt_multi_set_sky\(jpt_multi \*m, const jpt_sky_params \*params, int32_t width, int32_t height, int32_t samples\);",
                  r"int jpt_debug_sky\(int device_id, const jpt_sky_params \*params, int32_t width, int32_t height, int32_t samples, float \*rgb_out\);",
                  r"int jpt_debug_sky_radiance\(const jpt_sky_params \*params, const float \*dirs3, uint32_t n, float \*rgb_out\);",
                  r"int jpt_debug_pow01\(const float \*b, const float \*e, uint32_t n, float \*out\);"):
        assert re.search(proto, text), proto
    for name in ("jpt_sky_defaults", "jpt_set_sky", "jpt_read_environment_f32", "jpt_multi_set_sky", "jpt_debug_sky", "jpt_debug_sky_radiance", "jpt_debug_pow01"):
        assert name in capi.SYMBOLS and hasattr(L, name), name
    for name in ("set_sky", "read_environment"):
        assert hasattr(host.Context, name), name
    assert hasattr(host.MultiContext, "set_sky")
    csrc = os.path.join(ROOT, "gdpathtracing_amd", "csrc")
    sky_h = open(os.path.join(csrc, "jpt_sky.h")).read()
    assert '#include "jpt_sky.h"' in open(os.path.join(csrc, "jpt_kernels_sky.hip")).read()
    code = re.sub(r"//[^\n]*", "", sky_h)                                                                            # (comments name the functions it replaces)
    assert not re.search(r"\b(?:powf?|exp2f?|log2f?|expf|logf|acosf?|__builtin_(?:pow|exp|log|acos)\w*)\s*\(", code)       # no libm in the pinned arithmetic
