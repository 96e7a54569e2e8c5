"""The map's sampler and lookup at the sizes maps come in (1024 x 2048 to 2048 x 4096, and rows or columns as long as the limits
allow) against plain float64, not against a restatement of the same binary32 operations.  CPU (the host mirror, which builds the
same tables bit for bit): every texel's realized mass from the float32 tables against its weight, and the bias that difference
leaves in the MIS estimate of Lambertian irradiance.  GPU: the device tables against the host mirror, the pdf the device sampler
returns against the float64 density where its direction falls, an env-only Monte Carlo estimate against a float64 quadrature
(the sin theta Jacobian, the 2 pi^2 constant, orientation and rotation), and the device lookup against a float64 bilinear lookup."""
import ctypes as C
import functools

import numpy as np
import pytest

from gdpathtracing_amd import capi

import np_env
from test_gpu_env_sampling import ROT, sun_map

F = np.float32
HOST_ONLY = -1
EPS32 = 2.0 ** -24
NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


@functools.lru_cache(maxsize=None)
def real_map(name):
    """(h, w) A: 1024 x 2048, sun_map's sky at 0.5 with a 4 x 4 sun of 5e4; B: 2048 x 4096, the same with a 6 x 6 sun; C:
    2048 x 4096, a dim sky at 0.01 with a 6 x 6 sun of 1e5 whose first row is the equator row h / 2.  (Shared: not to be written.)"""
    if name == "C":
        rgb = np.roll(sun_map(2048, 4096, sun=(1e5, 1e5, 1e5), ambient=0.01, size=(6, 6)), 2048 // 2 - 2048 // 6, axis=0)
    else:
        h, w, n = (1024, 2048, 4) if name == "A" else (2048, 4096, 6)
        rgb = sun_map(h, w, sun=(5e4, 5e4, 5e4), ambient=0.5, size=(n, n))
    rgb = np.ascontiguousarray(rgb, dtype=F)
    rgb.flags.writeable = False
    return rgb


def _ptr(a):
    return None if a is None else a.ctypes.data


def tables(L, dev, rgb):
    h, w = rgb.shape[:2]
    cond, marg, tot = np.zeros((h, w), F), np.zeros(h, F), np.zeros(1, F)
    assert L.jpt_debug_env_tables(dev, _ptr(rgb), w, h, _ptr(cond), _ptr(marg), _ptr(tot)) == capi.OK, L.jpt_debug_last_error()
    return cond, marg, F(tot[0])


def lum64(rgb):
    r = rgb.astype(np.float64)
    return 0.2126 * r[..., 0] + 0.7152 * r[..., 1] + 0.0722 * r[..., 2]


def weights64(rgb):
    """a texel's weight in float64: luminance times sin theta at its row's centre"""
    h = rgb.shape[0]
    return lum64(rgb) * np.sin((np.arange(h) + 0.5) / h * np.pi)[:, None]


def realized_mass(cond, marg):
    """float64 [h, w]: the probability with which env_sample draws each texel, (marg_i - marg_i-1) (cond_ij - cond_ij-1)"""
    dm = np.diff(marg.astype(np.float64), prepend=0.0)
    dc = np.diff(cond.astype(np.float64), axis=1, prepend=0.0)
    return dm[:, None] * dc


def mis_bias(rgb, real):
    """Relative bias, per normal of NORMALS (map coordinates), of the MIS estimate of the Lambertian irradiance integral
    I = int lum(w) max(0, n.w) dw, lum constant over each texel as the sampler's density is.  The BRDF strategy (cosine sampling)
    is exact; the map strategy draws texel t with its realized mass but weighs the sample with the claimed density (weight / total),
    so its expectation is sum_t r_t int_t lum cos w_map dw, r_t = realized / claimed mass, w_map = p_map^2 / (p_map^2 + p_brdf^2):
    bias = sum_t (r_t - 1) int_t lum cos w_map dw / I, each texel's integral at its centre."""
    h, w = real.shape
    wt = weights64(rgb)
    want = wt / wt.sum()
    lum = lum64(rgb)
    th = (np.arange(h) + 0.5) / h * np.pi
    ph = ((np.arange(w) + 0.5) / w - 0.5) * 2.0 * np.pi
    dom = 2.0 * np.pi / w * (np.cos(np.arange(h) / h * np.pi) - np.cos((np.arange(h) + 1.0) / h * np.pi))
    sp, cp = np.sin(ph)[None, :], np.cos(ph)[None, :]
    num, den = np.zeros(len(NORMALS)), np.zeros(len(NORMALS))
    for a in range(0, h, 256):
        b = min(h, a + 256)
        st, ct = np.sin(th[a:b])[:, None], np.cos(th[a:b])[:, None]
        p_map = want[a:b] * (w * h) / (2.0 * np.pi ** 2 * st)
        with np.errstate(all="ignore"):
            r = np.where(want[a:b] > 0, real[a:b] / want[a:b], 1.0)
        lw = lum[a:b] * dom[a:b, None]
        for k, n in enumerate(NORMALS):
            c = np.maximum(0.0, n[0] * st * sp + n[1] * ct - n[2] * st * cp)
            p_b = c / np.pi
            with np.errstate(all="ignore"):
                w_map = np.where(p_map > 0, p_map * p_map / (p_map * p_map + p_b * p_b), 0.0)
            num[k] += ((r - 1.0) * lw * c * w_map).sum()
            den[k] += (lw * c).sum()
    return num / den


# ---- the tables against float64 (CPU) ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    return capi.lib()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_realized_texel_masses_against_float64(L, name):
    """Each texel's realized mass from the float32 tables against weight / sum of weights in float64: the mass-weighted
    discrepancy (the L1 distance of the two distributions) <= 5e-4, texels holding >= 1e-6 of the mass within 2e-4 relative, and
    the bias this leaves in the MIS estimate of Lambertian irradiance <= 1e-4 for six normals."""
    rgb = real_map(name)
    cond, marg, _ = tables(L, HOST_ONLY, rgb)
    real = realized_mass(cond, marg)
    wt = weights64(rgb)
    want = wt / wt.sum()
    disc = float(np.abs(real - want).sum())
    big = want >= 1e-6
    rel = float(np.abs(real[big] / want[big] - 1.0).max())
    never = (real == 0) & (want > 0)
    bias = mis_bias(rgb, real)
    print("map %s: mass-weighted discrepancy %.3g, largest relative error of texels with >= 1e-6 of the mass %.3g (%d texels), "
          "never drawn though weighted %d texels holding %.3g of the mass, MIS irradiance bias per normal %s" % (
              name, disc, rel, int(big.sum()), int(never.sum()), float(want[never].sum()), np.array2string(bias, precision=3)))
    assert disc <= 5e-4
    assert rel <= 2e-4
    assert (np.abs(bias) <= 1e-4).all()


# ---- the device tables and sampler (GPU) ------------------------------------------------------------------------------------

N_XI = 1 << 24
CHUNK = 1 << 22


def _shape_map(shape):
    return real_map(shape) if isinstance(shape, str) else sun_map(*shape, sun=(5e4, 5e4, 5e4), size=(3, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B", (64, 16384), (8192, 64)], ids=["A", "B", "widest", "tallest"])
def test_device_tables_equal_the_host_mirror_at_real_sizes(hiplib, shape):
    rgb = _shape_map(shape)
    dev, host = tables(hiplib, 0, rgb), tables(hiplib, HOST_ONLY, rgb)
    assert np.array_equal(dev[0].view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(dev[1].view(np.uint32), host[1].view(np.uint32))
    assert dev[2].view(np.uint32) == host[2].view(np.uint32)


def quadrature(lum, nm):
    """float64 int lum(m) max(0, nm_k . m) dm over the sphere of map directions for each row nm_k, lum constant over each texel:
    the midpoint rule on 2 x 2 points per texel"""
    h, w = lum.shape
    th = (np.arange(2 * h) + 0.5) / (2 * h) * np.pi
    ph = ((np.arange(2 * w) + 0.5) / (2 * w) - 0.5) * 2.0 * np.pi
    sp, cp = np.sin(ph)[None, :], np.cos(ph)[None, :]
    out = np.zeros(len(nm))
    for a in range(0, 2 * h, 256):
        b = min(2 * h, a + 256)
        st, ct = np.sin(th[a:b])[:, None], np.cos(th[a:b])[:, None]
        lw = np.repeat(np.repeat(lum[a // 2:(b + 1) // 2], 2, axis=0)[(a % 2):(a % 2) + b - a], 2, axis=1) * st
        for k, n in enumerate(nm):
            out[k] += (lw * np.maximum(0.0, n[0] * st * sp + n[1] * ct - n[2] * st * cp)).sum()
    return out * (np.pi / (2 * h)) * (2.0 * np.pi / (2 * w))


def sampler_against_float64(L, dev, rgb, n=N_XI, seed=17):
    """n samples of env_sample under ROT.  Returns (of the samples with sin theta > 1e-3: the fraction whose pdf misses the float64
    density at the texel the float64 mapping of the returned direction falls in by more than 2e-4 relative, and how many of those
    lie farther than 5e-7 rad from that texel's edges; the env-only Monte Carlo estimate of int lum max(0, n.w) dw per world normal
    of NORMALS, lum and density both the float64 ones of that texel; its standard error; the float64 quadrature of the same)"""
    h, w = rgb.shape[:2]
    xi = np.random.default_rng(seed).random((n, 2), dtype=F)
    d, p = np.zeros((n, 3), F), np.zeros(n, F)
    assert L.jpt_debug_env_sample(dev, _ptr(rgb), w, h, _ptr(ROT), _ptr(xi), n, _ptr(d), _ptr(p)) == capi.OK, L.jpt_debug_last_error()
    del xi
    assert (p > 0).all() and np.isfinite(p).all()
    wt = weights64(rgb)
    total = wt.sum()
    lum = lum64(rgb)
    R = ROT.astype(np.float64)
    away = missed = inside = 0
    s1, s2 = np.zeros(len(NORMALS)), np.zeros(len(NORMALS))
    for a in range(0, n, CHUNK):
        dd, pp = d[a:a + CHUNK].astype(np.float64), p[a:a + CHUNK].astype(np.float64)
        m = dd @ R.T                                        # m = R d
        s = np.hypot(m[:, 0], m[:, 2])
        fv = np.arctan2(s, m[:, 1]) / np.pi * h
        fu = (np.arctan2(m[:, 0], -m[:, 2]) / (2.0 * np.pi) + 0.5) * w
        i = np.clip(np.floor(fv).astype(np.int64), 0, h - 1)
        j = np.floor(fu).astype(np.int64) % w
        with np.errstate(all="ignore"):
            want = wt[i, j] / total * (w * h) / (2.0 * np.pi ** 2 * s)
        ok = s > 1e-3
        edge = np.minimum(np.abs(fv - np.round(fv)) * np.pi / h, np.abs(fu - np.round(fu)) * 2.0 * np.pi / w * s)   # rad of arc
        miss = ok & ~(np.abs(pp - want) <= 2e-4 * want)
        away += int(ok.sum())
        missed += int(miss.sum())
        inside += int((miss & (edge > 5e-7)).sum())
        f = lum[i, j][:, None] * np.maximum(0.0, dd @ NORMALS.T) / want[:, None]
        s1 += f.sum(axis=0)
        s2 += (f * f).sum(axis=0)
    est = s1 / n
    se = np.sqrt(np.maximum(s2 / n - est * est, 0.0) / n)
    return missed / away, inside, est, se, quadrature(lum, NORMALS @ R.T)   # n . R^T m = (R n) . m


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_sampler_against_float64(hiplib, name):
    """2^24 draws of the device sampler under ROT, away from the poles (sin theta > 1e-3): the returned pdf is the float64
    weight / total * w h / (2 pi^2 sin theta) of the texel where the float64 mapping of the returned direction falls, within 2e-4,
    except in a boundary sliver -- every miss lies within 5e-7 rad of that texel's edge, where the float32 direction may map to
    the neighbour (whose sin theta or luminance differs by more than 2e-4), and the sliver holds at most 2e-4 of the draws (it
    grows with the resolution: 6e-5 for A, 1.2e-4 for B).  And the distribution of the directions: the env-only estimate of
    int L max(0, n.w) dw, L the texel's luminance (the function the density follows, so the estimate has little variance) over
    the float64 density, agrees with a float64 quadrature within 5 sigma + 1e-4 relative for six normals."""
    sliver, inside, est, se, want = sampler_against_float64(hiplib, 0, real_map(name))
    print("map %s: sliver fraction %.3g (misses away from an edge: %d); estimate / quadrature - 1 per normal %s (sigma %s)" % (
        name, sliver, inside, np.array2string(est / want - 1.0, precision=3),
        np.array2string(se / want, formatter={"float_kind": lambda x: "%.2g" % x})))
    assert inside == 0
    assert sliver <= 2e-4
    assert (np.abs(est - want) <= 5.0 * se + 1e-4 * np.abs(want)).all()


# ---- the device lookup against float64 (GPU) ------------------------------------------------------------------------------------

def lookup64(rgb, d, rot):
    """float64 bilinear lookup of world directions d [n, 3] (float32) with exact atan2: m = R d in float32 as the kernels form it
    (the one binary32 step kept: at the poles the azimuth of a rounded m is anyone's), then phi, theta, the texel coordinates, the
    column wrap and the row clamp in float64.  Returns the value [n, 3] and its bound: the largest neighbouring-texel difference
    around the sample times how far atan2_'s 3.3e-7 rad and the rounding of fu, fv move the texel coordinates, plus 4 ulps of the
    largest texel involved."""
    h, w = rgb.shape[:2]
    R = np.asarray(rot, F)
    m = [(R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1] + R[k, 2] * d[:, 2]).astype(np.float64) for k in range(3)]
    pole = (m[0] == 0) & (m[2] == 0)                       # phi undefined: atan2_ answers 0 there
    phi = np.where(pole, 0.0, np.arctan2(m[0], -m[2]))
    theta = np.arctan2(np.hypot(m[0], m[2]), m[1])
    fu = (phi / (2.0 * np.pi) + 0.5) * w - 0.5
    fv = theta / np.pi * h - 0.5
    i0, j0 = np.floor(fu), np.floor(fv)
    a, b = (fu - i0)[:, None], (fv - j0)[:, None]
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    t = rgb.astype(np.float64)
    col = lambda k: (i0 + k) % w
    row = lambda k: np.clip(j0 + k, 0, h - 1)
    t00, t10, t01, t11 = t[row(0), col(0)], t[row(0), col(1)], t[row(1), col(0)], t[row(1), col(1)]
    val = (1.0 - b) * ((1.0 - a) * t00 + a * t10) + b * ((1.0 - a) * t01 + a * t11)
    blk = np.stack([np.stack([t[row(r), col(c)] for c in range(-1, 3)], axis=1) for r in range(-1, 3)], axis=1)   # [n, 4, 4, 3]
    du = np.abs(np.diff(blk, axis=2)).max(axis=(1, 2))
    dv = np.abs(np.diff(blk, axis=1)).max(axis=(1, 2))
    big = np.abs(blk[:, 1:3, 1:3]).max(axis=(1, 2))
    dfu = 3.3e-7 * w / (2.0 * np.pi) + 4.0 * EPS32 * (w + 1)
    dfv = (3.3e-7 + 2.0 * EPS32) * h / np.pi + 4.0 * EPS32 * (h + 1)
    return val, du * dfu + dv * dfv + 4.0 * EPS32 * big


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(1, 1), (1, 2048), (1024, 1), (1024, 2048), (64, 16384)], ids=["1x1", "1xW", "Hx1", "A", "widest"])
def test_device_lookup_against_float64(hiplib, hw):
    """jpt_debug_env_lookup on the device against lookup64 within its bound, on a million directions with the poles, the seam
    (u wrap), signed zeros and denormal components among them"""
    h, w = hw
    rgb = np.ascontiguousarray(real_map("A") if hw == (1024, 2048) else sun_map(h, w, sun=(5e4, 5e4, 5e4), ambient=0.5, size=(3, 3)))
    d = np_env.directions(1_000_000, seed=23)
    got = np.zeros_like(d)
    assert hiplib.jpt_debug_env_lookup(0, _ptr(rgb), w, h, _ptr(ROT), C.c_float(1.0), _ptr(d), len(d), _ptr(got)) == capi.OK, \
        hiplib.jpt_debug_last_error()
    want, bound = lookup64(rgb, d, ROT)
    err = np.abs(got.astype(np.float64) - want)
    worst = int(np.argmax((err / np.maximum(bound, 1e-300)).max(axis=1)))
    print("lookup %dx%d: largest error / bound %.3g (direction %s)" % (h, w, float((err[worst] / np.maximum(bound[worst], 1e-300)).max()),
                                                                       d[worst].tolist()))
    assert (err <= bound).all()
