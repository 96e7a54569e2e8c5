"""The procedural sky of jpt_set_sky (csrc/jpt_sky.h) restated in vectorised float32 numpy: the same binary32 operations in the same
order, so the library's host loop and its kernel must equal it bit for bit -- pow01_, sky_radiance and the texel
loop; and, next to it, the float64 form of the mathematical formula (np.arctan2, **), which shares no code with it.  Parameters are
plain dicts (params()); lib_params() turns one into the capi.SkyParams the library takes.  Test infrastructure."""
import math

import numpy as np

from np_env import atan2_

F = np.float32
HALF_PI, PI_F, TWO_PI = F("1.57079637"), F("3.14159274"), F("6.28318548")
SUN_RADIANCE, SUN_IRRADIANCE = 0, 1
MIN_NORMAL = F("1.17549435e-38")

LOG2_C = [F("0.320598900"), F("0.412198573"), F("0.577078044"), F("0.961796701"), F("2.88539004")]     # 2 / (k ln 2), k = 9, 7, 5, 3, 1
EXP_C = [F("1.98412701e-4"), F("1.38888892e-3"), F("8.33333377e-3"), F("4.16666679e-2"), F("0.166666672"), F("0.5"), F("1.0"), F("1.0")]
LN2, SQRT2 = F("0.693147182"), F("1.41421354")


def params(suns=(), **fields):
    """the defaults of jpt_sky_defaults, then `fields`; suns: dicts of direction, angular_radius, color (1, 1, 1), energy (1), mode (RADIANCE)"""
    p = dict(sky_top_color=(0.385, 0.454, 0.55), sky_horizon_color=(0.6463, 0.6558, 0.6708), sky_curve=0.15, sky_energy=1.0,
             ground_bottom_color=(0.2, 0.169, 0.133), ground_horizon_color=(0.6463, 0.6558, 0.6708), ground_curve=0.02, ground_energy=1.0,
             sun_angle_max=float(F(30.0 * 3.14159265358979323846 / 180.0)), sun_curve=0.15, exposure=1.0)
    for k in fields:
        assert k in p, k
    p.update(fields)
    p["suns"] = [dict(dict(color=(1.0, 1.0, 1.0), energy=1.0, mode=SUN_RADIANCE), **s) for s in suns]
    return p


def lib_params(p):
    from gdpathtracing_amd import capi
    return capi.sky_params(suns=p["suns"], **{k: v for k, v in p.items() if k != "suns"})


def sun_radiance64(s):
    """the disk's radiance as the host derives it: color * energy in float32, or color * energy / (2 pi (1 - cos r)) in float64, rounded"""
    col, en, r = np.asarray(s["color"], F), F(s["energy"]), F(s["angular_radius"])
    if s["mode"] == SUN_IRRADIANCE:
        cap = 2.0 * math.pi * (1.0 - math.cos(float(r)))                 # (libm, as the host)
        return (col.astype(np.float64) * np.float64(en) / cap).astype(F)
    return (col * en).astype(F)


def derived(p):
    """what the host derives once per call (jpt_lighting.cpp sky_params_dev), all float32"""
    d = {k: (np.asarray(v, F) if k.endswith("_color") else F(v)) for k, v in p.items() if k != "suns"}
    for k in ("sky", "ground", "sun"):
        d["inv_%s_curve" % k] = F(1.0) / F(p["%s_curve" % k])
    d["suns"] = []
    for s in p["suns"]:
        v = np.asarray(s["direction"], F).astype(np.float64)
        L = (v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])).astype(F)
        r = F(s["angular_radius"])
        amax = max(F(p["sun_angle_max"]), r)
        span = amax - r
        d["suns"].append(dict(L=L, r=r, amax=amax, inv_span=(F(1.0) / span if span > 0 else F(0.0)), R=sun_radiance64(s)))
    return d


def sincos_(x):
    """jpt_device_math.h sincos_"""
    x = np.asarray(x, F)
    ax = np.abs(x)
    y = np.floor(ax * F(1.27323954473516))
    j = y.astype(np.int64)
    odd = (j & 1) == 1
    j = np.where(odd, j + 1, j) & 7
    y = np.where(odd, y + F(1.0), y)
    r = ((ax - y * F(0.78515625)) - y * F(2.4187564849853515625e-4)) - y * F(3.77489497744594108e-8)
    z = r * r
    ps = ((F(-1.9515295891e-4) * z + F(8.3321608736e-3)) * z - F(1.6666654611e-1)) * z * r + r
    pc = ((F(2.443315711809948e-5) * z - F(1.388731625493765e-3)) * z + F(4.166664568298827e-2)) * z * z - F(0.5) * z + F(1.0)
    s = np.where(j == 0, ps, np.where(j == 2, pc, np.where(j == 4, -ps, -pc)))
    c = np.where(j == 0, pc, np.where(j == 2, -ps, np.where(j == 4, -pc, ps)))
    return np.where(x < 0, -s, s).astype(F), c.astype(F)


def pow01_(b, e):
    """jpt_sky.h pow01_: b^e for b in [0, 1], e in [1/8, 64]"""
    b = np.asarray(b, F)
    e = np.broadcast_to(np.asarray(e, F), b.shape)
    with np.errstate(all="ignore"):
        sub = b < MIN_NORMAL
        bn = np.where(sub, b * F(16777216.0), b).astype(F)
        u = bn.view(np.uint32) if bn.ndim else np.array(bn).reshape(1).view(np.uint32).reshape(())
        ex = (u >> np.uint32(23)).astype(np.int64) - np.where(sub, 151, 127)
        m = ((u & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(F)
        fold = m >= SQRT2
        m = np.where(fold, m * F(0.5), m).astype(F)
        ex = np.where(fold, ex + 1, ex)
        s = ((m - F(1.0)) / (m + F(1.0))).astype(F)
        z = s * s
        p = np.full(b.shape, LOG2_C[0], F)
        for c in LOG2_C[1:]:
            p = p * z + c
        l = ex.astype(F) + p * s
        t = (e * l).astype(F)
        nf = np.floor(t + F(0.5))
        x = (t - nf) * LN2
        q = np.full(b.shape, EXP_C[0], F)
        for c in EXP_C[1:]:
            q = q * x + c
        n = np.clip(np.where(nf == nf, nf, 0), -126, 0).astype(np.int64)
        scale = ((n + 127).astype(np.uint32) << np.uint32(23)).view(F)
        r = (q * scale).astype(F)
        r = np.where(r < MIN_NORMAL, F(0.0), r)
        r = np.where(t < F(-126.0), F(0.0), r)
        r = np.where(b >= F(1.0), F(1.0), r)
        return np.where(b > F(0.0), r, F(0.0)).astype(F)


def clamp_(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def mix_(a, b, t):
    return a * (F(1.0) - t) + b * t


def weight(b, inv_curve):
    return clamp_(F(1.0) - pow01_(clamp_(np.asarray(b, F), F(0.0), F(1.0)), inv_curve), F(0.0), F(1.0)).astype(F)


def gradient(D, theta, upper):
    """[..., 3]: the gradient at polar angles theta, `upper` choosing the sky's or the ground's branch"""
    b = (np.asarray(theta, F) / HALF_PI).astype(F)
    ws = weight(b, D["inv_sky_curve"])[..., None]
    wg = weight(F(2.0) - b, D["inv_ground_curve"])[..., None]
    sky = mix_(D["sky_horizon_color"], D["sky_top_color"], ws) * D["sky_energy"]
    ground = mix_(D["ground_horizon_color"], D["ground_bottom_color"], wg) * D["ground_energy"]
    return np.where(np.asarray(upper)[..., None], sky, ground).astype(F)


def suns_over(D, d, c, upper):
    """the suns, in order, over the colours c [..., 3] of the directions d [..., 3] (only where `upper`)"""
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    for s in D["suns"]:
        L = s["L"]
        cx = L[1] * dz - L[2] * dy
        cy = L[2] * dx - L[0] * dz
        cz = L[0] * dy - L[1] * dx
        a = atan2_(np.sqrt(cx * cx + cy * cy + cz * cz), L[0] * dx + L[1] * dy + L[2] * dz)
        disk = a < s["r"]
        halo = ~disk & (a < s["amax"])
        w = weight(F(1.0) - (a - s["r"]) * s["inv_span"], D["inv_sun_curve"])[..., None]
        blended = mix_(s["R"], c, w)
        c = np.where((disk & upper)[..., None], s["R"], np.where((halo & upper)[..., None], blended, c)).astype(F)
    return c


def sky_radiance(p, dirs):
    """jpt_debug_sky_radiance: float32 [n, 3] for unit directions [n, 3]; theta = atan2_(|d.xz|, d.y)"""
    D = derived(p)
    d = np.asarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        theta = atan2_(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), d[:, 1])
        upper = d[:, 1] >= F(0.0)
        c = suns_over(D, d, gradient(D, theta, upper), upper)
        return (c * D["exposure"]).astype(F)


def sky_map(p, w, h, n):
    """jpt_debug_sky / jpt_set_sky: float32 [h, w, 3], n x n subsamples per texel, sub-rows outside, summed from 0 in that order"""
    D = derived(p)
    total = np.zeros((h, w, 3), F)
    j, i = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    with np.errstate(all="ignore"):
        for sj in range(n):
            v = ((j * n + sj).astype(F) + F(0.5)) / F(h * n)
            theta = (v * PI_F).astype(F)
            st, ct = sincos_(theta)
            upper = ct >= F(0.0)
            g = gradient(D, theta, upper)                                  # [h, 3]: once per sub-row
            for si in range(n):
                u = ((i * n + si).astype(F) + F(0.5)) / F(w * n)
                phi = ((u - F(0.5)) * TWO_PI).astype(F)
                sp, cp = sincos_(phi)
                d = np.stack([st[:, None] * sp[None, :], np.broadcast_to(ct[:, None], (h, w)), -(st[:, None] * cp[None, :])], axis=-1).astype(F)
                up = np.broadcast_to(upper[:, None], (h, w))
                c = suns_over(D, d, np.broadcast_to(g[:, None, :], (h, w, 3)), up)
                total = total + c * D["exposure"]
        return (total * (F(1.0) / F(n * n))).astype(F)


# ---- the mathematical formula in float64 ------------------------------------------------------------------------------------------------

def weight64(b, curve):
    return np.clip(1.0 - np.clip(b, 0.0, 1.0) ** (1.0 / curve), 0.0, 1.0)


def sky_radiance64(p, dirs):
    """the formula of the issue in float64: np.arctan2, ** -- float64 [n, 3]; parameters as float32 values, as the library receives them"""
    P = {k: (np.asarray(v, F).astype(np.float64) if k.endswith("_color") else float(F(v))) for k, v in p.items() if k != "suns"}
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 2]), d[:, 1])
    b = theta / (np.pi / 2)
    mix = lambda a, c, t: a * (1.0 - t) + c * t
    sky = mix(P["sky_horizon_color"], P["sky_top_color"], weight64(b, P["sky_curve"])[:, None]) * P["sky_energy"]
    for s in p["suns"]:
        v = np.asarray(s["direction"], F).astype(np.float64)
        L = v / np.linalg.norm(v)
        r = float(F(s["angular_radius"]))
        amax = max(P["sun_angle_max"], r)
        R = sun_radiance64(s).astype(np.float64)
        a = np.arctan2(np.linalg.norm(np.cross(L, d), axis=1), d @ L)
        span = amax - r
        x = 1.0 - (a - r) / span if span > 0 else np.zeros_like(a)
        halo = mix(R, sky, weight64(x, P["sun_curve"])[:, None])
        sky = np.where((a < r)[:, None], R, np.where((a < amax)[:, None], halo, sky))
    ground = mix(P["ground_horizon_color"], P["ground_bottom_color"], weight64(2.0 - b, P["ground_curve"])[:, None]) * P["ground_energy"]
    return np.where((d[:, 1] >= 0)[:, None], sky, ground) * P["exposure"]


def sky_map64(p, w, h, n):
    """the texel loop with the float64 formula: float64 [h, w, 3]"""
    v = (np.arange(h * n) + 0.5) / (h * n)
    u = (np.arange(w * n) + 0.5) / (w * n)
    theta, phi = np.meshgrid(v * np.pi, (u - 0.5) * 2 * np.pi, indexing="ij")
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=-1)
    c = sky_radiance64(p, d.reshape(-1, 3)).reshape(h, n, w, n, 3)
    return c.mean(axis=(1, 3))


def row_solid_angles(w, h):
    """the exact solid angle of one texel of each row: (2 pi / w) (cos theta_top - cos theta_bottom)"""
    edges = np.cos(np.arange(h + 1) * np.pi / h)
    return (2.0 * np.pi / w) * (edges[:-1] - edges[1:])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
