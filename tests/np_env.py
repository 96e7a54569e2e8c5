"""The environment lookup of jpt_set_environment (csrc/jpt_device_math.h atan2_, csrc/jpt_shade.h env_radiance) restated in
vectorised float32 numpy: the same binary32 operations in the same order, so the library's host mirror
and its device function must equal it bit for bit.  Test infrastructure."""
import numpy as np

F = np.float32

# atan(r) ~ r * P(r^2) on [0, 1], highest coefficient first (jpt_device_math.h)
ATAN_P = [F("2.456719521433115e-3"), F("-1.4401350170373917e-2"), F("3.978123888373375e-2"), F("-7.234862446784973e-2"),
          F("1.0498950630426407e-1"), F("-1.4161232113838196e-1"), F("1.9985906779766083e-1"), F("-3.3332598209381104e-1"),
          F("9.999998807907104e-1")]
HALF_PI, PI_F = F("1.57079637"), F("3.14159274")
INV_2PI, INV_PI = F("0.159154943"), F("0.318309886")


def atan2_(y, x):
    y = np.asarray(y, dtype=F)
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        steep = ay > ax
        mx, mn = np.where(steep, ay, ax), np.where(steep, ax, ay)
        r = (mn / mx).astype(F)
        z = (r * r).astype(F)
        p = np.full(z.shape, ATAN_P[0], dtype=F)
        for c in ATAN_P[1:]:
            p = (p * z).astype(F) + c
        a = (p * r).astype(F)
        a = np.where(steep, HALF_PI - a, a)
        a = np.where(x < F(0), PI_F - a, a)
        a = np.where(y < F(0), -a, a)
        return np.where(a == a, a, F(0)).astype(F)


def _column(f, w):
    bad = ~(np.abs(f) < F(1073741824.0))          # NaN, or too large for the modulo (jpt_shade.h env_column)
    i = np.where(bad, F(0), f).astype(np.int64)
    i = np.fmod(i, w)
    return np.where(bad, 0, np.where(i < 0, i + w, i))


def _row(f, h):
    i = np.where(f >= F(h - 1), h - 1, np.where(f <= F(0), 0, np.where(f == f, f, F(0)).astype(np.int64)))
    return np.where(f == f, i, 0)


def _lerp(p, q, t):
    return p + t * (q - p)


def env_radiance(rgb, d, rotation=None, intensity=1.0):
    """rgb: float32 [H, W, 3]; d: float32 [n, 3] world directions -> float32 [n, 3]."""
    rgb = np.asarray(rgb, dtype=F)
    h, w = rgb.shape[0], rgb.shape[1]
    R = np.eye(3, dtype=F) if rotation is None else np.asarray(rotation, dtype=F).reshape(3, 3)
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        m = [R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1] + R[k, 2] * d[:, 2] for k in range(3)]
        phi = atan2_(m[0], -m[2])
        theta = atan2_(np.sqrt(m[0] * m[0] + m[2] * m[2]), m[1])
        fu = (phi * INV_2PI + F(0.5)) * F(w) - F(0.5)
        fv = theta * INV_PI * F(h) - F(0.5)
        i0, j0 = np.floor(fu), np.floor(fv)
        a, b = fu - i0, fv - j0
        a = np.where(a == a, a, F(0))
        b = np.where(b == b, b, F(0))
        x0, x1 = _column(i0, w), _column(i0 + F(1), w)
        y0, y1 = _row(j0, h), _row(j0 + F(1), h)
        t00, t10, t01, t11 = rgb[y0, x0], rgb[y0, x1], rgb[y1, x0], rgb[y1, x1]
        c = _lerp(_lerp(t00, t10, a[:, None]), _lerp(t01, t11, a[:, None]), b[:, None])
        return (c * F(intensity)).astype(F)


def directions(n, seed=0):
    """About n unit directions: random ones, the axes, both poles, the u seam (m.x = +-0 with m.z > 0), signed zeros and
    denormal components."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3)).astype(F)
    v /= np.sqrt((v * v).sum(1, keepdims=True)).astype(F)
    special = []
    tiny = [F(0.0), F(-0.0), F(1e-45), F(-1e-45), F(1e-40), F(-1e-40), F(1e-30), F(-1e-30), F(1e-7), F(-1e-7)]
    for s in (F(1), F(-1)):
        for k in range(3):
            e = np.zeros(3, dtype=F)
            e[k] = s
            special.append(e)
        for t in tiny:
            special.append(np.array([t, s, t], dtype=F))           # near the poles
            special.append(np.array([t, F(0.25), s], dtype=F))     # the seam behind -z ... and in front
            special.append(np.array([t, t, s], dtype=F))
            special.append(np.array([s, t, t], dtype=F))
    sp = np.array(special, dtype=F)
    return np.concatenate([v, sp, -sp], axis=0)
