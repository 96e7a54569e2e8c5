"""jpt_meter restated from its pin ("metering"; include/jpt.h), not from the kernels: the pixel step in
vectorised float32 numpy, the bins from the values' bits (view(np.uint32)), the resolve in Python integers and four float32
operations -- the same operations in the same order, so the library's host form (jpt_debug_meter, device -1), its kernels and
jpt_meter through a context must equal this in every bin and every bit of the result.  Test infrastructure."""
import numpy as np

F = np.float32
FLT_MAX = F(3.402823466e38)
AVERAGE, CENTER_WEIGHTED = 0, 1
EMPTY, FIRST = 1, 2
DEFAULTS = dict(mode=AVERAGE, low_permille=100, high_permille=900, key=0.18, min_exposure=1.0 / 64.0, max_exposure=64.0, adapt=1.0)


def clamp(x, lo, hi):
    """display_clamp: two selects; a NaN gives lo"""
    t = x if x > lo else lo
    return t if t < hi else hi


def bins_of(src, fc=1):
    """per pixel 1.-4.: int [H, W], the bin of every pixel, -1 for a skipped one"""
    with np.errstate(all="ignore"):
        m = (np.asarray(src, F)[..., :3] / F(fc)).astype(F)
        lum = F(0.2126) * m[..., 0] + F(0.7152) * m[..., 1]
        lum = (lum + F(0.0722) * m[..., 2]).astype(F)
        ok = (np.abs(m) <= FLT_MAX).all(-1) & (lum > F(0.0))
    b = (np.ascontiguousarray(lum).view(np.uint32) >> np.uint32(20)).astype(np.int64) - 856
    return np.where(ok, np.clip(b, 0, 255), -1)


def weights_of(height, width, mode):
    """per pixel 5."""
    w = np.ones((height, width), np.int64)
    if mode == CENTER_WEIGHTED:
        x, y = np.arange(width)[None, :], np.arange(height)[:, None]
        w[(4 * x >= width) & (4 * x < 3 * width) & (4 * y >= height) & (4 * y < 3 * height)] = 4
    return w


def histogram(src, fc=1, mode=AVERAGE):
    """the 256 bins as Python integers"""
    b = bins_of(src, fc)
    w = weights_of(b.shape[0], b.shape[1], mode)
    counted = b >= 0
    return [int(v) for v in np.bincount(b[counted], weights=None if mode == AVERAGE else w[counted], minlength=256).astype(np.int64)]


def resolve(hist, prev=None, **params):
    """the resolve: dict(exposure, target, luminance as float32; flags, weight, used as int).  prev None: a FIRST call."""
    p = dict(DEFAULTS, **params)
    key, lo_e, hi_e, adapt = F(p["key"]), F(p["min_exposure"]), F(p["max_exposure"]), F(p["adapt"])
    first = prev is None
    total = sum(hist)
    lo, hi = total * p["low_permille"] // 1000, total * p["high_permille"] // 1000
    cum = used = S = 0
    for b, h in enumerate(hist):
        c = max(0, min(cum + h, hi) - max(cum, lo))
        used += c
        S += c * (2 * b + 1)
        cum += h
    flags = FIRST if first else 0
    if used == 0:
        e = clamp(F(1.0), lo_e, hi_e) if first else F(prev)
        return dict(exposure=e, target=e, luminance=F(0.0), flags=flags | EMPTY, weight=total, used=0)
    q = (S * 32768) // used
    l_avg = np.array([0x35800000 + ((q << 4) & 0xFFFFFFFF)], np.uint32).view(F)[0]
    with np.errstate(all="ignore"):
        e_t = clamp(F(key / l_avg), lo_e, hi_e)
        if first:
            e = e_t
        else:
            d = F(e_t - F(prev))
            step = F(d * adapt)
            e = F(F(prev) + step)
    return dict(exposure=e, target=e_t, luminance=l_avg, flags=flags, weight=total, used=used)


def meter(src, fc=1, prev=None, **params):
    """jpt_meter on sums (float32 [H, W, >= 3]) and the frame count, or on an image with fc = 1: (bins, result)"""
    p = dict(DEFAULTS, **params)
    p.pop("source", None)
    hist = histogram(src, fc, p["mode"])
    return hist, resolve(hist, prev, **p)


def bits(v):
    return int(np.array([v], F).view(np.uint32)[0])


def bin_lower_bound(b):
    """the smallest float32 of bin b (b >= 1; bin 0 also takes everything below 2^-20)"""
    return np.array([(b + 856) << 20], np.uint32).view(F)[0]


def edge_image(width, height, seed=0):
    """float32 [H, W, 4] with what the pin names planted over a seeded image that spans the whole range: NaN, +-inf, negative values,
    zeros and denormals, values below 2^-20 and at and above 2^12, and for a sweep of bins the exact lower bound of the bin and the
    float just below it (as grey pixels: the luminance of a grey v is v up to rounding, so these land on and about the bounds)"""
    rng = np.random.default_rng(seed)
    n = width * height
    img = np.zeros((n, 4), F)
    img[:, :3] = (rng.random((n, 3)) * 2.0 ** rng.uniform(-24, 14, (n, 1))).astype(F)
    img[:, 3] = rng.random(n).astype(F)
    special = [np.nan, np.inf, -np.inf, -1.0, -1e-30, 0.0, -0.0, 1e-45, 1e-39, 1.1754942e-38, 2.0 ** -21, 2.0 ** -20, 4096.0, 5000.0, 1e30, 3e38]
    rows = [(v, v, v) for v in special]
    rows += [(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (3e38, 3e38, 3e38), (-1.0, 1.0, 0.5), (4.0, -1.0, 0.0)]
    for b in list(range(1, 256, 7)) + [255]:
        v = bin_lower_bound(b)
        rows += [(v, v, v), (np.nextafter(v, F(0)),) * 3, (np.nextafter(v, F(np.inf)),) * 3]
    if n > len(rows):
        where = rng.choice(n, len(rows), replace=False)
        for i, r in zip(where, rows):
            img[i, :3] = r
    return img.reshape(height, width, 4)
