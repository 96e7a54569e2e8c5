"""jpt_display restated in vectorised float32 numpy from its pin ("the display transform"; include/jpt.h), not
from the kernels: base, bright pass, the 4 x 4 binomial pyramid down, the 2 x tent back up, the composite, the three tone maps and
the two transfers -- the same binary32 operations in the same order, so the library's host form (jpt_debug_display, device -1) and
its kernels must equal this bit for bit.  The sRGB table is made here in float64 from the definition; the library's own comes from
jpt_debug_display_srgb_table.  Test infrastructure."""
import numpy as np

F = np.float32
W4 = (F(0.125), F(0.375), F(0.375), F(0.125))
FLT_MAX = F(3.402823466e38)
ACES_REF, REINHARD, CLAMP = 0, 1, 2
LINEAR, SRGB = 0, 1
DEFAULTS = dict(tonemap=ACES_REF, transfer=LINEAR, bloom_levels=0, exposure=1.0, white=4.0, bloom_threshold=1.0, bloom_strength=0.25)


def srgb_table():
    """T[1..255] as float32 [255]: the binary32 nearest to eotf((k - 0.5) / 255), evaluated in float64"""
    e = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    return np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4).astype(F)


def clamp(x, lo, hi):
    """the project's clamp_ (fmin(fmax(x, lo), hi)) as the two selects of jpt_display.h: a NaN gives lo, -0 gives +0"""
    t = np.where(x > lo, x, lo).astype(F)
    return np.where(t < hi, t, hi).astype(F)


def base(src, fc, exposure):
    """step 1: c = (sum.rgb / fc) * exposure"""
    return ((np.asarray(src, F)[..., :3] / F(fc)).astype(F) * F(exposure)).astype(F)


def bright(c, threshold):
    """step 2: B, 0 where a channel is not finite or the luminance is not over the threshold"""
    with np.errstate(all="ignore"):
        lum = F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]
        lum = lum + F(0.0722) * c[..., 2]
        ok = (np.abs(c) <= FLT_MAX).all(-1) & (lum > F(threshold))
        k = (lum - F(threshold)) / lum
        return np.where(ok[..., None], c * k[..., None], F(0.0)).astype(F)


def down(level):
    """step 3: D_k+1 from D_k, float32 [h, w, 3] -> [(h + 1) >> 1, (w + 1) >> 1, 3]"""
    h, w = level.shape[:2]
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    ys, xs = np.arange(ch), np.arange(cw)
    s = np.zeros((ch, cw, 3), F)
    for j in range(4):
        rows = np.clip(2 * ys - 1 + j, 0, h - 1)
        for i in range(4):
            cols = np.clip(2 * xs - 1 + i, 0, w - 1)
            s = s + level[rows][:, cols] * (W4[j] * W4[i])
    return s.astype(F)


def _tent_axis(n, coarse_n):
    """the two taps of the tent along one axis for p = 0..n-1: (indices [2, n], weights [2, n])"""
    p = np.arange(n)
    even = (p & 1) == 0
    half = p >> 1
    i0 = np.where(even, half - 1, half)
    i1 = np.where(even, half, half + 1)
    w0 = np.where(even, F(0.25), F(0.75)).astype(F)
    w1 = np.where(even, F(0.75), F(0.25)).astype(F)
    return np.clip(np.stack([i0, i1]), 0, coarse_n - 1), np.stack([w0, w1])


def tent(coarse, h, w):
    """step 4's T: the coarse level [ch, cw, 3] seen at h x w"""
    iy, wy = _tent_axis(h, coarse.shape[0])
    ix, wx = _tent_axis(w, coarse.shape[1])
    s = np.zeros((h, w, 3), F)
    for j in range(2):
        for i in range(2):
            wt = (wy[j][:, None] * wx[i][None, :]).astype(F)
            s = s + coarse[iy[j]][:, ix[i]] * wt[..., None]
    return s.astype(F)


def bloom(c, levels, threshold):
    """steps 2-4: T(U_1) at the size of c"""
    h, w = c.shape[:2]
    d = [bright(c, threshold)]
    for _ in range(levels):
        d.append(down(d[-1]))
    u = d[levels]
    for k in range(levels - 1, 0, -1):
        u = (d[k] + tent(u, d[k].shape[0], d[k].shape[1])).astype(F)
    return tent(u, h, w)


def aces(x):
    a, b, c, d, e = F(2.51), F(0.03), F(2.43), F(0.59), F(0.14)
    return clamp((x * (a * x + b)) / (x * (c * x + d) + e), F(0.0), F(1.0))


def tonemap(o, mode, white):
    if mode == ACES_REF:
        return aces(o)
    if mode == REINHARD:
        w2 = F(white) * F(white)
        return clamp((o * (F(1.0) + o / w2)) / (F(1.0) + o), F(0.0), F(1.0))
    return clamp(o, F(0.0), F(1.0))


def encode(v, transfer, table=None):
    """step 7: uint8 codes of the tone-mapped values"""
    if transfer == LINEAR:
        return np.floor(clamp(v, F(0.0), F(1.0)) * F(255.0) + F(0.5)).astype(np.uint8)
    t = srgb_table() if table is None else np.asarray(table, F)
    return np.where(np.isnan(v), 0, np.searchsorted(t, v, side="right")).astype(np.uint8)      # #{k : T[k] <= v}; a NaN counts nothing


def composite(src, fc=1, tonemap=ACES_REF, transfer=LINEAR, bloom_levels=0, exposure=1.0, white=4.0, bloom_threshold=1.0,
              bloom_strength=0.25, source=0):
    """steps 1-5: o, float32 [H, W, 3], before the tone map"""
    with np.errstate(all="ignore"):
        c = base(src, fc, exposure)
        if bloom_levels == 0:
            return c
        s = F(bloom_strength) / F(bloom_levels)
        return (c + bloom(c, bloom_levels, bloom_threshold) * s).astype(F)


def display(src, fc=1, table=None, **params):
    """jpt_display's two images from sums (float32 [H, W, >= 3]) and the frame count, or from an image with fc = 1:
    (float32 [H, W, 4] = (v, 1), uint8 [H, W, 4] = (codes, 255))"""
    prm = dict(DEFAULTS, **params)
    with np.errstate(all="ignore"):
        v = tonemap(composite(src, fc, **prm), prm["tonemap"], prm["white"])
        q = encode(v, prm["transfer"], table)
    out = np.ones(v.shape[:2] + (4,), F)
    out[..., :3] = v
    ldr = np.full(v.shape[:2] + (4,), 255, np.uint8)
    ldr[..., :3] = q
    return out, ldr


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def synthetic_image(width, height, seed=0):
    """float32 [H, W, 4]: a seeded image of values mostly under 1 with a tenth of the pixels up to 1e3 and a few up to 1e6, exact zeros
    and negative values, and NaN, +inf and -inf pixels planted (images of more than 16 pixels)"""
    rng = np.random.default_rng(seed)
    img = np.zeros((height, width, 4), F)
    rgb = rng.random((height, width, 3)) * 1.5
    hot = rng.random((height, width)) < 0.1
    rgb = np.where(hot[..., None], rgb * 10.0 ** rng.uniform(0, 3, (height, width, 1)), rgb)
    rgb = np.where((rng.random((height, width)) < 0.02)[..., None], 0.0, rgb)
    rgb = np.where((rng.random((height, width)) < 0.02)[..., None], -rgb, rgb)
    img[..., :3] = rgb.astype(F)
    img[..., 3] = rng.random((height, width)).astype(F)     # unused by the transform
    flat = img.reshape(-1, 4)
    n = len(flat)
    if n > 16:
        flat[n // 3, 0] = np.nan
        flat[n // 2, 1] = np.inf
        flat[(2 * n) // 3, 2] = -np.inf
        flat[n - 1, :3] = np.nan
        flat[7, :3] = 1e6
        flat[11, :3] = (1e6, 0.0, 3.0)
        flat[13, :3] = 0.0
    return img
