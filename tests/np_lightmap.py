"""jpt_bake_finish restated in vectorised float32 numpy from its pin ("finishing a lightmap"; include/jpt.h), not
from the kernels: the guides of the texel images, the chart-aware a-trous passes and the dilation -- the same binary32 operations in
the same order, so the library's host form (jpt_debug_bake_finish, device -1) and its kernels must equal this bit for bit.  Test
infrastructure, with the images the lightmap tests share."""
import numpy as np

import np_bake as nb
from np_denoise import H5, _finite3, _pos, _shift, same_bits   # noqa: F401  (same_bits: for the tests)

F = np.float32
DEFAULTS = dict(passes=3, normal_power_log2=4, dilate=4, sigma_distance=4.0, sigma_plane=1.0, sigma_color=4.0)


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


# ---- 1. prepare ------------------------------------------------------------------------------------------------------------------------------

def guides(position4, normal4):
    """(xg, ng) float32 [H, W, 4]: (position, fp2 | invalid: 0, 0, 0, -1) and (normalised normal, 0 | invalid: zeros); fp2 = the least
    squared distance to a valid 4-neighbour, in the order -x, +x, -y, +y (0: none)"""
    with np.errstate(all="ignore"):
        p4, n4 = np.asarray(position4, F), np.asarray(normal4, F)
        valid = nb.texel_valid(n4)
        fp2 = np.zeros(valid.shape, F)
        found = np.zeros(valid.shape, bool)
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            pq, inside = _shift(p4, dx, dy)
            vq, _ = _shift(valid, dx, dy)
            ok = inside & vq
            d = pq[..., :3] - p4[..., :3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(F)
            fp2 = np.where(ok, np.where(found, np.where(d2 < fp2, d2, fp2), d2), fp2).astype(F)
            found = found | ok
        n3 = n4[..., :3]
        inv = F(1.0) / np.sqrt(_dot3(n3, n3))
        xg = np.zeros(p4.shape, F)
        xg[..., :3] = p4[..., :3]
        xg[..., 3] = fp2
        ng = np.zeros(p4.shape, F)
        ng[..., :3] = n3 * inv[..., None]
        xg = np.where(valid[..., None], xg, np.array([0, 0, 0, -1], F)).astype(F)
        ng = np.where(valid[..., None], ng, F(0.0)).astype(F)
    return xg, ng


def colour0(mean, xg):
    """i_0 = (mean.rgb, 1) of a valid texel, zeros of an invalid one: float32 [H, W, 4]"""
    out = np.ones(xg.shape, F)
    out[..., :3] = np.asarray(mean, F)[..., :3]
    return np.where((xg[..., 3] < 0)[..., None], F(0.0), out).astype(F)


# ---- 2. filter -------------------------------------------------------------------------------------------------------------------------------

def filter_pass(ik, xg, ng, k, npow, sigma_distance, sigma_plane, sigma_color):
    """i_k -> i_k+1, float32 [H, W, 4] = (rgb, state)"""
    s = 1 << k
    sc = F(sigma_color)
    for _ in range(k):
        sc = F(sc * F(0.5))
    sc2 = F(sc * sc)
    sd2 = F(F(sigma_distance) * F(sigma_distance))
    sp2 = F(F(sigma_plane) * F(sigma_plane))
    xp, fp2, n_p = xg[..., :3], xg[..., 3], ng[..., :3]
    c3 = ik[..., :3]
    acc = np.zeros_like(c3)
    wsum = np.zeros(ik.shape[:2], F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, inside = _shift(c3, s * dx, s * dy)
            xq, _ = _shift(xg, s * dx, s * dy)
            nq, _ = _shift(ng, s * dx, s * dy)
            q_valid = ~(xq[..., 3] < 0)
            d = xq[..., :3] - xp
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            r2 = F(s * s * (dx * dx + dy * dy)) * fp2
            near = d2 <= sd2 * r2
            wn = _pos(_dot3(n_p, nq[..., :3]))
            for _ in range(npow):
                wn = wn * wn
            pd = n_p[..., 0] * d[..., 0] + n_p[..., 1] * d[..., 1] + n_p[..., 2] * d[..., 2]
            g = _pos(F(1.0) - (pd * pd) / (sp2 * r2))
            dc = cq - c3
            wc = F(1.0) / (F(1.0) + (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2]) / sc2)
            ew = np.where(q_valid & near, (wn * g) * wc, F(0.0)).astype(F)
            if dx == 0 and dy == 0:
                ew = np.ones_like(ew)
            wt = ((H5[dy + 2] * H5[dx + 2]) * ew).astype(F)
            wt = np.where(_finite3(cq) & (ew == ew) & inside, wt, F(0.0)).astype(F)
            use = wt != 0
            acc = acc + np.where(use[..., None], cq * wt[..., None], F(0.0)).astype(F)
            wsum = wsum + wt
    out = np.ones(ik.shape, F)
    out[..., :3] = np.where(_finite3(c3)[..., None], acc / wsum[..., None], c3)
    return np.where((xg[..., 3] < 0)[..., None], F(0.0), out).astype(F)


# ---- 3. dilate -------------------------------------------------------------------------------------------------------------------------------

def dilate_pass(img):
    """one ring: a texel of state 0 with an 8-neighbour of state > 0 and finite colour takes their weighted mean and state 0.5"""
    acc = np.zeros(img.shape[:2] + (3,), F)
    wsum = np.zeros(img.shape[:2], F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            if dx == 0 and dy == 0:
                continue
            q, inside = _shift(img, dx, dy)
            ok = inside & (q[..., 3] > 0) & _finite3(q)
            wt = F(2.0) if (dx == 0 or dy == 0) else F(1.0)
            acc = acc + np.where(ok[..., None], q[..., :3] * wt, F(0.0)).astype(F)
            wsum = wsum + np.where(ok, wt, F(0.0)).astype(F)
    filled = np.full(img.shape, 0.5, F)
    filled[..., :3] = acc / wsum[..., None]
    fill = (img[..., 3] == 0) & (wsum > 0)
    return np.where(fill[..., None], filled, img).astype(F)


def finish(mean, position4, normal4, passes=3, normal_power_log2=4, dilate=4, sigma_distance=4.0, sigma_plane=1.0, sigma_color=4.0):
    """the whole transform on a mean image (float32 [H, W, >= 3]) -> the lightmap (r, g, b, coverage), float32 [H, W, 4]"""
    with np.errstate(all="ignore"):
        xg, ng = guides(position4, normal4)
        img = colour0(mean, xg)
        for k in range(passes):
            img = filter_pass(img, xg, ng, k, normal_power_log2, sigma_distance, sigma_plane, sigma_color)
        for _ in range(dilate):
            img = dilate_pass(img)
    return img


# ---- the images of the tests -----------------------------------------------------------------------------------------------------------------

def three_charts(w=70, h=41):
    """(truth [H, W, 4], position4, normal4, (a, b, c) masks): the atlas of the bleeding and noise tests.  Chart A (x 2..29, y 2..37):
    the plane z = 0, texels of 0.1 x 0.3 world units, truth exactly 1.  Chart B (x 30..59, touching A in the atlas): the same
    orientation 50 units away (the plane z = 50), texels of 0.1 x 0.1, truth a ramp 1 + 0.01 (x - 30) along x.  Chart C (x 60..67): a
    wall with normal +x that meets B's edge and runs down from it, truth exactly 2."""
    assert (w, h) == (70, 41)
    ys, xs = np.mgrid[0:h, 0:w]
    rows = (ys >= 2) & (ys <= 37)
    a, b, c = rows & (xs >= 2) & (xs <= 29), rows & (xs >= 30) & (xs <= 59), rows & (xs >= 60) & (xs <= 67)
    p4, n4, truth = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    p4[a, 0], p4[a, 1] = ((xs[a] - 2 + 0.5) * 0.1).astype(F), ((ys[a] - 2 + 0.5) * 0.3).astype(F)
    n4[a] = (0, 0, 1, 1)
    p4[b, 0], p4[b, 1], p4[b, 2] = ((xs[b] - 30 + 0.5) * 0.1).astype(F), ((ys[b] - 2 + 0.5) * 0.1).astype(F), 50.0
    n4[b] = (0, 0, 1, 1)
    p4[c, 0], p4[c, 1], p4[c, 2] = 3.0, ((ys[c] - 2 + 0.5) * 0.1).astype(F), (50.0 - (xs[c] - 60 + 0.5) * 0.1).astype(F)
    n4[c] = (1, 0, 0, 1)
    truth[a, :3] = 1.0
    truth[b, :3] = (1.0 + 0.01 * (xs[b] - 30))[:, None].astype(F)
    truth[c, :3] = 2.0
    return truth, p4, n4, (a, b, c)


def synthetic_case(w, h, seed=0):
    """(mean, position4, normal4) float32 [H, W, 4] of the bit-for-bit tests: from 8 texels of width three charts that touch in the
    atlas (two parallel planes 50 units apart with texels of different size, then a wall; jittered positions, tilted and non-unit
    normals), an isolated valid texel in the corner (w - 1, 0) (fp2 = 0), invalid texels that hold NaN in every image, a seeded random
    mean with +inf in one valid texel and NaN in another.  Narrower images: one chart and the isolated texel; 1 x 1: that texel alone."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    p4, n4 = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    if w >= 8:
        rows = (ys >= 1) & (ys < h - 1)
        xa, xb, xc = int(w * 0.4), int(w * 0.75), w - 3
        a, b, c = rows & (xs >= 1) & (xs < xa), rows & (xs >= xa) & (xs < xb), rows & (xs >= xb) & (xs < xc)
    else:
        a = xs < w - 2
        b = c = np.zeros((h, w), bool)
    jitter = (rng.standard_normal((h, w, 3)) * 0.004).astype(F)
    p4[a, 0], p4[a, 1] = (xs[a] * 0.1).astype(F), (ys[a] * 0.3).astype(F)
    n4[a] = (0, 0, 1, 1)
    p4[b, 0], p4[b, 1], p4[b, 2] = (xs[b] * 0.1).astype(F), (ys[b] * 0.1).astype(F), 50.0
    n4[b, :3] = (np.array([0, 0, 1.5]) + rng.standard_normal((int(b.sum()), 3)) * 0.05).astype(F)      # tilted, not unit
    if c.any():
        x_edge = float(xs[c].min())
        p4[c, 0], p4[c, 1], p4[c, 2] = x_edge * 0.1, (ys[c] * 0.1).astype(F), (50.0 - (xs[c] - x_edge + 0.5) * 0.1).astype(F)
        n4[c] = (2, 0, 0, 1)
    chart = a | b | c
    p4[..., :3] = np.where(chart[..., None], p4[..., :3] + jitter, p4[..., :3])
    p4[0, w - 1], n4[0, w - 1] = (7.0, -3.0, 2.0, 0.0), (0.0, 1.0, 0.0, 1.0)                           # the isolated texel
    chart[0, w - 1] = True
    mean = np.zeros((h, w, 4), F)
    mean[..., :3] = (rng.random((h, w, 3)) * 2.0).astype(F) * np.where(b, F(0.3), F(1.0))[..., None]
    # invalid texels may hold anything
    bad = ~chart & (rng.random((h, w)) < 0.5)
    p4[bad] = np.nan
    mean[bad] = np.nan
    n4[bad & (xs % 2 == 0)] = (np.nan, 0, 1, 0)
    if w * h > 16:
        vy, vx = np.nonzero(a)
        k = len(vy) // 2
        mean[vy[k], vx[k], 1] = np.inf
        mean[vy[k // 2], vx[k // 2], :3] = np.nan
    assert not nb.texel_valid(n4)[~chart].any() and nb.texel_valid(n4)[chart].all()
    return mean, p4, n4
