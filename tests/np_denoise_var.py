"""jpt_denoise with jpt_set_denoise_variance on, restated in vectorised float32 numpy from its pin ("the
variance-guided a-trous filter"; include/jpt.h), not from the kernels: np_denoise's filter with the colour weight measured against the
variance of the mean, which the passes carry along -- the same binary32 operations in the same order, so the library's host form
(jpt_debug_atrous_variance, device -1) and its kernels must equal this bit for bit.  Test infrastructure."""
import numpy as np

import np_denoise as nd

F = np.float32
H3 = (F(0.25), F(0.5), F(0.25))
DEFAULTS = dict(sigma_variance=2.0, variance_floor=1e-6)


def first(accum, m2, frame_count, albedo):
    """(i_0 float32 [H, W, 3], v_0 float32 [H, W]) of the accumulation (sums) and the plane of jpt_set_variance"""
    nf = F(frame_count)
    q = F(nf * F(nf - F(1.0)))
    am = nd.amod(albedo)
    i0 = ((np.asarray(accum, F)[..., :3] / nf).astype(F) / am).astype(F)
    m = np.asarray(m2, F)[..., :3]
    t = [((m[..., c] / q).astype(F) / (am[..., c] * am[..., c]).astype(F)).astype(F) for c in range(3)]
    v = ((t[0] + t[1]).astype(F) + t[2]).astype(F)
    return i0, np.where(np.isfinite(v) & (v > 0), v, F(0.0)).astype(F)


def prefilter(vk):
    """gv: the 3 x 3 binomial of v_k at spacing 1 over the taps inside the image, divided by the sum of the weights used"""
    num, w = np.zeros_like(vk), np.zeros_like(vk)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq, inside = nd._shift(vk, dx, dy)
            wt = F(H3[dy + 1] * H3[dx + 1])
            num = np.where(inside, num + (wt * vq).astype(F), num).astype(F)
            w = np.where(inside, w + wt, w).astype(F)
    return (num / w).astype(F)


def var_pass(ik, vk, position_t, normal, k, npow, sigma_plane, sigma_variance, variance_floor):
    """(i_k, v_k) -> (i_k+1, v_k+1)"""
    s = 1 << k
    sv2 = F(F(sigma_variance) * F(sigma_variance))
    den = ((sv2 * prefilter(vk)).astype(F) + F(variance_floor)).astype(F)
    xp, tp, n_p = position_t[..., :3], position_t[..., 3], normal[..., :3]
    pm = tp < 0
    acc = np.zeros_like(ik)
    wsum, vs = np.zeros(ik.shape[:2], F), np.zeros(ik.shape[:2], F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, inside = nd._shift(ik, s * dx, s * dy)
            vq, _ = nd._shift(vk, s * dx, s * dy)
            pq, _ = nd._shift(position_t, s * dx, s * dy)
            nq, _ = nd._shift(normal, s * dx, s * dy)
            qm = pq[..., 3] < 0
            wn = nd._pos(n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1] + n_p[..., 2] * nq[..., 2])
            for _ in range(npow):
                wn = wn * wn
            dxyz = pq[..., :3] - xp
            rz = np.abs(n_p[..., 0] * dxyz[..., 0] + n_p[..., 1] * dxyz[..., 1] + n_p[..., 2] * dxyz[..., 2]) / (F(sigma_plane) * tp)
            g = nd._pos(F(1.0) - rz)
            e = np.where(pm & qm, F(1.0), np.where(pm | qm, F(0.0), wn * (g * g))).astype(F)
            dc = cq - ik
            wc = F(1.0) / (F(1.0) + (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2]) / den)
            ew = (e * wc).astype(F)
            if dx == 0 and dy == 0:
                ew = np.ones_like(ew)
            wt = ((nd.H5[dy + 2] * nd.H5[dx + 2]) * ew).astype(F)
            wt = np.where(nd._finite3(cq) & (ew == ew) & inside, wt, F(0.0)).astype(F)
            use = wt != 0
            acc = acc + np.where(use[..., None], cq * wt[..., None], F(0.0)).astype(F)
            vs = vs + np.where(use, (wt * wt).astype(F) * vq, F(0.0)).astype(F)
            wsum = wsum + wt
    keep = ~nd._finite3(ik)
    out = np.where(keep[..., None], ik, acc / wsum[..., None]).astype(F)
    return out, np.where(keep, vk, vs / (wsum * wsum).astype(F)).astype(F)


def denoise(accum, m2, frame_count, position_t, normal, albedo, passes=5, normal_power_log2=6, sigma_plane=0.02, sigma_color=None,
            sigma_variance=2.0, variance_floor=1e-6):
    """the guided jpt_denoise from the accumulation (sums, float32 [H, W, 4]), the plane of jpt_set_variance and the frame count ->
    (the denoised image float32 [H, W, 4] = (rgb, 1), the variance of the last pass float32 [H, W]).  sigma_color is not read."""
    with np.errstate(all="ignore"):
        position_t, normal = np.asarray(position_t, F), np.asarray(normal, F)
        i, v = first(accum, m2, frame_count, albedo)
        for k in range(passes):
            i, v = var_pass(i, v, position_t, normal, k, normal_power_log2, sigma_plane, sigma_variance, variance_floor)
        out = np.ones(i.shape[:2] + (4,), F)
        out[..., :3] = i * nd.amod(albedo)
    return out, v


# ---- synthetic inputs of the filter tests --------------------------------------------------------------------------------------

def synthetic_case(width, height, seed=0, frame_count=4):
    """(accum, m2, position_t, normal, albedo), float32 [H, W, 4] each: np_denoise.synthetic_case's images -- its mean, with the NaN /
    +inf / -inf / 1e30 pixels it plants, times the frame count as the accumulation -- and a seeded plane of second moments with zero,
    negative, NaN, +inf and huge entries planted (images of more than 16 pixels)."""
    mean, position_t, normal, albedo = nd.synthetic_case(width, height, seed)
    rng = np.random.default_rng(seed + 77)
    accum = np.ones((height, width, 4), F)
    with np.errstate(all="ignore"):
        accum[..., :3] = mean[..., :3] * F(frame_count)
    m2 = np.zeros((height, width, 4), F)
    m2[..., :3] = (rng.random((height, width, 3)) ** 2 * 0.5 * frame_count).astype(F)
    if width * height > 16:
        flat = m2.reshape(-1, 4)
        n = len(flat)
        flat[n // 5, :3] = 0.0
        flat[n // 4, 1] = -1.0
        flat[(2 * n) // 5, :3] = -3.0
        flat[(3 * n) // 5, 0] = np.nan
        flat[(4 * n) // 5, 2] = np.inf
        flat[5 % n, :3] = 3e38
        flat[n - 2, :3] = 1e36
        flat[11 % n, 1] = 1e-40
    return accum, m2, position_t, normal, albedo
