"""Per-pixel noise (jpt_set_variance, jpt_noise_estimate; csrc/jpt_variance.h) restated in float32 numpy: the second central moment of a
pixel's frames, kept with an update that does not cancel, and its reduction to a histogram, a tile map and one result.  Test
infrastructure, like np_meter: one IEEE binary32 operation per + - * / sqrt in source order."""
import numpy as np

F = np.float32
EMPTY, CONVERGED = 1, 2
DEFAULTS = dict(threshold=0.05, floor=0.01, percentile_permille=950, allowed_permille=0)


def frame_value(radiance, ldr8):
    """a frame's value as wf2_accumulate adds it: the radiance itself (JPT_ACCUM_HDR_F32), or the rgba8 store read back
    (JPT_ACCUM_REF_LDR8; idempotent, so values read from a one-frame render pass through unchanged)"""
    cur = np.asarray(radiance, F)
    if ldr8:
        with np.errstate(all="ignore"):
            clipped = np.fmin(np.fmax(cur, F(0)), F(1))          # minNum / maxNum: a NaN operand is ignored
            cur = (np.floor(clipped * F(255) + F(0.5)).astype(F) / F(255)).astype(F)
    return cur


def moments(frames, ldr8, frame_count=1, prev_sum=None, prev_m2=None):
    """(sum, m2), float32 [H, W, 3] each, after a render of `frames` ([H, W, 3] each) whose first frame has ProgressiveRendering frame
    count `frame_count`; frame_count > 1 continues prev_sum / prev_m2 (their first three channels), 1 ignores them"""
    have_prev = frame_count > 1
    s = np.array(np.asarray(prev_sum, F)[..., :3], F) if have_prev else None
    m2 = np.array(np.asarray(prev_m2, F)[..., :3], F) if have_prev else None
    with np.errstate(all="ignore"):
        for f, radiance in enumerate(frames):
            cur = frame_value(radiance, ldr8)[..., :3]
            k = int(frame_count) + f
            s = (cur + s).astype(F) if have_prev else cur.copy()
            have_prev = True
            if k < 2:
                m2 = np.zeros_like(cur)
                continue
            kf = F(k)
            d = ((kf * cur).astype(F) - s).astype(F)
            w = F(1.0) / F(kf * F(kf - F(1.0)))
            m2 = (m2 + ((d * d).astype(F) * w).astype(F)).astype(F)
    return s, m2


def plane(m2):
    """the device's plane: (M2.r, M2.g, M2.b, 0)"""
    out = np.zeros(m2.shape[:2] + (4,), F)
    out[..., :3] = m2
    return out


def _finite(v):
    return np.abs(v) <= F(3.402823466e38)


def estimate(sum4, m2_4, frame_count, valid=None, threshold=0.05, floor=0.01, percentile_permille=950, allowed_permille=0):
    """(result dict, hist uint32 [256], tiles float32 [ceil(H / 8), ceil(W / 8)]) of planes float32 [H, W, >= 3]"""
    s, m = np.asarray(sum4, F), np.asarray(m2_4, F)
    h, w = s.shape[:2]
    thr, flo = F(threshold), F(floor)
    with np.errstate(all="ignore"):
        nf = F(frame_count)
        q = F(nf * F(nf - F(1.0)))
        mean = (s[..., :3] / nf).astype(F)
        v = (m[..., :3] / q).astype(F)

        def lum(c):
            return ((F(0.2126) * c[..., 0]).astype(F) + (F(0.7152) * c[..., 1]).astype(F)).astype(F) + (F(0.0722) * c[..., 2]).astype(F)
        lm, lv = lum(mean).astype(F), lum(v).astype(F)
        e = (np.sqrt(lv).astype(F) / (lm + flo).astype(F)).astype(F)
        counted = _finite(s[..., :3]).all(-1) & _finite(m[..., :3]).all(-1) & (lm >= F(0))
        if valid is not None:
            counted &= np.asarray(valid, bool)
        bins = np.clip((np.ascontiguousarray(e).view(np.uint32) >> np.uint32(20)).astype(np.int64) - 856, 0, 255)
        above = counted & (e > thr)
        offer = np.where(counted & (e > F(0)), e, F(0)).astype(F)
    hist = np.bincount(bins[counted].ravel(), minlength=256).astype(np.uint32)
    ty, tx = -(-h // 8), -(-w // 8)
    padded = np.zeros((ty * 8, tx * 8), F)
    padded[:h, :w] = offer
    tiles = padded.reshape(ty, 8, tx, 8).max(axis=(1, 3)).astype(F)
    n_counted, n_above = int(counted.sum()), int(above.sum())
    res = dict(error=F(0), max_error=F(0), flags=0, tiles_above=int((tiles > thr).sum()), counted=n_counted, above=n_above)
    if frame_count < 2 or n_counted == 0:
        res["flags"] = EMPTY
        return res, hist, tiles
    target = (n_counted * int(percentile_permille) + 999) // 1000
    b = int(np.argmax(np.cumsum(hist.astype(np.uint64)) >= target))
    res["error"] = np.array([(b + 1 + 856) << 20], np.uint32).view(F)[0]
    res["max_error"] = tiles.max()
    if n_above * 1000 <= n_counted * int(allowed_permille):
        res["flags"] = CONVERGED
    return res, hist, tiles


def same_result(got, want):
    """a message naming the first field of two result dicts that differs (floats by their bits), or None"""
    for k in ("error", "max_error"):
        if np.array([got[k]], F).view(np.uint32)[0] != np.array([want[k]], F).view(np.uint32)[0]:
            return "%s: %r vs %r" % (k, got[k], want[k])
    for k in ("flags", "tiles_above", "counted", "above"):
        if int(got[k]) != int(want[k]):
            return "%s: %r vs %r" % (k, got[k], want[k])
    return None
