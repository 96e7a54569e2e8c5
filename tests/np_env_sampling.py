"""Importance sampling of the environment map (jpt_set_environment_sampling, csrc/jpt_shade.h env_build_row / env_build_marginal /
env_sample / env_pdf / env_nee) restated in vectorised float32 numpy, the same binary32 operations in the same order, and the
whole path of JPT_ENV_SAMPLING_MIS as an extension of np_path's loop (brute-force closest hits, so "blocked" is the brute-force
answer).  Test infrastructure."""
import numpy as np

import np_env
import np_path
import np_restatement as npr

F = np.float32
LUM = (F(0.2126), F(0.7152), F(0.0722))
PI_F, TWO_PI_F, TWO_PI2_F = F("3.14159274"), F("6.28318548"), F("19.7392088")
ONE_MINUS = F("0.99999994")
NEE_HASH = (0x68bc21eb, 0x02e5be93)


def row_sin(i, h):
    s, _ = np_path._sincos(((np.asarray(i).astype(F) + F(0.5)) / F(h)).astype(F) * PI_F)
    return s.astype(F)


def weights(rgb):
    """float32 [H, W]: luminance times sin theta at the row centre"""
    rgb = np.asarray(rgb, dtype=F)
    h = rgb.shape[0]
    lum = (LUM[0] * rgb[..., 0] + LUM[1] * rgb[..., 1]) + LUM[2] * rgb[..., 2]
    return (lum * row_sin(np.arange(h), h)[:, None]).astype(F)


def _normalised_cdf(prefix, total):
    with np.errstate(all="ignore"):
        c = np.where(total > F(0), prefix / total, F(1)).astype(F)
    c[..., -1] = F(1)
    return c


def tables(rgb):
    """(cond [H, W], marg [H], total): sequential float32 prefix sums (np.cumsum), normalised, last entries exactly 1"""
    wt = weights(rgb)
    pre = np.cumsum(wt, axis=1, dtype=F)
    rows = pre[:, -1].copy()
    cond = _normalised_cdf(pre, rows[:, None])
    mpre = np.cumsum(rows, dtype=F)
    total = F(mpre[-1])
    marg = _normalised_cdf(mpre, total)
    return cond, marg, total


def _rot(rotation):
    return np.eye(3, dtype=F) if rotation is None else np.asarray(rotation, dtype=F).reshape(3, 3)


def pdf(rgb, tabs, d, rotation=None):
    rgb = np.asarray(rgb, dtype=F)
    h, w = rgb.shape[0], rgb.shape[1]
    _, _, total = tabs
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    if not total > F(0):
        return np.zeros(len(d), dtype=F)
    R = _rot(rotation)
    with np.errstate(all="ignore"):
        m = [R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1] + R[k, 2] * d[:, 2] for k in range(3)]
        sin_t = np.sqrt(m[0] * m[0] + m[2] * m[2]).astype(F)
        phi = np_env.atan2_(m[0], -m[2])
        theta = np_env.atan2_(sin_t, m[1])
        j = np_env._column(np.floor((phi * np_env.INV_2PI + F(0.5)) * F(w)), w)
        i = np_env._row(np.floor(theta * np_env.INV_PI * F(h)), h)
        wt = weights(rgb)[i, j]
        p = (wt / total * (F(w) * F(h)) / (TWO_PI2_F * sin_t)).astype(F)
        return np.where(sin_t > F(0), p, F(0)).astype(F)


def sample(rgb, tabs, xi0, xi1, rotation=None):
    """world directions [n, 3] and their pdf [n]"""
    rgb = np.asarray(rgb, dtype=F)
    h, w = rgb.shape[0], rgb.shape[1]
    cond, marg, total = tabs
    xi0 = np.asarray(xi0, dtype=F).reshape(-1)
    xi1 = np.asarray(xi1, dtype=F).reshape(-1)
    n = len(xi0)
    if not total > F(0):
        return np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F)
    xi0 = np.where(xi0 < ONE_MINUS, xi0, ONE_MINUS).astype(F)
    xi1 = np.where(xi1 < ONE_MINUS, xi1, ONE_MINUS).astype(F)
    i = np.searchsorted(marg, xi1, side="right")
    m0 = np.where(i > 0, marg[np.maximum(i - 1, 0)], F(0)).astype(F)
    m1 = marg[i]
    j = np.array([np.searchsorted(cond[a], b, side="right") for a, b in zip(i, xi0)], dtype=np.int64)
    c0 = np.where(j > 0, cond[i, np.maximum(j - 1, 0)], F(0)).astype(F)
    c1 = cond[i, j]
    with np.errstate(all="ignore"):
        dv = (xi1 - m0) / (m1 - m0)
        du = (xi0 - c0) / (c1 - c0)
        u = (j.astype(F) + du) / F(w)
        v = (i.astype(F) + dv) / F(h)
        st, ct = np_path._sincos((v * PI_F).astype(F))
        sp, cp = np_path._sincos(((u - F(0.5)) * TWO_PI_F).astype(F))
        mx, my, mz = st * sp, ct, -(st * cp)
        R = _rot(rotation)
        d = np.stack([R[0, k] * mx + R[1, k] * my + R[2, k] * mz for k in range(3)], axis=-1).astype(F)
    return d, pdf(rgb, tabs, d, rotation)


def trace_mis(ref, cam, width, height, max_bounces, rgb, rot, intensity):
    """np_path.trace_frame's loop with the environment map and JPT_ENV_SAMPLING_MIS: radiance [H, W, 3] float32"""
    P = np_path
    tabs = tables(rgb)
    with np.errstate(all="ignore"):
        ys, xs = np.mgrid[0:height, 0:width]
        px, py = xs.reshape(-1), ys.reshape(-1)
        n = len(px)
        seed = npr.prng_seed(px, py, int(cam["frame_index"]))
        seed, r = npr.pcg2d(seed)
        js, jc = P._sincos(F(6.2831853) * (r[:, 1] * F(0.25)))
        sx = (px.astype(F) + jc) / F(width) * F(2.0) - F(1.0)
        sy = (py.astype(F) + js) / F(height) * F(2.0) - F(1.0)
        nx, ny = sx, -sy
        m = cam["ivp"].astype(F)
        wx = m[0] * nx + m[4] * ny + m[8] + m[12]
        wy = m[1] * nx + m[5] * ny + m[9] + m[13]
        wz = m[2] * nx + m[6] * ny + m[10] + m[14]
        ww = m[3] * nx + m[7] * ny + m[11] + m[15]
        world = np.stack([wx / ww, wy / ww, wz / ww], axis=-1)
        cpos = np.array([cam["position"][k] for k in range(3)], dtype=F)
        o = np.broadcast_to(cpos, (n, 3)).astype(F)
        d = P._normalize(world - cpos[None, :])
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = np.ones(n, dtype=bool)
        p_brdf = np.zeros(n, dtype=F)
        for i in range(max_bounces + 1):
            t, tri, blas, lpos, lout, u, v, front = P._closest_hit(ref, o, d)
            hit = t < F(1e9)
            sky = np_env.env_radiance(rgb, d, rot, intensity)
            sky_term = throughput * sky
            if i > 0:
                pe = pdf(rgb, tabs, d, rot)
                wm = np.where(pe > F(0), (p_brdf * p_brdf) / (p_brdf * p_brdf + pe * pe), F(1)).astype(F)
                sky_term = sky_term * wm[:, None]
            s = P._shading(ref, tri, blas, lpos, lout, u, v, front)
            term = np.where(hit[:, None], throughput * s["emission"], sky_term)
            radiance = np.where(alive[:, None], radiance + term, radiance)
            alive = alive & hit
            if i < max_bounces and tabs[2] > F(0):
                hs = (seed ^ np.array(NEE_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
                _, xi = npr.pcg2d(hs)
                l, pe = sample(rgb, tabs, xi[:, 0], xi[:, 1], rot)
                ndl = P._dot(s["normal"], l)
                pb = P._density(s, l)
                w = (pe * pe) / (pe * pe + pb * pb)
                c = ((throughput * (P._brdf(s, l) * ndl[:, None])) * np_env.env_radiance(rgb, l, rot, intensity)) * (w / pe)[:, None]
                emit = alive & (pe > F(0)) & (ndl > F(0)) & (c > F(0)).any(axis=1)
                so = s["position"] + s["normal"] * F(0.001)
                blocked = np.ones(n, dtype=bool)
                if emit.any():
                    blocked[emit] = P._closest_hit(ref, so[emit], l[emit])[0] < F(1e9)
                radiance = np.where((emit & ~blocked)[:, None], radiance + c, radiance)
            new_o = s["position"] + s["normal"] * F(0.001)
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = P._sample_brdf(s, xi)
            dens = P._density(s, new_d)
            lambert_in = P._dot(s["normal"], new_d)
            o = np.where(alive[:, None], new_o, o)
            d = np.where(alive[:, None], new_d, d)
            p_brdf = np.where(alive, dens, p_brdf).astype(F)
            alive = alive & ~(lambert_in <= 0)
            f = (P._brdf(s, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where(alive[:, None], throughput * f, throughput)
        return radiance.reshape(height, width, 3)
