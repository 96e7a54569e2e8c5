"""Importance sampling of the emissive triangles (jpt_set_light_sampling, csrc/jpt_shade.h light_emission / light_sample /
light_cos / light_pdf / light_nee / light_hit_weight, csrc/jpt_kernels_post.hip light_*_kernel) restated in vectorised float32
numpy, the same binary32 operations in the same order, and the whole path of JPT_LIGHT_SAMPLING_MIS -- alone, or with the
environment map and JPT_ENV_SAMPLING_MIS -- as an extension of np_env_sampling.trace_mis (brute-force closest hits, so
"blocked" is the brute-force answer).  Test infrastructure."""
import numpy as np

import np_env
import np_env_sampling as nes
import np_path
import np_restatement as npr

F = np.float32
LUM = nes.LUM
BLOCK = 256
ONE_MINUS = nes.ONE_MINUS
LIGHT_HASH = (0x2c1b3c6d, 0x297a2d39)
SHADOW_SCALE = F("0.9999")


def lum(rgb):
    rgb = np.asarray(rgb, dtype=F)
    return ((LUM[0] * rgb[..., 0] + LUM[1] * rgb[..., 1]) + LUM[2] * rgb[..., 2]).astype(F)


def _material_ids(ref, inst, tri):
    words = np.ascontiguousarray(ref.instances).view(np.uint32).reshape(-1)
    w = np.asarray(inst, np.int64) * 44 + 41 + ref.tri_data["material_index"][np.asarray(tri, np.int64)].astype(np.int64)
    mat = np.where(w < len(words), words[np.minimum(w, len(words) - 1)], 0)
    return np.where(mat >= len(ref.materials), 0, mat)


def emission(ref, inst, tri):
    """Le [n, 3] of (instance, triangle) pairs: get_shading_data's material lookup"""
    em = ref.materials["emission"][_material_ids(ref, inst, tri)].astype(F)
    w = np.where(em[:, 3] > F(0), em[:, 3], F(0)).astype(F)
    return (em[:, :3] * w[:, None]).astype(F)


def emitters(ref):
    """(instance, triangle) pairs [n, 2], instance-major, triangles ascending, lum(Le) > 0"""
    out = []
    for i, inst in enumerate(ref.instances):
        tris = np.unique(np.array(np_path._leaf_triangles(ref.bvh_nodes, inst["blas_index"]), dtype=np.int64))
        if len(tris) == 0:
            continue
        keep = lum(emission(ref, np.full(len(tris), i), tris)) > F(0)
        out += [(i, int(t)) for t in tris[keep]]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _world_edges(ref, inst, tri):
    geom = ref.tri_geom["vertices"][tri].astype(F)
    v0, v1, v2 = geom[:, 0, :3], geom[:, 1, :3], geom[:, 2, :3]
    m = np.moveaxis(ref.instances["transform"][inst].astype(F), -1, 0)
    return np_path._mat_point(m, v0), np_path._mat_dir(m, v1 - v0), np_path._mat_dir(m, v2 - v0)


def _normalised_prefix(x):
    """env_build_marginal: sequential float32 prefix sum, normalised, last entry exactly 1 (all 1s for a zero sum); and the sum"""
    pre = np.cumsum(x, dtype=F)
    total = F(pre[-1])
    with np.errstate(all="ignore"):
        c = np.where(total > F(0), pre / total, F(1)).astype(F)
    c[-1] = F(1)
    return c, total


def tables(ref):
    """dict(pairs, tri [n, 3, 4], cdf [n], marg [blocks + 1], total)"""
    pairs = emitters(ref)
    n = len(pairs)
    if n == 0:
        return dict(pairs=pairs, tri=np.zeros((0, 3, 4), F), cdf=np.zeros(0, F), marg=np.zeros(1, F), total=F(0))
    inst, tri = pairs[:, 0], pairs[:, 1]
    le = emission(ref, inst, tri)
    with np.errstate(all="ignore"):
        p0, e1, e2 = _world_edges(ref, inst, tri)
        g = np_path._cross(e1, e2)
        area = F(0.5) * np.sqrt(np_path._dot(g, g))
        power = lum(le) * area
        power = np.where((power > F(0)) & (power <= F(3.40282347e38)), power, F(0)).astype(F)
    t = np.zeros((n, 3, 4), F)
    t[:, 0, :3], t[:, 1, :3], t[:, 2, :3] = p0, e1, e2
    t[:, 0, 3], t[:, 1, 3], t[:, 2, 3] = le[:, 0], le[:, 1], le[:, 2]
    nb = (n + BLOCK - 1) // BLOCK
    cdf = np.zeros(n, F)
    sums = np.zeros(nb, F)
    for b in range(nb):
        cdf[b * BLOCK:(b + 1) * BLOCK], sums[b] = _normalised_prefix(power[b * BLOCK:(b + 1) * BLOCK])
    marg, total = _normalised_prefix(sums)
    return dict(pairs=pairs, tri=t, cdf=cdf, marg=np.append(marg, total).astype(F), total=total)


def light_cos(e1, e2, l):
    return np.abs(np_path._dot(np_path._normalize(np_path._cross(e1, e2)), l)).astype(F)


def light_pdf(le, total, d2, c):
    return ((lum(le) * d2) / (total * c)).astype(F)


def sample(tabs, xi4):
    """per draw: the point y [n, 3], the emitter's world edges e1, e2 and Le"""
    xi4 = np.asarray(xi4, F).reshape(-1, 4)
    n_e = len(tabs["cdf"])
    nb = len(tabs["marg"]) - 1
    x0 = np.where(xi4[:, 0] < ONE_MINUS, xi4[:, 0], ONE_MINUS).astype(F)
    x1 = np.where(xi4[:, 1] < ONE_MINUS, xi4[:, 1], ONE_MINUS).astype(F)
    b = np.searchsorted(tabs["marg"][:nb], x0, side="right")
    k = np.array([bb * BLOCK + np.searchsorted(tabs["cdf"][bb * BLOCK:min(n_e, (bb + 1) * BLOCK)], x, side="right")
                  for bb, x in zip(b, x1)], dtype=np.int64)
    t = tabs["tri"][k]
    p0, e1, e2 = t[:, 0, :3], t[:, 1, :3], t[:, 2, :3]
    le = np.stack([t[:, 0, 3], t[:, 1, 3], t[:, 2, 3]], axis=-1)
    with np.errstate(all="ignore"):
        s = np.sqrt(xi4[:, 2])
        y = (p0 + e1 * (s * (F(1) - xi4[:, 3]))[:, None]) + e2 * (s * xi4[:, 3])[:, None]
    return y.astype(F), e1, e2, le


def sample_seen_from(tabs, xi4, origins):
    """jpt_debug_light_sample: (y, l, p_L) seen from origins [n, 3]"""
    y, e1, e2, le = sample(tabs, xi4)
    with np.errstate(all="ignore"):
        dv = y - np.asarray(origins, F).reshape(-1, 3)
        d2 = np_path._dot(dv, dv)
        l = np_path._normalize(dv)
        c = light_cos(e1, e2, l)
        p = np.where((c > F(0)) & (tabs["total"] > F(0)), light_pdf(le, tabs["total"], d2, c), F(0)).astype(F)
    return y, l, p


def hit_pdf(ref, tabs, inst, tri, points, origins, dirs):
    """jpt_debug_light_pdf: p_L of hit points on (instance, triangle) seen from origins along dirs (0 unless lum(Le) > 0)"""
    inst, tri = np.asarray(inst, np.int64), np.asarray(tri, np.int64)
    le = emission(ref, inst, tri)
    with np.errstate(all="ignore"):
        _, e1, e2 = _world_edges(ref, inst, tri)
        dv = np.asarray(points, F) - np.asarray(origins, F)
        p = light_pdf(le, tabs["total"], np_path._dot(dv, dv), light_cos(e1, e2, np.asarray(dirs, F)))
    return np.where((lum(le) > F(0)) & (tabs["total"] > F(0)), p, F(0)).astype(F)


def _gradient_sky(d):
    t = F(0.5) * (d[:, 1] + F(1.0))
    m = np_path._mix
    return np.stack([m(F(0.95), F(0.9), t) * F(1.0), m(F(0.95), F(0.94), t) * F(1.0), m(F(0.95), F(1.0), t) * F(1.0)], axis=-1)


def trace_lights(ref, cam, width, height, max_bounces, rgb=None, rot=None, intensity=1.0, env_mis=False, tabs=None):
    """the path of JPT_LIGHT_SAMPLING_MIS: radiance [H, W, 3] float32.  rgb None: the gradient sky; env_mis: the map's NEE too"""
    P = np_path
    tabs = tables(ref) if tabs is None else tabs
    total = tabs["total"]
    etabs = nes.tables(rgb) if (rgb is not None and env_mis) else None
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
            sky = _gradient_sky(d) if rgb is None else np_env.env_radiance(rgb, d, rot, intensity)
            sky_term = throughput * sky
            if i > 0 and etabs is not None:
                pe = nes.pdf(rgb, etabs, d, rot)
                wm = np.where(pe > F(0), (p_brdf * p_brdf) / (p_brdf * p_brdf + pe * pe), F(1)).astype(F)
                sky_term = sky_term * wm[:, None]
            s = P._shading(ref, tri, blas, lpos, lout, u, v, front)
            hit_term = throughput * s["emission"]
            if i > 0:
                le = s["emission"]
                _, e1, e2 = _world_edges(ref, blas, tri)
                dv = s["position"] - o
                pl = light_pdf(le, total, P._dot(dv, dv), light_cos(e1, e2, d))
                wl = ((p_brdf * p_brdf) / (p_brdf * p_brdf + pl * pl)).astype(F)
                wl = np.where(wl == wl, wl, F(1))
                wl = np.where((lum(le) > F(0)) & (total > F(0)), wl, F(1)).astype(F)
                hit_term = np.where(((lum(le) > F(0)) & (total > F(0)))[:, None], hit_term * wl[:, None], hit_term)
            term = np.where(hit[:, None], hit_term, sky_term)
            radiance = np.where(alive[:, None], radiance + term, radiance)
            alive = alive & hit
            so = s["position"] + s["normal"] * F(0.001)
            if i < max_bounces and etabs is not None and etabs[2] > F(0):
                hs = (seed ^ np.array(nes.NEE_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
                _, xi = npr.pcg2d(hs)
                l, pe = nes.sample(rgb, etabs, xi[:, 0], xi[:, 1], rot)
                ndl = P._dot(s["normal"], l)
                pb = P._density(s, l)
                w = (pe * pe) / (pe * pe + pb * pb)
                c = ((throughput * (P._brdf(s, l) * ndl[:, None])) * np_env.env_radiance(rgb, l, rot, intensity)) * (w / pe)[:, None]
                emit = alive & (pe > F(0)) & (ndl > F(0)) & (c > F(0)).any(axis=1)
                blocked = np.ones(n, dtype=bool)
                if emit.any():
                    blocked[emit] = P._closest_hit(ref, so[emit], l[emit])[0] < F(1e9)
                radiance = np.where((emit & ~blocked)[:, None], radiance + c, radiance)
            if i < max_bounces and total > F(0):
                hs = (seed ^ np.array(LIGHT_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
                hs, xa = npr.pcg2d(hs)
                _, xb = npr.pcg2d(hs)
                y, e1, e2, le = sample(tabs, np.concatenate([xa, xb], axis=1))
                dv = y - so
                d2 = P._dot(dv, dv)
                l = P._normalize(dv)
                ndl = P._dot(s["normal"], l)
                c_y = light_cos(e1, e2, l)
                pl = light_pdf(le, total, d2, c_y)
                pb = P._density(s, l)
                w = (pl * pl) / (pl * pl + pb * pb)
                c = ((throughput * (P._brdf(s, l) * ndl[:, None])) * le) * (w / pl)[:, None]
                emit = alive & (ndl > F(0)) & (c_y > F(0)) & np.isfinite(c).all(axis=1) & (c > F(0)).any(axis=1)
                tmax = (np.sqrt(d2) * SHADOW_SCALE).astype(F)
                blocked = np.ones(n, dtype=bool)
                if emit.any():
                    blocked[emit] = P._closest_hit(ref, so[emit], l[emit])[0] < tmax[emit]
                radiance = np.where((emit & ~blocked)[:, None], radiance + c, radiance)
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = P._sample_brdf(s, xi)
            dens = P._density(s, new_d)
            lambert_in = P._dot(s["normal"], new_d)
            o = np.where(alive[:, None], so, o)
            d = np.where(alive[:, None], new_d, d)
            p_brdf = np.where(alive, dens, p_brdf).astype(F)
            alive = alive & ~(lambert_in <= 0)
            f = (P._brdf(s, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where(alive[:, None], throughput * f, throughput)
        return radiance.reshape(height, width, 3)
