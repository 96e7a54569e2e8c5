"""Light probes (jpt_set_probes, jpt_probe_project, csrc/jpt_probe.h) restated in numpy: the first ray of a tile cell's path and the
pinned sum of the projection in float32 -- one IEEE binary32 operation per + - * / sqrt in source order --, the
quadrature table in float64 from the same closed forms, and a whole frame: np_bake.trace_frame's loop over np_path with the probe rays
substituted.  Test infrastructure, like np_bake."""
import numpy as np

import np_env
import np_path as npp
import np_restatement as npr

F = np.float32
HASH = (0x510e527f, 0x9b05688c)
K0, K1, K2, K3, K4 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
BAND_FACTOR = np.array([np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0])[BAND]


def image_size(n, tw, th, per_row):
    return per_row * tw, -(-n // per_row) * th


def pixel_cells(n, tw, th, per_row):
    """for every pixel of the image, raster order: (probe, i, j, valid)"""
    w, h = image_size(n, tw, th, per_row)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    p = (ys // th) * per_row + xs // tw
    return p, xs % tw, ys % th, p < n


def probe_rays(positions, tw, th, per_row, frame):
    """probe_ray for every pixel of the image the probes make, row-major: (seed after the jitter draw [n, 2], o [n, 3], d [n, 3],
    valid [n]); the rays of tiles without a probe are zeros"""
    with np.errstate(all="ignore"):
        pos = np.asarray(positions, F).reshape(-1, 3)
        w, h = image_size(len(pos), tw, th, per_row)
        ys, xs = np.mgrid[0:h, 0:w]
        seed = npr.prng_seed(xs.reshape(-1), ys.reshape(-1), int(frame))
        seed, _ = npr.pcg2d(seed)                                                   # the jitter draw, taken and discarded
        copy = seed ^ np.array(HASH, dtype=seed.dtype)[None, :]
        _, xi = npr.pcg2d(copy)
        p, i, j, valid = pixel_cells(len(pos), tw, th, per_row)
        u = (i.astype(F) + xi[:, 0]) / F(tw)
        v = (j.astype(F) + xi[:, 1]) / F(th)
        phi = (u - F(0.5)) * F(6.2831853)
        z = F(1.0) - F(2.0) * v
        r = np.sqrt(F(1.0) - z * z)
        sp, cp = npp._sincos(phi)
        d = np.stack([r * sp, z, r * cp], axis=-1)
        o = pos[np.minimum(p, len(pos) - 1)]
        o = np.where(valid[:, None], o, F(0.0)).astype(F)
        d = np.where(valid[:, None], d, F(0.0)).astype(F)
        return seed, o, d, valid


def basis(d):
    """the nine basis functions at directions d [..., 3] (float64), in the frame of the map: (X, Y, Z) = (d.z, d.x, d.y)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([K0 + 0 * x, K1 * x, K1 * y, K1 * z, K2 * z * x, K2 * x * y, K3 * (3 * y * y - 1), K2 * z * y, K4 * (z * z - x * x)], axis=-1)


def directions(tw, th, sub):
    """float64 directions of the map at the sub x sub midpoints of every cell: [th * sub, tw * sub, 3]"""
    u = (np.arange(tw * sub) + 0.5) / (tw * sub)
    v = (np.arange(th * sub) + 0.5) / (th * sub)
    z = 1 - 2 * v
    r = np.sqrt(1 - z * z)
    phi = (u - 0.5) * 2 * np.pi
    return np.stack([np.outer(r, np.sin(phi)), np.outer(z, np.ones_like(phi)), np.outer(r, np.cos(phi))], axis=-1)


def cell_means(tw, th):
    """the mean of each basis function over each cell, float64 [th, tw, 9], from the closed forms"""
    jj, ii = np.arange(th, dtype=np.float64), np.arange(tw, dtype=np.float64)
    z0, z1 = 1.0 - 2.0 * jj / th, 1.0 - 2.0 * (jj + 1) / th
    dz = z0 - z1

    def fr(z):
        q = 1.0 - z * z
        return 0.5 * (z * np.sqrt(np.maximum(q, 0.0)) + np.arcsin(np.clip(z, -1.0, 1.0)))

    def fzr(z):
        q = np.maximum(1.0 - z * z, 0.0)
        return -(q * np.sqrt(q)) / 3.0
    mz = (z0 * z0 / 2.0 - z1 * z1 / 2.0) / dz
    mz2 = (z0 * z0 * z0 / 3.0 - z1 * z1 * z1 / 3.0) / dz
    mr = (fr(z0) - fr(z1)) / dz
    mzr = (fzr(z0) - fzr(z1)) / dz
    mr2 = 1.0 - mz2
    p0, p1 = (ii / tw - 0.5) * 2.0 * np.pi, ((ii + 1) / tw - 0.5) * 2.0 * np.pi
    dp = p1 - p0
    ms = (-np.cos(p1) - -np.cos(p0)) / dp
    mc = (np.sin(p1) - np.sin(p0)) / dp
    ms2 = (-np.cos(2.0 * p1) / 2.0 - -np.cos(2.0 * p0) / 2.0) / dp
    mc2 = (np.sin(2.0 * p1) / 2.0 - np.sin(2.0 * p0) / 2.0) / dp
    one_w = np.ones(tw)
    y = np.empty((th, tw, 9))
    y[..., 0] = K0
    y[..., 1] = K1 * np.outer(mr, ms)
    y[..., 2] = K1 * np.outer(mz, one_w)
    y[..., 3] = K1 * np.outer(mr, mc)
    y[..., 4] = K2 * np.outer(mr2, ms2 * 0.5)
    y[..., 5] = K2 * np.outer(mzr, ms)
    y[..., 6] = K3 * np.outer(3.0 * mz2 - 1.0, one_w)
    y[..., 7] = K2 * np.outer(mzr, mc)
    y[..., 8] = K4 * np.outer(mr2, mc2)
    return y


def table64(tw, th, flags=0):
    """the quadrature table in float64, [th, tw, 9]: cell means (closed forms) times the solid angle over the Gram diagonal, times
    the band factor with JPT_PROBE_IRRADIANCE (flags 1); a column whose Gram diagonal vanishes (kProbeGramMin: a function the grid
    cannot resolve -- Y6 with two rows, Y8 with four columns) is zero"""
    y = cell_means(tw, th)
    w = 4.0 * np.pi / (tw * th)
    gram = (w * y * y).reshape(-1, 9).sum(axis=0)
    with np.errstate(all="ignore"):
        t = np.where(gram < 1e-9, 0.0, w * y / gram)
    if flags & 1:
        t = t * BAND_FACTOR
    return t


def project(accum4, frame_count, n, tw, th, per_row, table):
    """jpt_probe_project's pinned sum over an accumulation image [H, W, 4] with `table` (float32 [th, tw, 9], the library's): float32
    [n, 9, 4].  Lane l adds its cells l, l + 64, ... in raster order, mean * t then an add; six indexed adds make the butterfly."""
    with np.errstate(all="ignore"):
        a = np.asarray(accum4, F)
        t = np.asarray(table, F).reshape(tw * th, 9)
        fc = F(frame_count)
        cells = tw * th
        lanes = np.arange(64)
        out = np.zeros((n, 9, 4), F)
        for p in range(n):
            x0, y0 = (p % per_row) * tw, (p // per_row) * th
            mean = (a[y0:y0 + th, x0:x0 + tw, :3] / fc).astype(F).reshape(cells, 3)
            acc = np.zeros((64, 9, 3), F)
            for base in range(0, cells, 64):
                c = base + lanes
                live = c < cells
                cc = np.minimum(c, cells - 1)
                term = (mean[cc][:, None, :] * t[cc][:, :, None]).astype(F)
                acc = np.where(live[:, None, None], (acc + term).astype(F), acc)
            for s in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[lanes ^ s]).astype(F)
            assert (acc.view(np.uint32) == acc[0].view(np.uint32)).all() or np.isnan(acc).any()
            out[p, :, :3] = acc[0]
        return out


def trace_frame(ref, positions, tw, th, per_row, cam, max_bounces, rgb=None):
    """np_bake.trace_frame's loop with the probe rays of frame cam["frame_index"]: float radiance [H, W, 3] and reversed-Z depth [H, W],
    float32.  Tiles without a probe are never alive: radiance 0, depth far.  rgb None: the gradient sky; else an environment map in
    BRDF mode."""
    _dot, _mix = npp._dot, npp._mix
    with np.errstate(all="ignore"):
        width, height = image_size(len(np.asarray(positions).reshape(-1, 3)), tw, th, per_row)
        seed, o, d, valid = probe_rays(positions, tw, th, per_row, int(cam["frame_index"]))
        n = len(o)
        far, near = F(cam["far"]), F(cam["near"])
        depth = np.full(n, far, dtype=F)
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = valid.copy()
        for i in range(max_bounces + 1):
            t, tri, blas, lpos, lout, u, v, front = npp._closest_hit(ref, o, d)
            hit = t < F(1e9)
            if rgb is None:
                tsky = F(0.5) * (d[:, 1] + F(1.0))
                sky = np.stack([_mix(F(0.95), F(0.9), tsky) * F(1.0), _mix(F(0.95), F(0.94), tsky) * F(1.0), _mix(F(0.95), F(1.0), tsky) * F(1.0)], axis=-1)
            else:
                sky = np_env.env_radiance(rgb, d)
            s = npp._shading(ref, tri, blas, lpos, lout, u, v, front)
            emission = np.where(hit[:, None], s["emission"], sky)
            radiance = np.where(alive[:, None], radiance + throughput * emission, radiance)
            alive = alive & hit
            if i == 0:
                diff = s["position"] - o
                depth = np.where(alive, np.sqrt(_dot(diff, diff)), depth)
            new_o = s["position"] + s["normal"] * F(0.001)
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = npp._sample_brdf(s, xi)
            dens = npp._density(s, new_d)
            lambert_in = _dot(s["normal"], new_d)
            o = np.where(alive[:, None], new_o, o)
            d = np.where(alive[:, None], new_d, d)
            alive = alive & ~(lambert_in <= 0)
            f = (npp._brdf(s, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where(alive[:, None], throughput * f, throughput)
        depth = far / (far - near) * (F(1.0) - near / depth)
        return radiance.reshape(height, width, 3).astype(F), depth.reshape(height, width).astype(F)
