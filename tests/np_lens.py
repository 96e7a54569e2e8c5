"""The thin-lens camera (jpt_set_lens, csrc/jpt_lens.h) restated in float32 numpy: the basis, the per-path step and a whole frame --
np_path.trace_frame's loop with the lens rays substituted.  Test infrastructure, like np_path: one IEEE binary32 operation per
+ - * / sqrt in source order."""
import numpy as np

import np_path as npp
import np_restatement as npr

F = np.float32
HASH_X, HASH_Y = 0x85ebca6b, 0xc2b2ae35


def _unproject(m, nx, ny):
    """ivp * (nx, ny, 1, 1) / w: primary_ray's four sums and three divisions"""
    nx, ny = F(nx), F(ny)
    wx = m[0] * nx + m[4] * ny + m[8] + m[12]
    wy = m[1] * nx + m[5] * ny + m[9] + m[13]
    wz = m[2] * nx + m[6] * ny + m[10] + m[14]
    ww = m[3] * nx + m[7] * ny + m[11] + m[15]
    return np.array([wx / ww, wy / ww, wz / ww], dtype=F)


def basis(cam):
    """(f, r, u) of a camera block (scenes.camera_block record), float32 [3] each"""
    with np.errstate(all="ignore"):
        m = cam["ivp"].astype(F).reshape(16)
        pos = np.array([cam["position"][k] for k in range(3)], dtype=F)
        c0 = _unproject(m, 0.0, 0.0)
        f = npp._normalize(c0 - pos)
        c1 = _unproject(m, 1.0, 0.0)
        r0 = c1 - c0
        r = npp._normalize(r0 - f * npp._dot(r0, f))
        u = npp._cross(r, f)
        return f.astype(F), r.astype(F), u.astype(F)


def lens_offsets(radius, xi):
    """(lu, lv) of n (xi0, xi1) pairs"""
    rad = F(radius) * np.sqrt(xi[:, 0])
    s, c = npp._sincos(F(6.2831853) * xi[:, 1])
    return rad * c, rad * s


def lens_apply(bas, radius, focus, o, d, xi):
    """the step from (xi0, xi1) on, for n pinhole rays (o, d): the rays the lens sends out"""
    with np.errstate(all="ignore"):
        f, r, u = bas
        lu, lv = lens_offsets(radius, xi)
        cf = npp._dot(d, f[None, :])
        keep = ~(cf > 0)
        tf = F(focus) / cf
        p = o + d * tf[:, None]
        o2 = (o + r[None, :] * lu[:, None]) + u[None, :] * lv[:, None]
        d2 = npp._normalize(p - o2)
        return np.where(keep[:, None], o, o2).astype(F), np.where(keep[:, None], d, d2).astype(F)


def lens_xi(seed):
    """the lens randoms of paths whose seeds after the jitter draw are `seed` [n, 2] uint32: one pcg2d round of a hashed copy"""
    h = seed.astype(np.uint32) ^ np.array([HASH_X, HASH_Y], dtype=np.uint32)[None, :]
    _, xi = npr.pcg2d(h)
    return xi


def pinhole_rays(cam, width, height):
    """np_path.trace_frame's ray set-up: (seed after the jitter draw [n, 2], o [n, 3], d [n, 3]), pixels row-major"""
    with np.errstate(all="ignore"):
        ys, xs = np.mgrid[0:height, 0:width]
        px, py = xs.reshape(-1), ys.reshape(-1)
        n = len(px)
        seed = npr.prng_seed(px, py, int(cam["frame_index"]))
        seed, r = npr.pcg2d(seed)
        js, jc = npp._sincos(F(6.2831853) * (r[:, 1] * F(0.25)))
        sx = (px.astype(F) + jc) / F(width) * F(2.0) - F(1.0)
        sy = (py.astype(F) + js) / F(height) * F(2.0) - F(1.0)
        nx, ny = sx, -sy
        m = cam["ivp"].astype(F).reshape(16)
        wx = m[0] * nx + m[4] * ny + m[8] + m[12]
        wy = m[1] * nx + m[5] * ny + m[9] + m[13]
        wz = m[2] * nx + m[6] * ny + m[10] + m[14]
        ww = m[3] * nx + m[7] * ny + m[11] + m[15]
        world = np.stack([wx / ww, wy / ww, wz / ww], axis=-1)
        cpos = np.array([cam["position"][k] for k in range(3)], dtype=F)
        o = np.broadcast_to(cpos, (n, 3)).astype(F)
        d = npp._normalize(world - cpos[None, :])
        return seed, o, d.astype(F)


def lens_rays(cam, width, height, radius, focus):
    """the rays of one frame of a lens render: (seed, o, d); radius 0: the pinhole's"""
    seed, o, d = pinhole_rays(cam, width, height)
    if float(radius) > 0.0:
        o, d = lens_apply(basis(cam), radius, focus, o, d, lens_xi(seed))
    return seed, o, d


def trace_frame(ref, cam, width, height, max_bounces, radius, focus):
    """np_path.trace_frame (sky lighting) with the lens rays: float radiance [H, W, 3] and reversed-Z depth [H, W], float32"""
    _dot, _mix = npp._dot, npp._mix
    with np.errstate(all="ignore"):
        seed, o, d = lens_rays(cam, width, height, radius, focus)
        n = len(o)
        far, near = F(cam["far"]), F(cam["near"])
        depth = np.full(n, far, dtype=F)
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = np.ones(n, dtype=bool)
        for i in range(max_bounces + 1):
            t, tri, blas, lpos, lout, u, v, front = npp._closest_hit(ref, o, d)
            hit = t < F(1e9)
            tsky = F(0.5) * (d[:, 1] + F(1.0))
            sky = np.stack([_mix(F(0.95), F(0.9), tsky) * F(1.0), _mix(F(0.95), F(0.94), tsky) * F(1.0), _mix(F(0.95), F(1.0), tsky) * F(1.0)], axis=-1)
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
        return radiance.reshape(height, width, 3), depth.reshape(height, width)
