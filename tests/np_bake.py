"""Lightmap baking (jpt_set_bake_texels, csrc/jpt_bake.h) restated in float32 numpy: the first ray of a texel's path, the UV2
rasteriser, and a whole frame -- np_camera.trace_frame's loop over np_path with the bake rays substituted.  Test infrastructure, like
np_camera: one IEEE binary32 operation per + - * / sqrt in source order."""
import numpy as np

import np_env
import np_path as npp
import np_restatement as npr

F = np.float32
PI = F(3.141592653589793238462643)


def texel_valid(normal4):
    """dot(n.xyz, n.xyz) > 0, NaN failing: [H, W] bool"""
    with np.errstate(all="ignore"):
        n = np.asarray(normal4, F)
        return (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]) > 0


def bake_rays(position4, normal4, frame):
    """bake_ray for every texel of images [H, W, 4], row-major: (seed after the jitter draw [n, 2], o [n, 3], d [n, 3], valid [n]);
    the rays of invalid texels are zeros"""
    with np.errstate(all="ignore"):
        p4 = np.asarray(position4, F)
        n4 = np.asarray(normal4, F)
        h, w = p4.shape[:2]
        ys, xs = np.mgrid[0:h, 0:w]
        seed = npr.prng_seed(xs.reshape(-1), ys.reshape(-1), int(frame))
        seed, _ = npr.pcg2d(seed)                                                   # the jitter draw, taken and discarded
        copy = seed ^ np.array([0x3c6ef372, 0xa54ff53a], dtype=seed.dtype)[None, :]
        _, xi = npr.pcg2d(copy)
        valid = texel_valid(n4).reshape(-1)
        n = npp._normalize(n4.reshape(-1, 4)[:, :3])
        sign = np.where(n[:, 2] > 0, F(1.0), F(-1.0))
        a = F(-1.0) / (sign + n[:, 2])
        b = n[:, 0] * n[:, 1] * a
        c0 = np.stack([F(1.0) + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], axis=-1)
        c1 = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=-1)
        c2 = n
        sp, cp = npp._sincos((F(2.0) * PI) * xi[:, 0])
        radius = np.sqrt(xi[:, 1])
        z = np.sqrt(F(1.0) - radius * radius)
        local = np.stack([radius * cp, radius * sp, z], axis=-1)
        d = c0 * local[:, 0:1] + c1 * local[:, 1:2] + c2 * local[:, 2:3]
        o = p4.reshape(-1, 4)[:, :3] + n * F(0.001)
        o = np.where(valid[:, None], o, F(0.0)).astype(F)
        d = np.where(valid[:, None], d, F(0.0)).astype(F)
        return seed, o, d, valid


def _edge(ux, uy, vx, vy, px, py):
    return (vx - ux) * (py - uy) - (vy - uy) * (px - ux)


def _box(q, w, h):
    """bake_tri_box: the texels a triangle may claim (x0, y0, x1, y1), or None"""
    if not np.isfinite(q).all():
        return 0, 0, w - 1, h - 1
    lx, hx = min(q[0], q[2], q[4]) - F(1.0), max(q[0], q[2], q[4]) + F(1.0)
    ly, hy = min(q[1], q[3], q[5]) - F(1.0), max(q[1], q[3], q[5]) + F(1.0)
    x0 = (int(lx) if lx < F(w) else w) if lx > 0 else 0
    y0 = (int(ly) if ly < F(h) else h) if ly > 0 else 0
    x1 = (int(hx) if hx > 0 else -1) if hx < F(w) else w - 1
    y1 = (int(hy) if hy > 0 else -1) if hy < F(h) else h - 1
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def rasterize(surface, uv2, t12, w, h, position4=None, normal4=None):
    """jpt_bake_add_surface on the images given (default: all invalid): (position4, normal4) float32 [h, w, 4].  The lowest
    triangle index wins a texel; a texel no triangle covers keeps what it held."""
    with np.errstate(all="ignore"):
        p4 = np.zeros((h, w, 4), F) if position4 is None else np.array(position4, F)
        n4 = np.zeros((h, w, 4), F) if normal4 is None else np.array(normal4, F)
        uv = np.asarray(uv2, F).reshape(-1, 2)
        t = np.asarray(t12, F).reshape(12)
        m = np.zeros(16, F)                      # transform12_to_mat16: column-major, the basis rows become the columns' entries
        for c in range(3):
            m[c * 4 + 0], m[c * 4 + 1], m[c * 4 + 2] = t[0 * 3 + c], t[1 * 3 + c], t[2 * 3 + c]
        m[12], m[13], m[14], m[15] = t[9], t[10], t[11], F(1.0)
        idx = np.asarray(surface.indices).reshape(-1, 3)
        winner = np.full((h, w), -1, np.int64)
        ys, xs = np.mgrid[0:h, 0:w]
        px, py = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
        tris = []
        for k, (ia, ib, ic) in enumerate(idx):
            ax, ay = uv[ia, 0] * F(w), uv[ia, 1] * F(h)
            bx, by = uv[ib, 0] * F(w), uv[ib, 1] * F(h)
            cx, cy = uv[ic, 0] * F(w), uv[ic, 1] * F(h)
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            tris.append((ax, ay, bx, by, cx, cy, area))
            if not np.abs(area) > 0:
                continue
            box = _box(np.array([ax, ay, bx, by, cx, cy], F), w, h)
            if box is None:
                continue
            ea, eb, ec = _edge(bx, by, cx, cy, px, py), _edge(cx, cy, ax, ay, px, py), _edge(ax, ay, bx, by, px, py)
            if area < 0:
                ea, eb, ec = -ea, -eb, -ec
            cover = (ea >= 0) & (eb >= 0) & (ec >= 0) & (xs >= box[0]) & (xs <= box[2]) & (ys >= box[1]) & (ys <= box[3])
            winner = np.where(cover & (winner < 0), k, winner)
        for y, x in np.argwhere(winner >= 0):
            k = int(winner[y, x])
            ax, ay, bx, by, cx, cy, area = tris[k]
            eb, ec = _edge(cx, cy, ax, ay, px[y, x], py[y, x]), _edge(ax, ay, bx, by, px[y, x], py[y, x])
            if area < 0:
                eb, ec = -eb, -ec
            aa = np.abs(area)
            u, v = eb / aa, ec / aa
            w0 = F(1.0) - u - v
            ia, ib, ic = idx[k]
            lp = (surface.vertices[ia] * w0 + surface.vertices[ib] * u) + surface.vertices[ic] * v
            ln = (surface.normals[ia] * w0 + surface.normals[ib] * u) + surface.normals[ic] * v
            pos = npp._mat_point(m, lp)
            nrm = npp._normalize(npp._mat_dir(m, ln))
            if np.isfinite(pos).all() and np.isfinite(nrm).all():
                p4[y, x] = (pos[0], pos[1], pos[2], F(k))
                n4[y, x] = (nrm[0], nrm[1], nrm[2], F(1.0))
            else:
                p4[y, x] = 0
                n4[y, x] = 0
        return p4, n4


def trace_frame(ref, position4, normal4, cam, max_bounces, rgb=None):
    """np_camera.trace_frame's loop with the bake rays of frame cam["frame_index"]: float radiance [H, W, 3] and reversed-Z depth [H, W],
    float32.  Invalid texels are never alive: radiance 0, depth far.  rgb None: the gradient sky; else an environment map in BRDF mode."""
    _dot, _mix = npp._dot, npp._mix
    with np.errstate(all="ignore"):
        height, width = np.asarray(position4).shape[:2]
        seed, o, d, valid = bake_rays(position4, normal4, int(cam["frame_index"]))
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
