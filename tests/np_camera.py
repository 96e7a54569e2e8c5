"""The camera models (jpt_set_camera_model, csrc/jpt_camera.h) restated in float32 numpy: the ray of a raster position under
PROJECTIVE and EQUIRECT, the jittered rays of a frame, the pixel-centre rays of the guides and of picking, and a whole frame --
np_lens.trace_frame's loop with the model's rays substituted.  Test infrastructure, like np_lens: one IEEE binary32 operation per
+ - * / sqrt in source order."""
import numpy as np

import np_env
import np_lens as nl
import np_path as npp
import np_restatement as npr

F = np.float32
PINHOLE, PROJECTIVE, EQUIRECT = 0, 1, 2


def _position(cam):
    return np.array([np.asarray(cam["position"]).reshape(-1)[k] for k in range(3)], dtype=F)


def jitter(cam, width, height, px=None, py=None):
    """primary_ray's seed and jitter draw for pixels (px, py) (default: every pixel, row-major): (seed after the draw [n, 2], fx, fy)
    with (fx, fy) = (px + jc, py + js), the jittered raster position"""
    if px is None:
        ys, xs = np.mgrid[0:height, 0:width]
        px, py = xs.reshape(-1), ys.reshape(-1)
    seed = npr.prng_seed(px, py, int(cam["frame_index"]))
    seed, r = npr.pcg2d(seed)
    js, jc = npp._sincos(F(6.2831853) * (r[:, 1] * F(0.25)))
    return seed, px.astype(F) + jc, py.astype(F) + js


def raster_rays(cam, width, height, model, fx, fy):
    """camera_raster_ray: (o [n, 3], d [n, 3]) of the raster positions (fx, fy) [n] float32, in pixels, under PROJECTIVE or EQUIRECT"""
    with np.errstate(all="ignore"):
        fx, fy = np.asarray(fx, F), np.asarray(fy, F)
        m = cam["ivp"].astype(F).reshape(16)
        if model == EQUIRECT:
            f, r, u_ = nl.basis(cam)
            u, v = fx / F(width), fy / F(height)
            phi, theta = (u - F(0.5)) * F(6.2831853), v * F(3.14159265)
            st, ct = npp._sincos(theta)
            sp, cp = npp._sincos(phi)
            mx, my, mz = st * sp, ct, st * cp
            o = np.broadcast_to(_position(cam), (len(fx), 3)).astype(F)
            d = npp._normalize((r[None, :] * mx[:, None] + u_[None, :] * my[:, None]) + f[None, :] * mz[:, None])
            return o, d.astype(F)
        assert model == PROJECTIVE
        scx = fx / F(width) * F(2.0) - F(1.0)
        scy = fy / F(height) * F(2.0) - F(1.0)
        nx, ny = scx, -scy
        w1 = m[3] * nx + m[7] * ny + m[11] + m[15]
        p1 = np.stack([(m[0] * nx + m[4] * ny + m[8] + m[12]) / w1, (m[1] * nx + m[5] * ny + m[9] + m[13]) / w1,
                       (m[2] * nx + m[6] * ny + m[10] + m[14]) / w1], axis=-1)
        w0 = m[3] * nx + m[7] * ny - m[11] + m[15]
        p0 = np.stack([(m[0] * nx + m[4] * ny - m[8] + m[12]) / w0, (m[1] * nx + m[5] * ny - m[9] + m[13]) / w0,
                       (m[2] * nx + m[6] * ny - m[10] + m[14]) / w0], axis=-1)
        return p0.astype(F), npp._normalize(p1 - p0).astype(F)


def camera_rays(cam, width, height, model):
    """the rays of one frame (cam["frame_index"]) of a render under `model`: (seed, o, d), pixels row-major; PINHOLE: np_lens's"""
    if model == PINHOLE:
        return nl.pinhole_rays(cam, width, height)
    with np.errstate(all="ignore"):
        seed, fx, fy = jitter(cam, width, height)
        o, d = raster_rays(cam, width, height, model, fx, fy)
        return seed, o, d


def centre_rays(cam, width, height, model):
    """the un-jittered rays through the pixel centres (the guides of jpt_denoise): (o, d), row-major; PINHOLE: np_denoise's"""
    if model == PINHOLE:
        import np_denoise
        return np_denoise.centre_rays(cam, width, height)
    ys, xs = np.mgrid[0:height, 0:width]
    return raster_rays(cam, width, height, model, xs.reshape(-1).astype(F) + F(0.5), ys.reshape(-1).astype(F) + F(0.5))


def trace_frame(ref, cam, width, height, max_bounces, model, rgb=None):
    """np_lens.trace_frame's loop with the model's rays: float radiance [H, W, 3] and reversed-Z depth [H, W], float32.  rgb None: the
    gradient sky; else an environment map in BRDF mode, np_env.env_radiance at the misses."""
    _dot, _mix = npp._dot, npp._mix
    with np.errstate(all="ignore"):
        seed, o, d = camera_rays(cam, width, height, model)
        n = len(o)
        far, near = F(cam["far"]), F(cam["near"])
        depth = np.full(n, far, dtype=F)
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = np.ones(n, dtype=bool)
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
        return radiance.reshape(height, width, 3), depth.reshape(height, width)
