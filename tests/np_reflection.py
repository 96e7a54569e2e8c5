"""Reflection probes (jpt_set_reflection_probes, jpt_reflection_prefilter; csrc/jpt_cube.h, csrc/jpt_reflection.h) restated in numpy: the
first ray of a face texel's path, the source chain and the prefilter's pinned sum in float32 -- one IEEE binary32 operation per + - * /
sqrt in source order --, the sample table in float64 from the same formulas, and a whole frame: np_probe.trace_frame's
loop over np_path with the cube rays substituted.  Test infrastructure, like np_probe."""
import numpy as np

import np_env
import np_path as npp
import np_restatement as npr

F = np.float32
HASH = (0x1f83d9ab, 0x5be0cd19)


def log2i(s):
    return int(s).bit_length() - 1


def image_size(n, s, per_row):
    return per_row * 6 * s, -(-n // per_row) * s


def pixel_cells(n, s, per_row):
    """for every pixel of the image, raster order: (probe, face, i, j, valid)"""
    w, h = image_size(n, s, per_row)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    p = (ys // s) * per_row + xs // (6 * s)
    return p, (xs // s) % 6, xs % s, ys % s, p < n


def face_direction(f, a, b):
    """the OpenGL cube-map face table: the direction of (a, b) on face f before normalize3, float32 [..., 3]"""
    one = np.ones_like(a)
    table = [(one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one)]
    out = np.zeros(np.shape(a) + (3,), F)
    for k, v in enumerate(table):
        out = np.where((f == k)[..., None], np.stack(v, axis=-1), out)
    return out.astype(F)


def cube_rays(positions, s, per_row, frame):
    """cube_ray for every pixel of the image the probes make, row-major: (seed after the jitter draw [n, 2], o [n, 3], d [n, 3],
    valid [n]); the rays of strips without a probe are zeros"""
    with np.errstate(all="ignore"):
        pos = np.asarray(positions, F).reshape(-1, 3)
        w, h = image_size(len(pos), s, per_row)
        ys, xs = np.mgrid[0:h, 0:w]
        seed = npr.prng_seed(xs.reshape(-1), ys.reshape(-1), int(frame))
        seed, _ = npr.pcg2d(seed)                                                   # the jitter draw, taken and discarded
        copy = seed ^ np.array(HASH, dtype=seed.dtype)[None, :]
        _, xi = npr.pcg2d(copy)
        p, f, i, j, valid = pixel_cells(len(pos), s, per_row)
        a = F(2.0) * ((i.astype(F) + xi[:, 0]) / F(s)) - F(1.0)
        b = F(2.0) * ((j.astype(F) + xi[:, 1]) / F(s)) - F(1.0)
        d = npp._normalize(face_direction(f, a, b))
        o = pos[np.minimum(p, len(pos) - 1)]
        o = np.where(valid[:, None], o, F(0.0)).astype(F)
        d = np.where(valid[:, None], d, F(0.0)).astype(F)
        return seed, o, d, valid


def lookup(d, size):
    """direction d [..., 3] float32 -> (face, s, t) of a level of `size` texels a side: the nearest texel"""
    with np.errstate(all="ignore"):
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        mx = (ax >= ay) & (ax >= az)
        my = ~mx & (ay >= az)
        face = np.where(mx, np.where(x < 0, 1, 0), np.where(my, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
        sc = np.where(mx, np.where(x < 0, z, -z), np.where(my, x, np.where(z < 0, -x, x))).astype(F)
        tc = np.where(mx, -y, np.where(my, np.where(y < 0, -z, z), -y)).astype(F)
        ma = np.where(mx, ax, np.where(my, ay, az)).astype(F)
        s01 = (sc / ma + F(1.0)) * F(0.5)
        t01 = (tc / ma + F(1.0)) * F(0.5)
        si = np.minimum((s01 * F(size)).astype(np.int32), size - 1)
        ti = np.minimum((t01 * F(size)).astype(np.int32), size - 1)
        return face, si, ti


def texel_normals(size):
    """N of every output texel of a level: float32 [6, size, size, 3], indexed (f, j, i)"""
    f, j, i = np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing="ij")
    a = (F(2.0) * (i.astype(F) + F(0.5))) / F(size) - F(1.0)
    b = (F(2.0) * (j.astype(F) + F(0.5))) / F(size) - F(1.0)
    return npp._normalize(face_direction(f, a, b))


def frame(n):
    """the branch-free tangent frame of Duff et al. in the header's operation order: (T, B) float32 [..., 3]"""
    with np.errstate(all="ignore"):
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        sg = np.copysign(F(1.0), nz).astype(F)
        q = F(-1.0) / (sg + nz)
        c = (nx * ny) * q
        sx = sg * nx
        t = np.stack([F(1.0) + (sx * nx) * q, sg * c, -sx], axis=-1)
        b = np.stack([c, sg + (ny * ny) * q, -ny], axis=-1)
        return t.astype(F), b.astype(F)


def source_chain(accum4, frame_count, n, s, per_row):
    """the source chain: a list over levels 0 .. log2 s of float32 [n, 6, s_m, s_m, 3]"""
    with np.errstate(all="ignore"):
        a = np.asarray(accum4, F)
        fc = F(frame_count)
        lvl0 = np.zeros((n, 6, s, s, 3), F)
        for p in range(n):
            x0, y0 = (p % per_row) * 6 * s, (p // per_row) * s
            strip = (a[y0:y0 + s, x0:x0 + 6 * s, :3] / fc).astype(F)
            lvl0[p] = strip.reshape(s, 6, s, 3).transpose(1, 0, 2, 3)
        chain = [lvl0]
        while chain[-1].shape[2] > 1:
            c = chain[-1]
            aa, bb, cc, dd = c[:, :, 0::2, 0::2], c[:, :, 0::2, 1::2], c[:, :, 1::2, 0::2], c[:, :, 1::2, 1::2]
            chain.append((((aa + bb) + (cc + dd)) * F(0.25)).astype(F))
        return chain


def prefilter(accum4, frame_count, n, s, per_row, n_levels, level, table, src_levels):
    """output level `level` of jpt_reflection_prefilter with the level's kept entries `table` [kept, 4] and `src_levels` [kept] (the
    library's): float32 [n, 6, s_l, s_l, 4]"""
    with np.errstate(all="ignore"):
        chain = source_chain(accum4, frame_count, n, s, per_row)
        sl = s >> level
        out = np.ones((n, 6, sl, sl, 4), F)
        if level == 0:
            out[..., :3] = chain[0]
            return out
        nrm = texel_normals(sl)
        t, b = frame(nrm)
        acc = np.zeros((n, 6, sl, sl, 3), F)
        tab = np.asarray(table, F)
        for k in range(len(tab)):
            lx, ly, lz, w = tab[k]
            d = ((t * lx + b * ly) + nrm * lz).astype(F)
            m = int(src_levels[k])
            face, si, ti = lookup(d, s >> m)
            c = chain[m][:, face, ti, si]                   # [n, 6, sl, sl, 3]
            acc = (acc + (c * w).astype(F)).astype(F)
        out[..., :3] = acc
        return out


def sample_table64(s, n_levels, K, level):
    """the sample table of output level `level` in float64: (L [K, 3], weights [K], the un-floored level expression [K], kept [K] bool);
    weights are L_z / sum over the kept"""
    k = np.arange(K)
    alpha = level / (n_levels - 1.0)
    a2 = alpha * alpha
    u1 = (k + 0.5) / K
    u2 = np.zeros(K)
    for bit in range(8):
        u2 += ((k >> bit) & 1) * 0.5 ** (bit + 1)
    ct = np.sqrt((1.0 - u1) / (1.0 + (a2 - 1.0) * u1))
    st = np.sqrt(1.0 - ct * ct)
    phi = 2.0 * np.pi * u2
    h = np.stack([st * np.cos(phi), st * np.sin(phi), ct], axis=-1)
    L = np.stack([2.0 * h[:, 2] * h[:, 0], 2.0 * h[:, 2] * h[:, 1], 2.0 * h[:, 2] * h[:, 2] - 1.0], axis=-1)
    kept = L[:, 2] > 0.0
    w = L[:, 2] / L[kept, 2].sum()
    den = h[:, 2] * h[:, 2] * (a2 - 1.0) + 1.0
    ndf = a2 / (np.pi * den * den)
    omega_s = 4.0 / (K * ndf)
    omega_0 = 4.0 * np.pi / (6.0 * s * s)
    expr = 0.5 * np.log2(omega_s / omega_0) + 0.5
    return L, w, expr, kept


def texel_solid_angles(size):
    """the solid angle of every texel of a face of `size` texels a side, float64 [size, size]: differences of the corner function
    atan2(a b, sqrt(a^2 + b^2 + 1))"""
    e = 2.0 * np.arange(size + 1) / size - 1.0
    aa, bb = np.meshgrid(e, e, indexing="xy")
    g = np.arctan2(aa * bb, np.sqrt(aa * aa + bb * bb + 1.0))
    return g[1:, 1:] - g[1:, :-1] - g[:-1, 1:] + g[:-1, :-1]


def trace_frame(ref, positions, s, per_row, cam, max_bounces, rgb=None):
    """np_probe.trace_frame's loop with the cube rays of frame cam["frame_index"]: float radiance [H, W, 3] and reversed-Z depth [H, W],
    float32.  Strips without a probe are never alive: radiance 0, depth far.  rgb None: the gradient sky; else an environment map in
    BRDF mode."""
    _dot, _mix = npp._dot, npp._mix
    with np.errstate(all="ignore"):
        width, height = image_size(len(np.asarray(positions).reshape(-1, 3)), s, per_row)
        seed, o, d, valid = cube_rays(positions, s, per_row, int(cam["frame_index"]))
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
            sh = npp._shading(ref, tri, blas, lpos, lout, u, v, front)
            emission = np.where(hit[:, None], sh["emission"], sky)
            radiance = np.where(alive[:, None], radiance + throughput * emission, radiance)
            alive = alive & hit
            if i == 0:
                diff = sh["position"] - o
                depth = np.where(alive, np.sqrt(_dot(diff, diff)), depth)
            new_o = sh["position"] + sh["normal"] * F(0.001)
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = npp._sample_brdf(sh, xi)
            dens = npp._density(sh, new_d)
            lambert_in = _dot(sh["normal"], new_d)
            o = np.where(alive[:, None], new_o, o)
            d = np.where(alive[:, None], new_d, d)
            alive = alive & ~(lambert_in <= 0)
            fthr = (npp._brdf(sh, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where(alive[:, None], throughput * fthr, throughput)
        depth = far / (far - near) * (F(1.0) - near / depth)
        return radiance.reshape(height, width, 3).astype(F), depth.reshape(height, width).astype(F)
