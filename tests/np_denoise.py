"""jpt_denoise restated in vectorised float32 numpy from its pin ("the a-trous filter"; include/jpt.h), not
from the kernels: the guide images from np_path's brute-force closest hit and shading record with the un-jittered ray through
the pixel centre, and the edge-avoiding a-trous filter -- the same binary32 operations in the same order, so the library's host
form (jpt_debug_atrous, device -1) and its kernels must equal this bit for bit.  Test infrastructure.  No textures (np_path)."""
import numpy as np

import np_path as npp

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
ALBEDO_FLOOR = F(0.015625)
DEFAULTS = dict(passes=5, normal_power_log2=6, sigma_plane=0.02, sigma_color=4.0)


# ---- guides -----------------------------------------------------------------------------------------------------------------

def centre_rays(cam, width, height):
    """raster_direction(cam, W, H, x + 0.5, y + 0.5) from the camera position, every pixel, row-major"""
    ys, xs = np.mgrid[0:height, 0:width]
    fx, fy = xs.reshape(-1).astype(F) + F(0.5), ys.reshape(-1).astype(F) + F(0.5)
    sx = fx / F(width) * F(2.0) - F(1.0)
    sy = fy / F(height) * F(2.0) - F(1.0)
    nx, ny = sx, -sy
    m = cam["ivp"].astype(F).reshape(-1)
    wx = m[0] * nx + m[4] * ny + m[8] + m[12]
    wy = m[1] * nx + m[5] * ny + m[9] + m[13]
    wz = m[2] * nx + m[6] * ny + m[10] + m[14]
    ww = m[3] * nx + m[7] * ny + m[11] + m[15]
    world = np.stack([wx / ww, wy / ww, wz / ww], axis=-1)
    cpos = np.array([np.asarray(cam["position"]).reshape(-1)[k] for k in range(3)], dtype=F)
    o = np.broadcast_to(cpos, (len(fx), 3)).astype(F)
    return o, npp._normalize(world - cpos[None, :])


def _guides_of(ref, o, hit, tri, inst, lpos, lout, u, v, front):
    s = npp._shading(ref, tri, inst, lpos, lout, u, v, front)
    n = len(o)
    diff = s["position"] - o
    dist = np.sqrt(npp._dot(diff, diff))
    pos = np.concatenate([s["position"], dist[:, None]], axis=1)
    nrm = np.concatenate([s["normal"], np.zeros((n, 1), F)], axis=1)
    e = s["emission"]
    lum = F(0.2126) * e[:, 0] + F(0.7152) * e[:, 1] + F(0.0722) * e[:, 2]
    alb3 = np.where((lum > 0)[:, None], F(1.0), s["diffuse"] + s["f0"])
    alb = np.concatenate([alb3, np.zeros((n, 1), F)], axis=1)
    miss_p = np.array([0, 0, 0, -1], F)
    miss_a = np.array([1, 1, 1, 0], F)
    pos = np.where(hit[:, None], pos, miss_p[None, :]).astype(F)
    nrm = np.where(hit[:, None], nrm, F(0.0)).astype(F)
    alb = np.where(hit[:, None], alb, miss_a[None, :]).astype(F)
    return pos, nrm, alb


def guides(ref, cam, width, height):
    """(position_t, normal, albedo), float32 [H, W, 4] each: the smallest accepted t over every triangle of every instance
    (np_path._closest_hit's test, restated per triangle in _tri_tests so that the triangle kept and its instance stay together;
    at an exact distance tie the last one tested is kept: the pin has no tie rule, see guides_match), np_path._shading of it."""
    with np.errstate(all="ignore"):
        o, d = centre_rays(cam, width, height)
        n = len(o)
        best = np.full(n, F(1e9), F)
        tri, inst = np.zeros(n, np.int64), np.zeros(n, np.int64)
        lpos, lout = np.zeros((n, 3), F), np.zeros((n, 3), F)
        bu, bv, bfront = np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool)
        for i, ti, ok, t, p, od, u, v, front in _tri_tests(ref, o, d):
            ok = ok & ~(t > best)
            best = np.where(ok, t, best)
            tri, inst = np.where(ok, ti, tri), np.where(ok, i, inst)
            lpos, lout = np.where(ok[:, None], p, lpos), np.where(ok[:, None], od, lout)
            bu, bv, bfront = np.where(ok, u, bu), np.where(ok, v, bv), np.where(ok, front, bfront)
        g = _guides_of(ref, o, best < F(1e9), tri, inst, lpos, lout, bu, bv, bfront)
    return tuple(a.reshape(height, width, 4) for a in g)


def _instance_triangles(ref):
    return [(i, npp._leaf_triangles(ref.bvh_nodes, inst["blas_index"])) for i, inst in enumerate(ref.instances)]


def _tri_tests(ref, o, d):
    """Moller-Trumbore (main.glsl:224-257) of every ray against every triangle of every instance, one triangle at a time:
    yields (instance, triangle, accepted, t, local position, local out_dir, u, v, front), acceptance without the t <= best test"""
    geom = ref.tri_geom["vertices"]
    for i, tris in _instance_triangles(ref):
        inv = ref.instances[i]["inverse_transform"].astype(F)
        lo, ld = npp._mat_point(inv, o), npp._mat_dir(inv, d)
        for ti in tris:
            v0, v1, v2 = (geom[ti][k][:3].astype(F) for k in range(3))
            e1, e2 = v1 - v0, v2 - v0
            pvec = npp._cross(ld, e2[None, :])
            det = npp._dot(e1[None, :], pvec)
            inv_det = F(1.0) / det
            tvec = lo - v0[None, :]
            u = npp._dot(tvec, pvec) * inv_det
            qvec = npp._cross(tvec, e1[None, :])
            v = npp._dot(ld, qvec) * inv_det
            t = npp._dot(e2[None, :], qvec) * inv_det
            ok = ~(np.abs(det) < F(1e-5)) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & ~((t < 0) | (t > F(1e9)))
            front = npp._dot(npp._cross(e1[None, :], e2[None, :]), ld) > 0
            yield i, ti, ok, t, lo + t[:, None] * ld, -ld, u, v, front


def brute_force_t(ref, cam, width, height):
    """the smallest accepted t per pixel over all triangles of all instances (1e9: a miss), float32 [H * W]"""
    with np.errstate(all="ignore"):
        o, d = centre_rays(cam, width, height)
        best = np.full(len(o), F(1e9), F)
        for _, _, ok, t, *_ in _tri_tests(ref, o, d):
            best = np.where(ok & (t < best), t, best)
    return best


def guides_match(ref, cam, width, height, position_t, normal, albedo):
    """Per pixel [H * W]: do the three guide texels given equal, bit for bit, those of SOME triangle at the pixel's minimal t
    (exact ties may pick any of the tying triangles), or the miss encoding when nothing is hit?  Also returns the minimal t."""
    got = np.concatenate([np.asarray(a, F).reshape(-1, 4) for a in (position_t, normal, albedo)], axis=1).view(np.uint32)
    with np.errstate(all="ignore"):
        o, d = centre_rays(cam, width, height)
        best = brute_force_t(ref, cam, width, height)
        n = len(o)
        matched = np.zeros(n, bool)
        miss = best >= F(1e9)
        if miss.any():
            z = np.zeros(n, np.int64)
            g = _guides_of(ref, o, np.zeros(n, bool), z, z, np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool))
            want = np.concatenate(g, axis=1).view(np.uint32)
            matched |= miss & (want == got).all(axis=1)
        for i, ti, ok, t, lpos, lout, u, v, front in _tri_tests(ref, o, d):
            sel = np.nonzero(ok & (t == best) & ~miss)[0]
            if len(sel) == 0:
                continue
            g = _guides_of(ref, o[sel], np.ones(len(sel), bool), np.full(len(sel), ti, np.int64), np.full(len(sel), i, np.int64), lpos[sel],
                           lout[sel], u[sel], v[sel], front[sel])
            want = np.concatenate(g, axis=1).view(np.uint32)
            matched[sel] |= (want == got[sel]).all(axis=1)
    return matched, best


# ---- filter -----------------------------------------------------------------------------------------------------------------

def _pos(v):
    return np.where(v > 0, v, F(0.0)).astype(F)      # max(0, v); a NaN gives 0


def _finite3(c):
    return np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2])


def amod(albedo):
    a = np.asarray(albedo, F)[..., :3]
    return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR).astype(F)


def _shift(a, dx, dy):
    """a[y + dy, x + dx] where inside the image (zeros elsewhere) and the mask of where that is"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
        ok[ys0:ys1, xs0:xs1] = True
    return out, ok


def atrous_pass(ik, position_t, normal, k, npow, sigma_plane, sigma_color):
    """i_k -> i_k+1 (float32 [H, W, 3]); position_t / normal [H, W, 4]"""
    s = 1 << k
    sc = F(sigma_color)
    for _ in range(k):
        sc = F(sc * F(0.5))
    sc2 = F(sc * sc)
    xp, tp, n_p = position_t[..., :3], position_t[..., 3], normal[..., :3]
    pm = tp < 0
    acc = np.zeros_like(ik)
    wsum = np.zeros(ik.shape[:2], F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, inside = _shift(ik, s * dx, s * dy)
            pq, _ = _shift(position_t, s * dx, s * dy)
            nq, _ = _shift(normal, s * dx, s * dy)
            qm = pq[..., 3] < 0
            wn = _pos(n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1] + n_p[..., 2] * nq[..., 2])
            for _ in range(npow):
                wn = wn * wn
            dxyz = pq[..., :3] - xp
            rz = np.abs(n_p[..., 0] * dxyz[..., 0] + n_p[..., 1] * dxyz[..., 1] + n_p[..., 2] * dxyz[..., 2]) / (F(sigma_plane) * tp)
            g = _pos(F(1.0) - rz)
            e = np.where(pm & qm, F(1.0), np.where(pm | qm, F(0.0), wn * (g * g))).astype(F)
            dc = cq - ik
            wc = F(1.0) / (F(1.0) + (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2]) / sc2)
            ew = (e * wc).astype(F)
            if dx == 0 and dy == 0:
                ew = np.ones_like(ew)
            wt = ((H5[dy + 2] * H5[dx + 2]) * ew).astype(F)
            wt = np.where(_finite3(cq) & (ew == ew) & inside, wt, F(0.0)).astype(F)
            use = wt != 0
            acc = acc + np.where(use[..., None], cq * wt[..., None], F(0.0)).astype(F)
            wsum = wsum + wt
    out = acc / wsum[..., None]
    return np.where(_finite3(ik)[..., None], out, ik).astype(F)


def atrous(mean, position_t, normal, albedo, passes=5, normal_power_log2=6, sigma_plane=0.02, sigma_color=4.0):
    """the filter on a mean image (float32 [H, W, >= 3]) -> the denoised image, float32 [H, W, 4] = (rgb, 1)"""
    with np.errstate(all="ignore"):
        mean = np.asarray(mean, F)[..., :3]
        position_t, normal = np.asarray(position_t, F), np.asarray(normal, F)
        am = amod(albedo)
        i = (mean / am).astype(F)
        for k in range(passes):
            i = atrous_pass(i, position_t, normal, k, normal_power_log2, sigma_plane, sigma_color)
        out = np.ones(mean.shape[:2] + (4,), F)
        out[..., :3] = i * am
    return out


def denoise(accum, frame_count, position_t, normal, albedo, **params):
    """jpt_denoise's image from the accumulation (sums, float32 [H, W, 4]) and the frame count"""
    with np.errstate(all="ignore"):
        mean = (np.asarray(accum, F)[..., :3] / F(frame_count)).astype(F)
    return atrous(mean, position_t, normal, albedo, **params)


def _clamp01(x):
    return np.fmin(np.fmax(x, F(0.0)), F(1.0))


def display(denoised):
    """unorm8(aces_film(denoised)), alpha 255: uint8 [H, W, 4] (progressive_rendering.glsl:19-26, float32 as the kernels)"""
    with np.errstate(all="ignore"):
        x = np.asarray(denoised, F)[..., :3]
        a, b, c, d, e = F(2.51), F(0.03), F(2.43), F(0.59), F(0.14)
        col = _clamp01((x * (a * x + b)) / (x * (c * x + d) + e))
        q = np.floor(_clamp01(col) * F(255.0) + F(0.5))
    out = np.full(x.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = q.astype(np.uint8)
    return out


# ---- synthetic inputs of the filter tests --------------------------------------------------------------------------------------

def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN (which payload a NaN operand leaves is not part of the pin)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def synthetic_case(width, height, seed=0):
    """(mean, position_t, normal, albedo), float32 [H, W, 4] each: a wall facing a camera at the origin with a depth step at 40 %
    of the width and a crease at 70 %, a miss region in the upper right, albedos that include one under the floor, and a seeded
    random colour image with NaN, +inf and -inf pixels planted (images of more than 16 pixels)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    fx, fy = (xs + 0.5) / width, (ys + 0.5) / height
    z = np.where(fx < 0.4, -4.0, -6.0)
    px = (fx - 0.5) * 3.0
    crease = fx >= 0.7
    z = np.where(crease, z + (px - 0.6), z)
    pos = np.stack([px, (0.5 - fy) * 2.0, z], axis=-1).astype(F)
    nrm = np.zeros((height, width, 3), F)
    nrm[..., 2] = 1.0
    nrm[crease] = np.array([-0.70710678, 0.0, 0.70710678], F)
    t = np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).astype(F)
    miss = (fy < 0.2) & (fx > 0.5)
    position_t = np.concatenate([pos, t[..., None]], axis=-1).astype(F)
    position_t[miss] = np.array([0, 0, 0, -1], F)
    normal = np.concatenate([nrm, np.zeros((height, width, 1), F)], axis=-1).astype(F)
    normal[miss] = 0
    alb = np.where((fx < 0.4)[..., None], np.array([0.8, 0.3, 0.001], F), np.array([0.25, 1.0, 0.6], F)).astype(F)
    alb = np.where((fy > 0.8)[..., None], (alb * rng.random((height, width, 3)).astype(F)).astype(F), alb)
    albedo = np.concatenate([alb, np.zeros((height, width, 1), F)], axis=-1).astype(F)
    albedo[miss] = np.array([1, 1, 1, 0], F)
    mean = np.zeros((height, width, 4), F)
    mean[..., :3] = (rng.random((height, width, 3)) * 2.0).astype(F) * np.where(fx < 0.55, F(1.0), F(0.3))[..., None]
    if width * height > 16:
        flat = mean.reshape(-1, 4)
        n = len(flat)
        flat[n // 3, 0] = np.nan
        flat[n // 2, 1] = np.inf
        flat[(2 * n) // 3, 2] = -np.inf
        flat[n - 1, :3] = np.nan
        flat[7 % n, :3] = 1e30
    return mean, position_t, normal, albedo
