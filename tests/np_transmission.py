"""Transparent materials (jpt_set_material_extensions, csrc/jpt_shade.h material_transmission / material_ior / dielectric_event /
material_ext / transmission_step) restated in vectorised float32 numpy, the same binary32 operations in the same order, and the
whole path of the *_tx kernels as an extension of np_light_sampling.trace_lights: the miss model (gradient, map, map with MIS),
emitter sampling on or off, and the transmission lobe.  Test infrastructure."""
import numpy as np

import np_env
import np_env_sampling as nes
import np_lens
import np_light_sampling as nls
import np_path
import np_restatement as npr

F = np.float32
LOBE_HASH = (0x5bd1e995, 0x1b873593)
DELTA = F(-1.0)          # kDeltaDensity
EXT_TRANSMISSION = 1     # JPT_MATERIAL_EXT_TRANSMISSION


def transmission_of(x):
    x = np.asarray(x, F)
    x = np.where(x == x, x, F(0))
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def ior_of(x):
    x = np.asarray(x, F)
    x = np.where(x == x, x, F(1))
    return np.where(x < F(1), F(1), np.where(x > F(4), F(4), x)).astype(F)


def dielectric_event(n, v, ior, front, xi_f):
    """dielectric_event of csrc/jpt_shade.h: (d [k, 3], F [k], event [k]: 0 refract, 1 reflect, 2 total internal reflection)"""
    n, v = np.asarray(n, F).reshape(-1, 3), np.asarray(v, F).reshape(-1, 3)
    k_ = len(n)
    ior = ior_of(np.broadcast_to(np.asarray(ior, F), (k_,)))
    front = np.broadcast_to(np.asarray(front), (k_,)).astype(bool)
    xi_f = np.broadcast_to(np.asarray(xi_f, F), (k_,)).astype(F)
    with np.errstate(all="ignore"):
        ndv = n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1] + n[:, 2] * v[:, 2]
        m = np.where((ndv < F(0))[:, None], -n, n)
        c = np.abs(ndv)
        c = np.where(c < F(1), c, F(1)).astype(F)
        inv = F(1) / ior
        eta = np.where(front, inv, ior).astype(F)
        etap = np.where(front, ior, inv).astype(F)
        k = F(1) - (eta * eta) * (F(1) - c * c)
        tir = k < F(0)
        ct = np.where(tir, F(0), np.sqrt(np.where(tir, F(0), k))).astype(F)
        a, b = etap * ct, etap * c
        rs, rp = (c - a) / (c + a), (ct - b) / (ct + b)
        f = F(0.5) * (rs * rs + rp * rp)
        fres = np.where(tir, F(1), np.where(f <= F(1), f, F(1))).astype(F)
        event = np.where(tir, 2, np.where(xi_f < fres, 1, 0)).astype(np.uint8)
        t = F(2) * c
        refl = m * t[:, None] - v
        g = eta * c - ct
        r = m * g[:, None] - v * eta[:, None]
        il = F(1) / np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        refr = r * il[:, None]
        d = np.where((event != 0)[:, None], refl, refr).astype(F)
    return d, fres, event


def _tex_index(f, res, repeat):
    """tex_index of csrc/jpt_shade.h on floor()ed coordinates"""
    nan = f != f
    f = np.where(nan, F(0), f)
    if not repeat:
        i = np.where(f >= F(res - 1), res - 1, np.where(f <= F(0), 0, np.trunc(np.clip(f, 0, res)).astype(np.int64)))
    else:
        big = (f >= F(1073741824.0)) | (f <= F(-1073741824.0))
        i = np.trunc(np.where(big, F(0), f)).astype(np.int64) % res     # (python's % is the non-negative modulo)
        i = np.where(big, 0, i)
    return np.where(nan, 0, i)


def _texture(tex, u, v, layer, mode):
    """sample_texture of csrc/jpt_shade.h, the nearest filter: rgb [k, 3] float32 (texel / 255 correctly rounded: from_unorm8)"""
    assert (mode & 2) == 0, "np_transmission samples with the nearest filter only"
    res = tex.shape[1]
    layer = np.minimum(layer, tex.shape[0] - 1)
    with np.errstate(all="ignore"):
        ix = _tex_index(np.floor(u * F(res)), res, bool(mode & 1))
        iy = _tex_index(np.floor(v * F(res)), res, bool(mode & 1))
    return (tex[layer, iy, ix, :3].astype(F) / F(255)).astype(F)


class _Untextured:
    """`ref` with every material's texture index -1: what np_path._shading (no textures) is given"""
    def __init__(self, ref):
        self.tri_geom, self.tri_data, self.bvh_nodes, self.instances = ref.tri_geom, ref.tri_data, ref.bvh_nodes, ref.instances
        self.materials = ref.materials.copy()
        self.materials["albedo_texture_index"] = -1


def shading(ref, plain, tri, blas, lpos, lout, u, v, front, textures=None, sampler_mode=0):
    """np_path._shading with get_shading_data's texture, and the lobe's inputs: tint [k, 3], material ids"""
    P = np_path
    s = P._shading(plain, tri, blas, lpos, lout, u, v, front)
    mat_id = nls._material_ids(ref, blas, tri)
    mat = ref.materials[mat_id]
    albedo = mat["albedo"].astype(F)[:, :3]
    layer = mat["albedo_texture_index"].astype(np.int64)
    has = layer >= 0
    if has.any():
        if textures is None or len(textures) == 0:
            texel = np.zeros((len(tri), 3), F)
        else:
            uvs = ref.tri_data["uvs"][tri].astype(F)
            w0 = F(1.0) - u - v
            uvx = uvs[:, 0, 0] * w0 + uvs[:, 1, 0] * u + uvs[:, 2, 0] * v
            uvy = uvs[:, 0, 1] * w0 + uvs[:, 1, 1] * u + uvs[:, 2, 1] * v
            texel = _texture(np.asarray(textures), uvx, uvy, np.maximum(layer, 0), sampler_mode)
        albedo = np.where(has[:, None], albedo * texel, albedo).astype(F)
        metal = mat["metallic"].astype(F)
        s["f0"] = P._mix(F(0.02), albedo, metal[:, None])
        s["diffuse"] = albedo - albedo * metal[:, None]
    return s, albedo, mat_id


def trace_tx(ref, cam, width, height, max_bounces, ext_flags, rgb=None, rot=None, intensity=1.0, env_mis=False, light_tabs=None,
             textures=None, sampler_mode=0, lens=None):
    """the path of the *_tx kernels: radiance [H, W, 3] float32.  ext_flags: JPT_MATERIAL_EXT_*; rgb None: the gradient sky;
    env_mis: the map's NEE too; light_tabs: np_light_sampling.tables(ref) for JPT_LIGHT_SAMPLING_MIS, None for emitter sampling off;
    lens: (radius, focus) of jpt_set_lens, None or radius 0 for the pinhole (the lens draws from a hashed copy of the seed after the
    jitter draw and does not advance it: np_lens.lens_xi)"""
    P = np_path
    plain = _Untextured(ref)
    total = F(0) if light_tabs is None else light_tabs["total"]
    etabs = nes.tables(rgb) if (rgb is not None and env_mis) else None
    if etabs is not None and not etabs[2] > F(0):
        etabs = None   # (a black map's MIS render is the BRDF-mode render)
    pad = ref.materials["padding"].astype(F)
    on = (int(ext_flags) & EXT_TRANSMISSION) != 0
    t_all = transmission_of(pad[:, 0]) if on else np.zeros(len(pad), F)
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
        if lens is not None and float(lens[0]) > 0.0:
            o, d = np_lens.lens_apply(np_lens.basis(cam), lens[0], lens[1], o, d, np_lens.lens_xi(seed))
        radiance = np.zeros((n, 3), dtype=F)
        throughput = np.ones((n, 3), dtype=F)
        alive = np.ones(n, dtype=bool)
        p_brdf = np.zeros(n, dtype=F)
        for i in range(max_bounces + 1):
            t, tri, blas, lpos, lout, u, v, front = P._closest_hit(ref, o, d)
            hit = t < F(1e9)
            delta = p_brdf == DELTA     # the previous vertex was a dielectric one: every weight here is 1
            sky = nls._gradient_sky(d) if rgb is None else np_env.env_radiance(rgb, d, rot, intensity)
            sky_term = throughput * sky
            if i > 0 and etabs is not None:
                pe = nes.pdf(rgb, etabs, d, rot)
                wm = np.where(pe > F(0), (p_brdf * p_brdf) / (p_brdf * p_brdf + pe * pe), F(1)).astype(F)
                wm = np.where(delta, F(1), wm).astype(F)
                sky_term = sky_term * wm[:, None]
            s, tint, mat_id = shading(ref, plain, tri, blas, lpos, lout, u, v, front, textures, sampler_mode)
            hit_term = throughput * s["emission"]
            if i > 0:
                le = s["emission"]
                _, e1, e2 = nls._world_edges(ref, blas, tri)
                dv = s["position"] - o
                pl = nls.light_pdf(le, total, P._dot(dv, dv), nls.light_cos(e1, e2, d))
                wl = ((p_brdf * p_brdf) / (p_brdf * p_brdf + pl * pl)).astype(F)
                wl = np.where(wl == wl, wl, F(1))
                weighted = (nls.lum(le) > F(0)) & (total > F(0))
                wl = np.where(weighted & ~delta, wl, F(1)).astype(F)
                hit_term = hit_term * wl[:, None]   # (every path at bounce >= 1 multiplies by its weight, 1 included: x * 1 is x)
            term = np.where(hit[:, None], hit_term, sky_term)
            radiance = np.where(alive[:, None], radiance + term, radiance)
            alive = alive & hit
            # the lobe choice: one round over a hashed copy of the seeds
            hs = (seed ^ np.array(LOBE_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
            _, xl = npr.pcg2d(hs)
            glass = alive & (xl[:, 0] < t_all[mat_id])
            opaque = alive & ~glass
            so = s["position"] + s["normal"] * F(0.001)
            if i < max_bounces and etabs is not None:
                hs = (seed ^ np.array(nes.NEE_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
                _, xi = npr.pcg2d(hs)
                l, pe = nes.sample(rgb, etabs, xi[:, 0], xi[:, 1], rot)
                ndl = P._dot(s["normal"], l)
                pb = P._density(s, l)
                w = (pe * pe) / (pe * pe + pb * pb)
                c = ((throughput * (P._brdf(s, l) * ndl[:, None])) * np_env.env_radiance(rgb, l, rot, intensity)) * (w / pe)[:, None]
                emit = opaque & (pe > F(0)) & (ndl > F(0)) & (c > F(0)).any(axis=1)
                blocked = np.ones(n, dtype=bool)
                if emit.any():
                    blocked[emit] = P._closest_hit(ref, so[emit], l[emit])[0] < F(1e9)
                radiance = np.where((emit & ~blocked)[:, None], radiance + c, radiance)
            if i < max_bounces and total > F(0):
                hs = (seed ^ np.array(nls.LIGHT_HASH, dtype=seed.dtype)[None, :]).astype(seed.dtype)
                hs, xa = npr.pcg2d(hs)
                _, xb = npr.pcg2d(hs)
                y, e1, e2, le = nls.sample(light_tabs, np.concatenate([xa, xb], axis=1))
                dv = y - so
                d2 = P._dot(dv, dv)
                l = P._normalize(dv)
                ndl = P._dot(s["normal"], l)
                c_y = nls.light_cos(e1, e2, l)
                pl = nls.light_pdf(le, total, d2, c_y)
                pb = P._density(s, l)
                w = (pl * pl) / (pl * pl + pb * pb)
                c = ((throughput * (P._brdf(s, l) * ndl[:, None])) * le) * (w / pl)[:, None]
                emit = opaque & (ndl > F(0)) & (c_y > F(0)) & np.isfinite(c).all(axis=1) & (c > F(0)).any(axis=1)
                tmax = (np.sqrt(d2) * nls.SHADOW_SCALE).astype(F)
                blocked = np.ones(n, dtype=bool)
                if emit.any():
                    blocked[emit] = P._closest_hit(ref, so[emit], l[emit])[0] < tmax[emit]
                radiance = np.where((emit & ~blocked)[:, None], radiance + c, radiance)
            # the path's own draw: taken by both kinds of vertex, used by the opaque one only
            seed2, xi = npr.pcg2d(seed)
            seed = np.where(alive[:, None], seed2, seed)
            new_d = P._sample_brdf(s, xi)
            dens = P._density(s, new_d)
            lambert_in = P._dot(s["normal"], new_d)
            gd, _, gev = dielectric_event(s["normal"], s["out_dir"], ior_of(pad[mat_id, 1]), front, xl[:, 1])
            refracted = gev == 0
            go = s["position"] + s["normal"] * np.where(refracted, F(-0.001), F(0.001)).astype(F)[:, None]
            o = np.where(glass[:, None], go, np.where(alive[:, None], so, o))
            d = np.where(glass[:, None], gd, np.where(alive[:, None], new_d, d))
            p_brdf = np.where(glass, DELTA, np.where(alive, dens, p_brdf)).astype(F)
            alive = alive & (glass | ~(lambert_in <= 0))
            f = (P._brdf(s, new_d) * lambert_in[:, None]) / dens[:, None]
            throughput = np.where((glass & refracted)[:, None], throughput * tint, np.where((alive & ~glass)[:, None], throughput * f, throughput))
        return radiance.reshape(height, width, 3)
