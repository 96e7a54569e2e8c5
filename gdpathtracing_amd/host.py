"""Host-side mirror of the reference's interface for this path, over the C ABI (include/jpt.h).

Same names and meaning as the reference's C++ classes, minus the Godot scene tree:

  GeometryGroup3D      src/path_tracing/geometry_group3d.{h,cpp}   build(), get_*_buffer(), counts
  PathTracingCamera    src/path_tracing/path_tracing_camera.{h,cpp} init(), render(), denoising_mode
  ProgressiveRendering src/path_tracing/post_processing/progressive_rendering.{h,cpp}  frame_count logic

This is plumbing (ctypes + numpy); the product is libjpt_hip.so.  The C++ form of the same adapter, for
linking into the addon, is described in INTEGRATION.md.
"""
from __future__ import annotations

import atexit
import ctypes as C
import weakref
from typing import Optional

import numpy as np

from . import capi, scenes, wire


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


_live_contexts = weakref.WeakSet()


def _update_surfaces(mesh: scenes.Mesh, with_normals: bool = True):
    """jpt_surface array of a deformed mesh for jpt_scene_update_mesh (uvs are not read); the caller keeps `mesh` alive"""
    arr = (capi.Surface * len(mesh.surfaces))()
    for i, s in enumerate(mesh.surfaces):
        arr[i].vertices, arr[i].indices = _ptr(s.vertices), _ptr(s.indices)
        arr[i].normals = _ptr(s.normals) if with_normals else None
        arr[i].n_vertices, arr[i].n_indices = len(s.vertices), len(s.indices)
    return arr


class SurfaceRig:
    """One surface's part of a rig (jpt_surface_rig): bones int32 [n_vertices, influences] and weights float32 of the same shape (None
    without bones), position_deltas float32 [n_blend_shapes, n_vertices, 3] (None without shapes), normal_deltas the same or None."""

    def __init__(self, bones=None, weights=None, position_deltas=None, normal_deltas=None):
        c = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.bones, self.weights = c(bones, np.int32), c(weights, np.float32)
        self.position_deltas, self.normal_deltas = c(position_deltas, np.float32), c(normal_deltas, np.float32)


def _rig_surfaces(rigs):
    """jpt_surface_rig array of a list of SurfaceRig; the caller keeps `rigs` alive"""
    arr = (capi.SurfaceRig * len(rigs))()
    for i, r in enumerate(rigs):
        arr[i].bones, arr[i].weights = _ptr(r.bones), _ptr(r.weights)
        arr[i].position_deltas, arr[i].normal_deltas = _ptr(r.position_deltas), _ptr(r.normal_deltas)
    return arr


def _pose_arrays(bone_transforms12, blend_weights):
    b = None if bone_transforms12 is None else np.ascontiguousarray(bone_transforms12, dtype=np.float32).reshape(-1, 12)
    w = None if blend_weights is None else np.ascontiguousarray(blend_weights, dtype=np.float32).reshape(-1)
    return b, (0 if b is None else len(b)), w, (0 if w is None else len(w))


def debug_skin(device_id, bind_positions, bind_normals, rig: "SurfaceRig", influences, n_blend_shapes, bone_transforms12=None, blend_weights=None):
    """jpt_debug_skin: jpt_scene_pose_mesh's arithmetic alone on one caller-made surface -- (positions, normals) float32 [n_vertices, 3]
    each (normals None without bind normals).  device_id -1: the host's copy of the functions, in plain loops.  A refusal raises
    capi.JptError with the library's code as its second argument."""
    L = capi.lib()
    pos = np.ascontiguousarray(bind_positions, dtype=np.float32).reshape(-1, 3)
    nrm = None if bind_normals is None else np.ascontiguousarray(bind_normals, dtype=np.float32).reshape(-1, 3)
    b, nb, w, _ = _pose_arrays(bone_transforms12, blend_weights)
    out_p = np.zeros_like(pos)
    out_n = None if nrm is None else np.zeros_like(nrm)
    rc = L.jpt_debug_skin(device_id, _ptr(pos), _ptr(nrm), len(pos), _ptr(rig.bones), _ptr(rig.weights), influences, _ptr(rig.position_deltas),
                          _ptr(rig.normal_deltas), n_blend_shapes, _ptr(b), nb, _ptr(w), _ptr(out_p), _ptr(out_n))
    if rc != capi.OK:
        msg = L.jpt_debug_last_error()
        raise capi.JptError("jpt_debug_skin failed (%d): %s" % (rc, msg.decode() if msg else ""), rc)
    return out_p, out_n


def _debug_check(L, rc, what):
    if rc != capi.OK:
        msg = L.jpt_debug_last_error()
        raise capi.JptError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""), rc)


def debug_tlas_order(device_id, lo, hi, with_keys=True):
    """jpt_debug_tlas_order: the sort of jpt_scene_rebuild_tlas alone over caller-made world boxes (float32 [n, 3] each) -- (keys uint64
    [n] per instance, or None; the instance at every sorted position, uint32 [n]).  device_id -1: the host's copy of the functions."""
    L = capi.lib()
    lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(-1, 3)
    keys = np.zeros(len(lo), np.uint64) if with_keys else None
    order = np.zeros(len(lo), np.uint32)
    _debug_check(L, L.jpt_debug_tlas_order(device_id, _ptr(lo), _ptr(hi), len(lo), _ptr(keys), _ptr(order)), "jpt_debug_tlas_order")
    return keys, order


def debug_mesh_order(device_id, vertices, indices, with_codes=True):
    """jpt_debug_mesh_order: the order of jpt_scene_rebuild_mesh alone over a caller-made mesh (vertices float32 [v, 3], indices uint32
    [t, 3]) -- (codes uint32 [t] per triangle, or None; the triangle at every sorted position, uint32 [t]).  device_id -1: the host's
    copy of the functions."""
    L = capi.lib()
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    codes = np.zeros(len(ix), np.uint32) if with_codes else None
    order = np.zeros(len(ix), np.uint32)
    _debug_check(L, L.jpt_debug_mesh_order(device_id, _ptr(v), len(v), _ptr(ix), len(ix), _ptr(codes), _ptr(order)), "jpt_debug_mesh_order")
    return codes, order


def debug_tlas_template(n):
    """jpt_debug_tlas_template: the tree jpt_scene_rebuild_tlas puts over n sorted positions -- dict with `child` (int32 [n_records, 4]:
    >= 0 a record, ~position a leaf, INT32_MIN empty), `n_levels` and `stack_need`."""
    L = capi.lib()
    nr, nl, sn = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _debug_check(L, L.jpt_debug_tlas_template(n, None, 0, C.byref(nr), C.byref(nl), C.byref(sn)), "jpt_debug_tlas_template")
    child = np.zeros((nr.value, 4), np.int32)
    _debug_check(L, L.jpt_debug_tlas_template(n, _ptr(child), nr.value, C.byref(nr), C.byref(nl), C.byref(sn)), "jpt_debug_tlas_template")
    return dict(child=child, n_levels=int(nl.value), stack_need=int(sn.value))


@atexit.register
def _close_live_contexts():
    # contexts the caller forgot to close are destroyed while the HIP runtime is still up (this handler is registered
    # after torch's, so it runs before it), not from __del__ during interpreter teardown
    for ctx in list(_live_contexts):
        try:
            ctx.close()
        except Exception:
            pass


def _env_map(rgb):
    """An environment map as the C ABI takes it: float32 [height, width, 3], C order (None stays None)."""
    if rgb is None:
        return None, 0, 0
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an environment map is a [height, width, 3] array")
    return a, a.shape[1], a.shape[0]


def _env_rotation(rotation):
    if rotation is None:
        return None
    return np.ascontiguousarray(rotation, dtype=np.float32).reshape(9)


def _sky_ref(params):
    return None if params is None else C.byref(params)


def debug_sky(device_id, params, width, height, samples):
    """jpt_debug_sky: the width x height map of the procedural sky `params` (a capi.SkyParams; None: the defaults), float32 [height,
    width, 3].  device_id >= 0: jpt_set_sky's kernel on that device; -1: the same functions in a host loop."""
    L = capi.lib()
    out = np.zeros((max(int(height), 0), max(int(width), 0), 3), np.float32)
    rc = L.jpt_debug_sky(int(device_id), _sky_ref(params), int(width), int(height), int(samples), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_sky failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_sky_radiance(params, dirs):
    """jpt_debug_sky_radiance: sky_radiance of n unit directions [n, 3] (theta = atan2_(|d.xz|, d.y)), on the host -- float32 [n, 3]"""
    L = capi.lib()
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 3), np.float32)
    rc = L.jpt_debug_sky_radiance(_sky_ref(params), _ptr(d), len(d), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_sky_radiance failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_pow01(b, e):
    """jpt_debug_pow01: the pinned b^e (b in [0, 1], e in [1/8, 64]) of the procedural sky, on the host -- float32 [n]"""
    L = capi.lib()
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, np.float32), b.shape))
    out = np.zeros(len(b), np.float32)
    rc = L.jpt_debug_pow01(_ptr(b), _ptr(e), len(b), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_pow01 failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_dielectric(device_id, normals, out_dirs, ior, front, xi_f):
    """jpt_debug_dielectric: the dielectric event of capi.MATERIAL_EXT_TRANSMISSION for n cases -- (dirs [n, 3] float32, fresnel [n]
    float32, event [n] uint8: 0 refract, 1 reflect, 2 total internal reflection).  device_id -1: the host's copy of the function."""
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    out = np.ascontiguousarray(out_dirs, np.float32).reshape(-1, 3)
    n = len(nrm)
    ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, np.float32), (n,)))
    front = np.ascontiguousarray(np.broadcast_to(np.asarray(front), (n,)).astype(np.uint8))
    xi_f = np.ascontiguousarray(np.broadcast_to(np.asarray(xi_f, np.float32), (n,)))
    dirs, fresnel, event = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    L = capi.lib()
    rc = L.jpt_debug_dielectric(int(device_id), _ptr(nrm), _ptr(out), _ptr(ior), _ptr(front), _ptr(xi_f), n, _ptr(dirs), _ptr(fresnel), _ptr(event))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_dielectric failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return dirs, fresnel, event


def debug_lens_rays(device_id, camera160, width, height, frame_index, aperture_radius, focus_distance):
    """jpt_debug_lens_rays: the ray generation of a render with set_lens(aperture_radius, focus_distance) for every pixel of one frame
    -- (origins [height, width, 3], dirs [height, width, 3]) float32.  device_id -1: the host's copy of the functions."""
    cam = np.ascontiguousarray(camera160).tobytes()
    if len(cam) != 160:
        raise ValueError("camera160 is the 160-byte Camera block")
    origins, dirs = np.zeros((height, width, 3), np.float32), np.zeros((height, width, 3), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_lens_rays(int(device_id), cam, int(width), int(height), int(frame_index), float(aperture_radius), float(focus_distance),
                               _ptr(origins), _ptr(dirs))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_lens_rays failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return origins, dirs


def debug_camera_rays(device_id, camera160, width, height, frame_index, model):
    """jpt_debug_camera_rays: the ray generation of a render with set_camera_model(model) for every pixel of one frame -- (origins
    [height, width, 3], dirs [height, width, 3]) float32.  device_id -1: the host's copy of the functions."""
    cam = np.ascontiguousarray(camera160).tobytes()
    if len(cam) != 160:
        raise ValueError("camera160 is the 160-byte Camera block")
    origins, dirs = np.zeros((height, width, 3), np.float32), np.zeros((height, width, 3), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_camera_rays(int(device_id), cam, int(width), int(height), int(frame_index), int(model), _ptr(origins), _ptr(dirs))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_camera_rays failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return origins, dirs


def _bake_surface(surface, uv2, transform12):
    """(jpt_surface, uv2 [n, 2], transform12 [12]) for jpt_bake_add_surface / jpt_debug_bake_raster; the caller keeps the tuple alive"""
    uv = np.ascontiguousarray(uv2, dtype=np.float32).reshape(-1, 2)
    if len(uv) != len(surface.vertices):
        raise ValueError("uv2 has one (u, v) per vertex")
    t12 = np.ascontiguousarray(transform12, dtype=np.float32).reshape(12)
    s = capi.Surface()
    s.vertices, s.normals, s.uvs, s.indices = _ptr(surface.vertices), _ptr(surface.normals), _ptr(surface.uvs), _ptr(surface.indices)
    s.n_vertices, s.n_indices = len(surface.vertices), len(surface.indices)
    return s, uv, t12


def _bake_images(position4, normal4):
    p = np.ascontiguousarray(position4, dtype=np.float32)
    n = np.ascontiguousarray(normal4, dtype=np.float32)
    if p.ndim != 3 or p.shape[2] != 4 or n.shape != p.shape:
        raise ValueError("position4 and normal4 are float32 [height, width, 4]")
    return p, n


def debug_bake_rays(device_id, position4, normal4, frame_index):
    """jpt_debug_bake_rays: the first rays of a bake render's paths for every texel of one frame -- (origins [height, width, 3], dirs
    [height, width, 3]) float32 and valid [height, width] uint8 (an invalid texel: zeros).  device_id -1: the host's copy."""
    p, n = _bake_images(position4, normal4)
    h, w = p.shape[:2]
    origins, dirs, valid = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.uint8)
    L = capi.lib()
    rc = L.jpt_debug_bake_rays(int(device_id), _ptr(p), _ptr(n), w, h, int(frame_index), _ptr(origins), _ptr(dirs), _ptr(valid))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_bake_rays failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return origins, dirs, valid


def debug_bake_raster(device_id, surface, uv2, transform12, width, height):
    """jpt_debug_bake_raster: jpt_bake_add_surface on all-invalid images -- (position4, normal4) float32 [height, width, 4].
    device_id -1: a plain host loop over texels and triangles calling the same functions."""
    s, uv, t12 = _bake_surface(surface, uv2, transform12)
    p, n = np.zeros((height, width, 4), np.float32), np.zeros((height, width, 4), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_bake_raster(int(device_id), C.byref(s), _ptr(uv), _ptr(t12), int(width), int(height), _ptr(p), _ptr(n))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_bake_raster failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return p, n


def debug_bake_finish(device_id, mean4, position4, normal4, params=None, **fields):
    """jpt_debug_bake_finish: the whole transform of jpt_bake_finish (guides, filter passes, dilation) on caller-made images, float32
    [height, width, 4] each, mean4 taken as the mean itself -- the lightmap (r, g, b, coverage) float32 [height, width, 4].  params: a
    capi.BakeFinishParams, or its fields by name.  device_id -1: the host's copy of the functions, in plain loops."""
    p, n = _bake_images(position4, normal4)
    m = np.ascontiguousarray(mean4, dtype=np.float32)
    if m.shape != p.shape:
        raise ValueError("mean4 is float32 [height, width, 4], the size of the texel images")
    if params is None and fields:
        params = capi.BakeFinishParams(**fields)
    out = np.zeros(p.shape, np.float32)
    L = capi.lib()
    rc = L.jpt_debug_bake_finish(int(device_id), p.shape[1], p.shape[0], None if params is None else C.byref(params), _ptr(m), _ptr(p), _ptr(n), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_bake_finish failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_bake_moments(position4, normal4, radiance, first_frame_index, accum_mode=capi.ACCUM_HDR_F32, frame_count=1, moments=None):
    """jpt_debug_bake_moments: the moments of jpt_set_bake_directional on the host, over texel images float32 [height, width, 4] and
    radiance float32 [n_frames, height, width, 3] (frame f is frame first_frame_index + f) -- float32 [3, height, width, 4], plane k =
    (M_k.r, M_k.g, M_k.b, 0).  frame_count > 1 continues the sums of `moments` (a copy is returned)."""
    p, n = _bake_images(position4, normal4)
    r = np.ascontiguousarray(radiance, dtype=np.float32)
    if r.ndim != 4 or r.shape[1:] != (p.shape[0], p.shape[1], 3):
        raise ValueError("radiance is float32 [n_frames, height, width, 3], the size of the texel images")
    out = np.zeros((3,) + p.shape, np.float32) if moments is None else np.array(moments, dtype=np.float32, order="C")
    if out.shape != (3,) + p.shape:
        raise ValueError("moments is float32 [3, height, width, 4]")
    L = capi.lib()
    rc = L.jpt_debug_bake_moments(_ptr(p), _ptr(n), p.shape[1], p.shape[0], _ptr(r), r.shape[0], int(first_frame_index), int(frame_count), int(accum_mode),
                                  _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_bake_moments failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_variance_moments(radiance, accum_mode=capi.ACCUM_HDR_F32, frame_count=1, sum4=None, m2=None):
    """jpt_debug_variance_moments: the update of jpt_set_variance on the host over radiance float32 [n_frames, height, width, 3] --
    (sum, m2), float32 [height, width, 4] each: (sum.rgb, 1) as the accumulation holds it and (M2.rgb, 0).  frame_count is that of the
    first frame: 1 overwrites `sum4` / `m2` whatever they hold, more continues them (copies are returned)."""
    r = np.ascontiguousarray(radiance, dtype=np.float32)
    if r.ndim != 4 or r.shape[3] != 3:
        raise ValueError("radiance is float32 [n_frames, height, width, 3]")
    shape = (r.shape[1], r.shape[2], 4)
    s = np.zeros(shape, np.float32) if sum4 is None else np.array(sum4, dtype=np.float32, order="C")
    m = np.zeros(shape, np.float32) if m2 is None else np.array(m2, dtype=np.float32, order="C")
    if s.shape != shape or m.shape != shape:
        raise ValueError("sum4 and m2 are float32 [height, width, 4]")
    L = capi.lib()
    rc = L.jpt_debug_variance_moments(_ptr(r), r.shape[0], int(frame_count), int(accum_mode), _ptr(s), _ptr(m), shape[1], shape[0])
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_variance_moments failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return s, m


def debug_atrous_variance(device_id, sum4, m2, frame_count, position_t, normal, albedo, params=None, vparams=None):
    """jpt_debug_atrous_variance: the variance-guided filter of jpt_denoise over caller-made planes float32 [height, width, 4], on a
    device or (device_id -1, JPT_DEVICE_HOST_ONLY) on the host -- (the denoised image float32 [height, width, 4], the variance the last
    pass leaves float32 [height, width]).  params: a capi.DenoiseParams, vparams: a capi.DenoiseVarianceParams, or None for the defaults."""
    arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in (sum4, m2, position_t, normal, albedo)]
    h, w = arrays[0].shape[:2]
    if any(a.shape != (h, w, 4) for a in arrays):
        raise ValueError("every plane is float32 [height, width, 4]")
    out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    s, m, x, n, a = arrays
    rc = capi.lib().jpt_debug_atrous_variance(int(device_id), w, h, None if params is None else C.byref(params), None if vparams is None else C.byref(vparams),
                                              _ptr(s), _ptr(m), int(frame_count), _ptr(x), _ptr(n), _ptr(a), _ptr(out), _ptr(var))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_atrous_variance failed (%d)" % rc)
    return out, var


def debug_denoise_history(device_id, sum4, frame_count, position_t, normal, albedo, prev=None, prev_vp=None, same_view=False, params=None, hparams=None):
    """jpt_debug_denoise_history: the history stage of jpt_denoise over caller-made planes float32 [height, width, 4], on a device or
    (device_id -1, JPT_DEVICE_HOST_ONLY) on the host.  prev: the previous history set (integrated = (m.rgb, N), normal_s = (normal, S),
    position_t) or None; prev_vp: the previous call's view-projection matrix, 16 floats column-major (not read with same_view).
    Returns (iv = (m.rgb, v_0), integrated, normal_s): what the filter reads and the new set's first two planes (its third is
    position_t).  params: a capi.DenoiseParams, hparams: a capi.DenoiseHistoryParams, or None for the defaults."""
    arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in (sum4, position_t, normal, albedo)]
    h, w = arrays[0].shape[:2]
    old = [None, None, None] if prev is None else [np.ascontiguousarray(a, dtype=np.float32) for a in prev]
    if any(a.shape != (h, w, 4) for a in arrays + [a for a in old if a is not None]):
        raise ValueError("every plane is float32 [height, width, 4]")
    vp16 = None if prev_vp is None else np.ascontiguousarray(prev_vp, dtype=np.float32).reshape(16)
    outs = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
    s, x, n, a = arrays
    rc = capi.lib().jpt_debug_denoise_history(int(device_id), w, h, None if params is None else C.byref(params), None if hparams is None else C.byref(hparams),
                                              _ptr(s), int(frame_count), _ptr(x), _ptr(n), _ptr(a), None if vp16 is None else _ptr(vp16), int(bool(same_view)),
                                              *[None if o is None else _ptr(o) for o in old], *[_ptr(o) for o in outs])
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_denoise_history failed (%d)" % rc)
    return tuple(outs)


def debug_noise_estimate(device_id, sum4, m2, frame_count, params=None, valid=None, **fields):
    """jpt_debug_noise_estimate: jpt_noise_estimate's pass over caller-made planes float32 [height, width, 4], on a device or
    (device_id -1, JPT_DEVICE_HOST_ONLY) on the host --(the capi.NoiseResult as a dict, hist uint32 [256], tiles float32 [ceil(h / 8), ceil(w / 8)]).
    valid: bool [height, width], False = a texel without a surface, or None."""
    s = np.ascontiguousarray(sum4, dtype=np.float32)
    m = np.ascontiguousarray(m2, dtype=np.float32)
    if s.ndim != 3 or s.shape[2] != 4 or m.shape != s.shape:
        raise ValueError("sum4 and m2 are float32 [height, width, 4]")
    if params is None and fields:
        params = capi.NoiseParams(**fields)
    h, w = s.shape[:2]
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    if v is not None and v.shape != (h, w):
        raise ValueError("valid is [height, width]")
    hist = np.zeros(256, np.uint32)
    tiles = np.zeros((-(-h // 8), -(-w // 8)), np.float32)
    res = capi.NoiseResult()
    L = capi.lib()
    rc = L.jpt_debug_noise_estimate(int(device_id), w, h, None if params is None else C.byref(params), _ptr(s), _ptr(m), int(frame_count), _ptr(v),
                                    _ptr(hist), _ptr(tiles), C.byref(res))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_noise_estimate failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return res.as_dict(), hist, tiles


def probe_image_size(n_probes, tile_w, tile_h, probes_per_row):
    """(width, height) of the image n_probes tiles make, probes_per_row to a row (jpt_get_probe_image_size's rule)"""
    return int(probes_per_row) * int(tile_w), -(-int(n_probes) // int(probes_per_row)) * int(tile_h)


def debug_probe_rays(device_id, positions, tile_w, tile_h, probes_per_row, frame_index):
    """jpt_debug_probe_rays: the first rays of a probe render's paths for every pixel of one frame -- (origins [height, width, 3], dirs
    [height, width, 3]) float32 and valid [height, width] uint8 (a tile without a probe: zeros).  device_id -1: the host's copy."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    w, h = probe_image_size(max(len(pos), 1), max(int(tile_w), 1), max(int(tile_h), 1), max(int(probes_per_row), 1))
    origins, dirs, valid = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.uint8)
    L = capi.lib()
    rc = L.jpt_debug_probe_rays(int(device_id), _ptr(pos), len(pos), int(tile_w), int(tile_h), int(probes_per_row), int(frame_index), _ptr(origins), _ptr(dirs),
                                _ptr(valid))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_probe_rays failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return origins, dirs, valid


def debug_probe_basis(tile_w, tile_h, flags=capi.PROBE_RADIANCE):
    """jpt_debug_probe_basis: the host's quadrature table of (tile_w, tile_h, flags), float32 [tile_h, tile_w, 9]"""
    out = np.zeros((max(int(tile_h), 1), max(int(tile_w), 1), 9), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_probe_basis(int(tile_w), int(tile_h), int(flags), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_probe_basis failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_probe_project(device_id, accum4, frame_count, n_probes, tile_w, tile_h, probes_per_row, table):
    """jpt_debug_probe_project: the projection over a caller-made accumulation image (float32 [height, width, 4], the size the probes
    make), frame count and table ([tile_h, tile_w, 9]) -- float32 [n_probes, 9, 4], (r, g, b, 0) per coefficient.  device_id -1: the
    same sum in plain loops on the host."""
    a = np.ascontiguousarray(accum4, dtype=np.float32)
    t = np.ascontiguousarray(table, dtype=np.float32)
    w, h = probe_image_size(n_probes, tile_w, tile_h, probes_per_row)
    if a.shape != (h, w, 4) or t.size != int(tile_w) * int(tile_h) * 9:
        raise ValueError("accum4 is float32 [%d, %d, 4] and the table [tile_h, tile_w, 9]" % (h, w))
    out = np.zeros((int(n_probes), 9, 4), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_probe_project(int(device_id), _ptr(a), int(frame_count), int(n_probes), int(tile_w), int(tile_h), int(probes_per_row), _ptr(t), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_probe_project failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def reflection_image_size(n_probes, face_size, probes_per_row):
    """(width, height) of the image n_probes strips of six faces make, probes_per_row to a row (jpt_get_reflection_image_size's rule)"""
    return int(probes_per_row) * 6 * int(face_size), -(-int(n_probes) // int(probes_per_row)) * int(face_size)


def debug_cube_rays(device_id, positions, face_size, probes_per_row, frame_index):
    """jpt_debug_cube_rays: the first rays of a cube render's paths for every pixel of one frame -- float32 [height, width, 6], the
    origin then the direction (a strip without a probe: zeros).  device_id -1: the host's copy."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    w, h = reflection_image_size(max(len(pos), 1), max(int(face_size), 1), max(int(probes_per_row), 1))
    rays = np.zeros((h, w, 6), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_cube_rays(int(device_id), _ptr(pos), len(pos), int(face_size), int(probes_per_row), int(frame_index), _ptr(rays))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_cube_rays failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return rays


def debug_reflection_samples(face_size, n_levels, samples, level):
    """jpt_debug_reflection_samples: the host's sample table of output level `level` -- (entries float32 [kept, 4]: L_x, L_y, L_z, w;
    source levels uint8 [kept]); kept <= samples (the library pads with level byte 0xff, cut off here)"""
    table = np.zeros((max(int(samples), 1), 4), np.float32)
    lvl = np.zeros(max(int(samples), 1), np.uint8)
    L = capi.lib()
    rc = L.jpt_debug_reflection_samples(int(face_size), int(n_levels), int(samples), int(level), _ptr(table), _ptr(lvl))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_reflection_samples failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    kept = int((lvl != 0xff).sum())
    assert (lvl[:kept] != 0xff).all() and not table[kept:].any()
    return table[:kept].copy(), lvl[:kept].copy()


def debug_reflection_prefilter(device_id, accum4, frame_count, n_probes, face_size, probes_per_row, level, params=None, **fields):
    """jpt_debug_reflection_prefilter: level `level` of the chain of a caller-made accumulation image (float32 [height, width, 4], the
    size the probes make) -- float32 [n_probes, 6, s, s, 4], s = face_size >> level.  device_id -1: the same in plain loops on the host."""
    a = np.ascontiguousarray(accum4, dtype=np.float32)
    w, h = reflection_image_size(n_probes, face_size, probes_per_row)
    if a.shape != (h, w, 4):
        raise ValueError("accum4 is float32 [%d, %d, 4]" % (h, w))
    if params is None:
        params = capi.ReflectionParams(**fields)
    s = max(int(face_size) >> max(int(level), 0), 1)
    out = np.zeros((int(n_probes), 6, s, s, 4), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_reflection_prefilter(int(device_id), _ptr(a), int(frame_count), int(n_probes), int(face_size), int(probes_per_row), C.byref(params),
                                          int(level), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_reflection_prefilter failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_encode(device_id, texels4, fmt, divisor=1.0, alpha_one=False):
    """jpt_debug_encode: float32 [n, 4] texels in a jpt_encode format (rgb / divisor when it is not 1, alpha as given or 1) -- float16
    [n, 4] (ENCODE_RGBA16F), uint32 [n] (ENCODE_RGB9E5) or uint8 [n, 4] (ENCODE_RGBE8).  device_id -1: the same functions on the host."""
    t = np.ascontiguousarray(texels4, dtype=np.float32).reshape(-1, 4)
    L = capi.lib()
    out = capi.encoded_array(int(fmt), len(t)) if int(fmt) in (1, 2, 3) else np.zeros(1, np.uint8)
    rc = L.jpt_debug_encode(int(device_id), _ptr(t), len(t), float(divisor), 1 if alpha_one else 0, int(fmt), _ptr(out))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_encode failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return out


def debug_lens_sample(camera160, aperture_radius, focus_distance, origins, dirs, xi2):
    """jpt_debug_lens_sample: the lens step alone, on the host, for n pinhole rays and n (xi0, xi1) pairs -- (origins [n, 3], dirs
    [n, 3], basis [3, 3]: f, r, u) float32.  A basis that is not finite raises JptError (code E_STATE)."""
    cam = np.ascontiguousarray(camera160).tobytes()
    if len(cam) != 160:
        raise ValueError("camera160 is the 160-byte Camera block")
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    xi = np.ascontiguousarray(xi2, np.float32).reshape(-1, 2)
    n = len(o)
    o2, d2, basis = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((3, 3), np.float32)
    L = capi.lib()
    rc = L.jpt_debug_lens_sample(cam, float(aperture_radius), float(focus_distance), _ptr(o), _ptr(d), _ptr(xi), n, _ptr(o2), _ptr(d2), _ptr(basis))
    if rc != capi.OK:
        raise capi.JptError("jpt_debug_lens_sample failed (%d): %s" % (rc, (L.jpt_debug_last_error() or b"?").decode()))
    return o2, d2, basis


def make_rays(origins, dirs, tmax=None) -> np.ndarray:
    """a wire.RAY array (jpt_ray) from origins and dirs [n, 3] and tmax (a scalar or [n]; None: 0, which the library reads as
    unbounded)"""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), wire.RAY)
    rays["origin"] = o
    rays["dir"] = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if tmax is not None:
        rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    return rays


class Context:
    """One jpt_ctx (one GPU).  Thin, explicit wrapper: every method is one C-ABI call."""

    def __init__(self, device: int = 0, _borrowed=None):
        self._lib = capi.lib()
        self._owned = _borrowed is None
        if _borrowed is not None:       # a rank's context inside a MultiContext: the jpt_multi owns it
            self.h = _borrowed
        else:
            h = C.c_void_p()
            rc = self._lib.jpt_create(device, C.byref(h))
            if rc != capi.OK:
                msg = self._lib.jpt_last_error(None)
                raise capi.JptError("jpt_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
            self.h = h
        self.width = self.height = 0
        self._n_probes = 0   # what set_probes last gave the context: sizes read_probes / read_probe_sh
        self._n_cubes = 0    # likewise set_reflection_probes: sizes read_reflection_probes / read_reflection
        self._keep = []
        if self._owned:
            _live_contexts.add(self)

    def close(self):
        if getattr(self, "h", None):
            if self._owned:
                self._lib.jpt_destroy(self.h)
            self.h = None

    def last_error(self) -> str:
        msg = self._lib.jpt_last_error(self.h)
        return msg.decode() if msg else ""

    def share_scene_from(self, other: "Context"):
        """jpt_scene_share: the committed scene of `other` becomes this context's scene too (no builder runs)."""
        self._ck(self._lib.jpt_scene_share(self.h, other.h), "jpt_scene_share")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        capi.check(self.h, rc, what)

    # ---- scene
    def upload_reference_layout(self, tri_geom, tri_data, materials, bvh_nodes, instances, tlas_nodes, textures=None,
                                as_given: bool = False):
        """Route (i).  Default: the kernels walk the native tree built over the uploaded triangles, with reach records
        from the uploaded leaf / TLAS-leaf boxes.  as_given=True: the uploaded trees are walked node for node (audits)."""
        self._ck(self._lib.jpt_set_upload_mode(self.h, capi.UPLOAD_WALK_AS_GIVEN if as_given else capi.UPLOAD_NATIVE_TREE),
                 "jpt_set_upload_mode")
        arrs = [np.ascontiguousarray(a) for a in (tri_geom, tri_data, materials, bvh_nodes, instances, tlas_nodes)]
        tex = None if textures is None else np.ascontiguousarray(textures, dtype=np.uint8)
        self._ck(self._lib.jpt_scene_upload_reference_layout(
            self.h, _ptr(arrs[0]), len(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), len(arrs[2]), _ptr(arrs[3]), len(arrs[3]),
            _ptr(arrs[4]), len(arrs[4]), _ptr(arrs[5]), len(arrs[5]), _ptr(tex),
            0 if tex is None else tex.shape[1], 0 if tex is None else tex.shape[0]), "jpt_scene_upload_reference_layout")

    def set_memory_policy(self, renders_in_flight: int = 0, workspace_budget_bytes: int = 0):
        """Cap on the device memory spent on renders in flight: 1..8 workspaces (0: the library's rule -- 4, or 6 where six slot streams run side by side) and the most bytes
        one workspace may take (0: 24 GiB) -- jpt_set_memory_policy."""
        self._ck(self._lib.jpt_set_memory_policy(self.h, renders_in_flight, workspace_budget_bytes), "jpt_set_memory_policy")

    def workspace_bytes(self) -> int:
        n = C.c_uint64(0)
        self._ck(self._lib.jpt_get_workspace_bytes(self.h, C.byref(n)), "jpt_get_workspace_bytes")
        return int(n.value)

    def set_stream_priority(self, priority: int):
        """capi.STREAM_PRIORITY_*: the priority level of the streams queued renders run on (jpt_set_stream_priority)."""
        self._ck(self._lib.jpt_set_stream_priority(self.h, priority), "jpt_set_stream_priority")

    def renders_in_flight(self) -> int:
        """the pipeline slots the last queued render was dealt among: 4, or 6 where six slot streams run side by side (0 before the first)"""
        return int(self._lib.jpt_renders_in_flight(self.h)) if hasattr(self._lib, "jpt_renders_in_flight") else 0

    def set_debug_steps(self, enable: bool):
        """main.glsl's DEBUG_STEPS build: the image is the primary ray's triangle-test count / 256 (jpt_set_debug_steps)."""
        self._ck(self._lib.jpt_set_debug_steps(self.h, 1 if enable else 0), "jpt_set_debug_steps")

    def tree_kind(self) -> int:
        """capi.TREE_*: which tree the kernels walk for the current scene."""
        k = self._lib.jpt_scene_tree_kind(self.h)
        if k < 0:
            self._ck(k, "jpt_scene_tree_kind")
        return k

    def ties_exact(self):
        """(bool, why): are exact distance ties decided as the reference decides them (jpt_scene_ties_exact)?"""
        why = C.c_char_p()
        rc = self._lib.jpt_scene_ties_exact(self.h, C.byref(why))
        if rc < 0:
            self._ck(rc, "jpt_scene_ties_exact")
        return bool(rc), (why.value.decode() if why.value else "")

    def upload_note(self) -> str:
        msg = self._lib.jpt_scene_upload_note(self.h)
        return msg.decode() if msg else ""

    def build_scene(self, scene: scenes.Scene, builder: int = capi.BUILD_SAH):
        L = self._lib
        self._ck(L.jpt_scene_begin(self.h), "jpt_scene_begin")
        ids = []
        for mesh in scene.meshes:
            arr = (capi.Surface * len(mesh.surfaces))()
            for i, s in enumerate(mesh.surfaces):
                arr[i].vertices, arr[i].normals, arr[i].uvs, arr[i].indices = map(_ptr, (s.vertices, s.normals, s.uvs, s.indices))
                arr[i].n_vertices, arr[i].n_indices = len(s.vertices), len(s.indices)
            mid = C.c_uint32()
            self._ck(L.jpt_scene_add_mesh(self.h, arr, len(mesh.surfaces), C.byref(mid)), "jpt_scene_add_mesh")
            ids.append(mid.value)
        for inst in scene.instances:
            t = np.ascontiguousarray(inst.transform, dtype=np.float32)
            m = np.ascontiguousarray(inst.material_ids, dtype=np.int32)
            self._ck(L.jpt_scene_add_instance(self.h, ids[inst.mesh], _ptr(t), _ptr(m), len(m)), "jpt_scene_add_instance")
        mats = np.ascontiguousarray(scene.materials, dtype=wire.MATERIAL)
        self._ck(L.jpt_scene_set_materials(self.h, _ptr(mats), len(mats)), "jpt_scene_set_materials")
        if scene.textures is not None:
            tex = np.ascontiguousarray(scene.textures, dtype=np.uint8)
            self._ck(L.jpt_scene_set_textures(self.h, _ptr(tex), tex.shape[1], tex.shape[0]), "jpt_scene_set_textures")
        self._ck(L.jpt_scene_commit(self.h, builder), "jpt_scene_commit")

    # ---- moving instances (no full rebuild: BLASes stay on the device)
    def set_instance_transform(self, instance: int, transform12):
        t = np.ascontiguousarray(transform12, dtype=np.float32).reshape(12)
        self._ck(self._lib.jpt_scene_set_instance_transform(self.h, instance, _ptr(t)), "jpt_scene_set_instance_transform")

    def update_tlas(self):
        self._ck(self._lib.jpt_scene_update_tlas(self.h), "jpt_scene_update_tlas")

    def refit_tlas(self, transforms12):
        """All instance transforms at once, instance records + TLAS boxes recomputed on the device (no host rebuild,
        no synchronisation); transforms12: [n_instances, 12] float32."""
        t = np.ascontiguousarray(transforms12, dtype=np.float32).reshape(-1, 12)
        self._ck(self._lib.jpt_scene_refit_tlas(self.h, _ptr(t), t.shape[0]), "jpt_scene_refit_tlas")

    def rebuild_tlas(self, transforms12):
        """refit_tlas with a new topology (jpt_scene_rebuild_tlas): the instances are sorted along a Morton curve on the device and a
        fixed four-way tree over that order replaces the TLAS records; no host rebuild, no synchronisation."""
        t = np.ascontiguousarray(transforms12, dtype=np.float32).reshape(-1, 12)
        self._ck(self._lib.jpt_scene_rebuild_tlas(self.h, _ptr(t), t.shape[0]), "jpt_scene_rebuild_tlas")

    debug_tlas_order = staticmethod(debug_tlas_order)
    debug_tlas_template = staticmethod(debug_tlas_template)

    def debug_tlas_records(self, n_instances: int):
        """The TLAS records new renders read (jpt_debug_tlas_records): dict with `root`, `nodes4` (uint8 [n, 128]), `nodesq` (uint8
        [n, 64]), child references counted from the first record, and the world boxes `lo`, `hi` (float32 [n_instances, 3]) of the scene's n_instances
        instance records."""
        L = self._lib
        n, root = C.c_uint32(), C.c_int32()
        self._ck(L.jpt_debug_tlas_records(self.h, None, None, 0, C.byref(n), C.byref(root), None, None), "jpt_debug_tlas_records")
        nodes4, nodesq = np.zeros((n.value, 128), np.uint8), np.zeros((n.value, 64), np.uint8)
        lo, hi = np.zeros((n_instances, 3), np.float32), np.zeros((n_instances, 3), np.float32)
        self._ck(L.jpt_debug_tlas_records(self.h, _ptr(nodes4), _ptr(nodesq), n.value, C.byref(n), C.byref(root), _ptr(lo), _ptr(hi)),
                 "jpt_debug_tlas_records")
        return dict(root=int(root.value), nodes4=nodes4, nodesq=nodesq, lo=lo, hi=hi)

    def update_reference_tlas(self, instances, tlas_nodes):
        a, b = np.ascontiguousarray(instances), np.ascontiguousarray(tlas_nodes)
        self._ck(self._lib.jpt_scene_update_reference_tlas(self.h, _ptr(a), len(a), _ptr(b), len(b)), "jpt_scene_update_reference_tlas")

    def update_mesh(self, mesh_id: int, mesh: scenes.Mesh, with_normals: bool = True):
        """New vertex positions (and normals, unless with_normals=False) for mesh `mesh_id` of a JPT_BUILD_SAH_WATERTIGHT
        commit: same surfaces, vertex counts and index arrays as at commit.  Triangle records and BLAS boxes are refitted on
        the device (jpt_scene_update_mesh); no host rebuild, no synchronisation."""
        arr = _update_surfaces(mesh, with_normals)
        self._ck(self._lib.jpt_scene_update_mesh(self.h, mesh_id, arr, len(mesh.surfaces)), "jpt_scene_update_mesh")

    def rebuild_mesh(self, mesh_id: int, mesh: scenes.Mesh, with_normals: bool = True):
        """update_mesh with a new BLAS topology (jpt_scene_rebuild_mesh): the mesh's triangles are sorted along a Morton curve on the
        device and a fixed four-way tree over that order, in a region of its own, replaces the mesh's records; later update_mesh /
        pose_mesh calls refit over it.  The mesh's first rebuild may wait for the queued renders; no later one does."""
        arr = _update_surfaces(mesh, with_normals)
        self._ck(self._lib.jpt_scene_rebuild_mesh(self.h, mesh_id, arr, len(mesh.surfaces)), "jpt_scene_rebuild_mesh")

    debug_mesh_order = staticmethod(debug_mesh_order)

    def set_mesh_rig(self, mesh_id: int, bind: scenes.Mesh, rigs, influences: int, n_blend_shapes: int, with_normals: bool = True):
        """The rig of a committed mesh, kept on the device (jpt_scene_set_mesh_rig): `bind` is the bind-pose mesh (same surfaces, vertex
        counts and index arrays as committed; with_normals False: the committed normals stay), `rigs` one SurfaceRig per surface."""
        arr, rarr = _update_surfaces(bind, with_normals), _rig_surfaces(rigs)
        self._ck(self._lib.jpt_scene_set_mesh_rig(self.h, mesh_id, arr, rarr, len(bind.surfaces), influences, n_blend_shapes), "jpt_scene_set_mesh_rig")

    def pose_mesh(self, mesh_id: int, bone_transforms12=None, blend_weights=None, rebuild: bool = False):
        """One pose of a rigged mesh (jpt_scene_pose_mesh): float32 [n_bones, 12] bone transforms (bone pose x inverse bind, transform12
        layout) and one weight per blend shape; the vertices are computed and the mesh refitted on the device, no synchronisation.
        rebuild: with a new BLAS topology over the posed vertices (jpt_scene_pose_mesh_rebuild), as rebuild_mesh."""
        b, nb, w, nw = _pose_arrays(bone_transforms12, blend_weights)
        name = "jpt_scene_pose_mesh_rebuild" if rebuild else "jpt_scene_pose_mesh"
        self._ck(getattr(self._lib, name)(self.h, mesh_id, _ptr(b), nb, _ptr(w), nw), name)

    def clear_mesh_rig(self, mesh_id: int):
        self._ck(self._lib.jpt_scene_clear_mesh_rig(self.h, mesh_id), "jpt_scene_clear_mesh_rig")

    debug_skin = staticmethod(debug_skin)

    def debug_mesh_records(self, mesh_id: int):
        """The device's records of one mesh (jpt_debug_mesh_records): dict with the info words and, when the device holds a
        tree for the mesh, `nodes4` (uint8 [n, 128]), `nodesq` (uint8 [n, 64]), `tris` (uint8 [t, 48]), `shade` (uint8 [t, 64])."""
        info = (C.c_int32 * 6)()
        L = self._lib
        self._ck(L.jpt_debug_mesh_records(self.h, mesh_id, None, None, 0, None, None, 0, info), "jpt_debug_mesh_records")
        out = dict(has_tree=bool(info[0]), root=int(info[1]), first_record=int(info[2]), n_records=int(info[3]),
                   first_tri=int(info[4]), n_tris=int(info[5]))
        if not out["has_tree"]:
            return out
        n, t = out["n_records"], out["n_tris"]
        nodes4, nodesq = np.zeros((n, 128), np.uint8), np.zeros((n, 64), np.uint8)
        tris, shade = np.zeros((t, 48), np.uint8), np.zeros((t, 64), np.uint8)
        self._ck(L.jpt_debug_mesh_records(self.h, mesh_id, _ptr(nodes4), _ptr(nodesq), n, _ptr(tris), _ptr(shade), t, info),
                 "jpt_debug_mesh_records")
        out.update(nodes4=nodes4, nodesq=nodesq, tris=tris, shade=shade)
        return out

    def reference_buffer(self, which: int, dtype) -> np.ndarray:
        n = C.c_size_t()
        self._ck(self._lib.jpt_scene_get_reference_buffer(self.h, which, None, 0, C.byref(n)), "jpt_scene_get_reference_buffer")
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        self._ck(self._lib.jpt_scene_get_reference_buffer(self.h, which, _ptr(out), out.nbytes, C.byref(n)),
                 "jpt_scene_get_reference_buffer")
        return out

    # ---- per-render state
    def set_params(self, width, height, max_bounces=4, accum_mode=capi.ACCUM_REF_LDR8, sampler_mode=0):
        self._ck(self._lib.jpt_set_params(self.h, width, height, max_bounces, accum_mode, sampler_mode), "jpt_set_params")
        self.width, self.height = width, height

    def set_environment(self, rgb):
        """jpt_set_environment: light the scene with an HDR environment map, float32 [height, width, 3] (equirectangular, row 0
        the +y pole; hdrio.load_hdr reads one), or None for main.glsl's sky gradient.  Waits for the renders already queued."""
        a, w, h = _env_map(rgb)
        self._ck(self._lib.jpt_set_environment(self.h, None if a is None else _ptr(a), w, h), "jpt_set_environment")

    def set_sky(self, params=None, width=2048, height=1024, samples=4):
        """jpt_set_sky: make the environment map of a procedural sky on the device -- `params` a capi.SkyParams (capi.sky_params builds
        one; None: Godot's defaults), samples x samples subsamples per texel.  With a map of this size already present the kernel is
        queued behind the renders already queued and the call does not wait (unless capi.ENV_SAMPLING_MIS is on: the tables' rebuild
        waits); otherwise it waits and allocates like set_environment."""
        self._ck(self._lib.jpt_set_sky(self.h, _sky_ref(params), int(width), int(height), int(samples)), "jpt_set_sky")

    def read_environment(self) -> np.ndarray:
        """jpt_read_environment_f32: the map the context holds (from set_environment or set_sky), float32 [height, width, 3]; waits for
        the context's stream.  Without a map: JptError (E_STATE)."""
        w, h = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.jpt_read_environment_f32(self.h, None, C.byref(w), C.byref(h)), "jpt_read_environment_f32")
        out = np.zeros((h.value, w.value, 3), np.float32)
        self._ck(self._lib.jpt_read_environment_f32(self.h, _ptr(out), C.byref(w), C.byref(h)), "jpt_read_environment_f32")
        return out

    def set_environment_params(self, rotation=None, intensity: float = 1.0):
        """jpt_set_environment_params: row-major 3x3 world -> map rotation (None: identity) and intensity, for later renders."""
        r = _env_rotation(rotation)
        self._ck(self._lib.jpt_set_environment_params(self.h, None if r is None else _ptr(r), float(intensity)),
                 "jpt_set_environment_params")

    def set_environment_sampling(self, mode):
        """jpt_set_environment_sampling: capi.ENV_SAMPLING_BRDF (default) or capi.ENV_SAMPLING_MIS (importance sampling of the map
        with shadow rays, combined with BRDF sampling by the power heuristic), for later renders."""
        self._ck(self._lib.jpt_set_environment_sampling(self.h, int(mode)), "jpt_set_environment_sampling")

    def set_light_sampling(self, mode):
        """jpt_set_light_sampling: capi.LIGHT_SAMPLING_BRDF (default) or capi.LIGHT_SAMPLING_MIS (emissive triangles sampled with
        shadow rays, combined with BRDF sampling by the power heuristic), for later renders."""
        self._ck(self._lib.jpt_set_light_sampling(self.h, int(mode)), "jpt_set_light_sampling")

    def set_lens(self, aperture_radius, focus_distance):
        """jpt_set_lens: a thin lens of `aperture_radius` world units focused `focus_distance` along the camera's forward axis; radius
        0 (the default) is the pinhole.  The context's, like the sampling modes; each render takes it by value."""
        self._ck(self._lib.jpt_set_lens(self.h, float(aperture_radius), float(focus_distance)), "jpt_set_lens")

    def set_camera_model(self, model):
        """jpt_set_camera_model: capi.CAMERA_PINHOLE (default), capi.CAMERA_PROJECTIVE (near-plane point towards far-plane point: exact
        for an orthographic matrix) or capi.CAMERA_EQUIRECT (the full sphere, in the environment map's layout).  The context's, like the
        lens; each render takes it by value."""
        self._ck(self._lib.jpt_set_camera_model(self.h, int(model)), "jpt_set_camera_model")

    # ---- lightmap baking (jpt_set_bake_texels, jpt_bake_begin / jpt_bake_add_surface)
    def set_bake_texels(self, position4, normal4):
        """jpt_set_bake_texels: float32 [height, width, 4] each -- (world position, w) and (world normal, w); a texel is valid when its
        normal's xyz is not zero.  While images are present every render is a bake render (one path per texel, cosine-distributed
        about the normal).  (None, None) frees them.  Waits for the renders already queued."""
        if position4 is None and normal4 is None:
            self._ck(self._lib.jpt_set_bake_texels(self.h, None, None, 0, 0), "jpt_set_bake_texels")
            self._bake_size = None
            return
        p, n = _bake_images(position4, normal4)
        self._ck(self._lib.jpt_set_bake_texels(self.h, _ptr(p), _ptr(n), p.shape[1], p.shape[0]), "jpt_set_bake_texels")
        self._bake_size = (p.shape[1], p.shape[0])

    def bake_begin(self, width, height):
        """jpt_bake_begin: width x height images, every texel invalid, for bake_add_surface to fill"""
        self._ck(self._lib.jpt_bake_begin(self.h, int(width), int(height)), "jpt_bake_begin")
        self._bake_size = (int(width), int(height))

    def bake_add_surface(self, surface, uv2, transform12):
        """jpt_bake_add_surface: rasterise one scenes.Surface's UV2 triangles (uv2 [n_vertices, 2]) through the instance's transform12
        into the images, on the device; the lowest triangle index wins a texel, a later call replaces what it covers"""
        s, uv, t12 = _bake_surface(surface, uv2, transform12)
        self._ck(self._lib.jpt_bake_add_surface(self.h, C.byref(s), _ptr(uv), _ptr(t12)), "jpt_bake_add_surface")

    def read_bake_texels(self):
        """jpt_read_bake_texels: (position4, normal4) float32 [height, width, 4], the size the images were made with by this object"""
        width, height = getattr(self, "_bake_size", None) or (1, 1)   # (without images the call answers E_STATE before it writes)
        p, n = np.zeros((height, width, 4), np.float32), np.zeros((height, width, 4), np.float32)
        self._ck(self._lib.jpt_read_bake_texels(self.h, _ptr(p), _ptr(n)), "jpt_read_bake_texels")
        return p, n

    # ---- finishing a baked lightmap (jpt_bake_finish)
    def set_bake_finish_params(self, params: Optional[capi.BakeFinishParams] = None, **fields):
        """jpt_set_bake_finish_params: a capi.BakeFinishParams, or its fields by name (passes, normal_power_log2, dilate,
        sigma_distance, sigma_plane, sigma_color; the rest at the defaults); nothing: the defaults"""
        if params is None and fields:
            params = capi.BakeFinishParams(**fields)
        self._ck(self._lib.jpt_set_bake_finish_params(self.h, None if params is None else C.byref(params)), "jpt_set_bake_finish_params")

    def bake_finish(self):
        """jpt_bake_finish: queue the chart-aware filter passes and the dilation over the accumulation of the bake renders queued so
        far, guided by the texel images; the accumulation itself is not touched"""
        self._ck(self._lib.jpt_bake_finish(self.h), "jpt_bake_finish")

    def read_lightmap(self) -> np.ndarray:
        """jpt_read_lightmap_f32: (r, g, b, coverage) float32 [height, width, 4]; coverage 1 a texel of a chart, 0.5 a dilated one, 0
        an untouched one"""
        out = np.zeros((max(self.height, 1), max(self.width, 1), 4), dtype=np.float32)   # (without a size the call answers before it writes)
        self._ck(self._lib.jpt_read_lightmap_f32(self.h, _ptr(out)), "jpt_read_lightmap_f32")
        return out

    # ---- directional lightmaps (jpt_set_bake_directional)
    def set_bake_directional(self, enable=True):
        """jpt_set_bake_directional: bake renders also keep the three first moments of the incoming light per texel, sum of (frame's
        value * the world x, y, z of the direction its path left the surface in).  A change of the value resets the accumulation."""
        self._ck(self._lib.jpt_set_bake_directional(self.h, 1 if enable else 0), "jpt_set_bake_directional")

    def read_bake_directional(self) -> np.ndarray:
        """jpt_read_bake_directional_f32: the raw sums, float32 [3, local rows, width, 4] -- plane k holds (M_k.r, M_k.g, M_k.b, 0), k =
        world x, y, z, over the context's own rows in their local order.  Divide by the frame count for the mean."""
        out = np.zeros((3, max(self.local_rows(), 1), max(self.width, 1), 4), dtype=np.float32)   # (without a size the call answers before it writes)
        self._ck(self._lib.jpt_read_bake_directional_f32(self.h, _ptr(out)), "jpt_read_bake_directional_f32")
        return out

    def device_bake_directional(self, finished=False):
        """jpt_device_bake_directional: (device pointer or None, bytes) of the raw or the finished planes"""
        n = C.c_size_t(0)
        p = self._lib.jpt_device_bake_directional(self.h, 1 if finished else 0, C.byref(n))
        return p, int(n.value)

    def bake_finish_directional(self):
        """jpt_bake_finish_directional: jpt_bake_finish's filter and dilation over each of the three planes, with the same frame count,
        images and parameters; the planes themselves and the L0 lightmap are not touched"""
        self._ck(self._lib.jpt_bake_finish_directional(self.h), "jpt_bake_finish_directional")

    def read_lightmap_directional(self) -> np.ndarray:
        """jpt_read_lightmap_directional_f32: float32 [3, height, width, 4] -- plane k holds (the filtered mean of M_k, coverage)"""
        out = np.zeros((3, max(self.height, 1), max(self.width, 1), 4), dtype=np.float32)
        self._ck(self._lib.jpt_read_lightmap_directional_f32(self.h, _ptr(out)), "jpt_read_lightmap_directional_f32")
        return out

    # ---- light probes (jpt_set_probes, jpt_probe_project)
    def set_probes(self, positions, tile_w=0, tile_h=0, probes_per_row=0):
        """jpt_set_probes: float32 [n, 3] world positions; while probes are present every render is a probe render, one tile_w x tile_h
        sphere tile per probe, probes_per_row to a row (probe_image_size: the size for set_params).  None frees them.  Waits for the
        renders already queued."""
        if positions is None:
            self._ck(self._lib.jpt_set_probes(self.h, None, 0, 0, 0, 0), "jpt_set_probes")
            self._n_probes = 0
            return
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        self._ck(self._lib.jpt_set_probes(self.h, _ptr(pos), len(pos), int(tile_w), int(tile_h), int(probes_per_row)), "jpt_set_probes")
        self._n_probes = len(pos)

    def probe_image_size(self):
        """jpt_get_probe_image_size: (width, height) of the image the context's probes make"""
        w, h = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.jpt_get_probe_image_size(self.h, C.byref(w), C.byref(h)), "jpt_get_probe_image_size")
        return w.value, h.value

    def read_probes(self, n_probes=None):
        """jpt_read_probes: the positions the context holds, float32 [n, 3].  n_probes: the count the context holds, by default the one
        this object's set_probes gave it (give it when the probes were set through the handle: the call writes that many)"""
        n = self._n_probes if n_probes is None else int(n_probes)
        out = np.zeros((max(n, 1), 3), np.float32)   # (without probes the call answers E_STATE before it writes)
        self._ck(self._lib.jpt_read_probes(self.h, _ptr(out)), "jpt_read_probes")
        return out

    def probe_project(self, flags=capi.PROBE_RADIANCE):
        """jpt_probe_project: queue the projection of every probe's tile of the accumulation to nine L2 SH coefficients per channel
        (capi.PROBE_IRRADIANCE: convolved with the cosine lobe); the accumulation itself is not touched"""
        self._ck(self._lib.jpt_probe_project(self.h, int(flags)), "jpt_probe_project")

    def read_probe_sh(self, n_probes=None) -> np.ndarray:
        """jpt_read_probe_sh_f32: float32 [n_probes, 9, 4], (r, g, b, 0) per coefficient; n_probes as in read_probes"""
        n = self._n_probes if n_probes is None else int(n_probes)
        out = np.zeros((max(n, 1), 9, 4), np.float32)
        self._ck(self._lib.jpt_read_probe_sh_f32(self.h, _ptr(out)), "jpt_read_probe_sh_f32")
        return out

    # ---- reflection probes (jpt_set_reflection_probes, jpt_reflection_prefilter)
    def set_reflection_probes(self, positions, face_size=0, probes_per_row=0):
        """jpt_set_reflection_probes: float32 [n, 3] world positions; while they are present every render is a cube render, one strip of
        six face_size x face_size faces per probe, probes_per_row to a row (reflection_image_size: the size for set_params).  None
        frees them.  Waits for the renders already queued."""
        if positions is None:
            self._ck(self._lib.jpt_set_reflection_probes(self.h, None, 0, 0, 0), "jpt_set_reflection_probes")
            self._n_cubes = 0
            return
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        self._ck(self._lib.jpt_set_reflection_probes(self.h, _ptr(pos), len(pos), int(face_size), int(probes_per_row)), "jpt_set_reflection_probes")
        self._n_cubes = len(pos)

    def reflection_image_size(self):
        """jpt_get_reflection_image_size: (width, height) of the image the context's reflection probes make"""
        w, h = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.jpt_get_reflection_image_size(self.h, C.byref(w), C.byref(h)), "jpt_get_reflection_image_size")
        return w.value, h.value

    def read_reflection_probes(self, n_probes=None):
        """jpt_read_reflection_probes: the positions the context holds, float32 [n, 3]; n_probes as in read_probes"""
        n = self._n_cubes if n_probes is None else int(n_probes)
        out = np.zeros((max(n, 1), 3), np.float32)   # (without probes the call answers E_STATE before it writes)
        self._ck(self._lib.jpt_read_reflection_probes(self.h, _ptr(out)), "jpt_read_reflection_probes")
        return out

    def set_reflection_params(self, params=None, **fields):
        """jpt_set_reflection_params: a capi.ReflectionParams, or its fields by name (n_levels, samples); nothing: the defaults"""
        if params is None and fields:
            params = capi.ReflectionParams(**fields)
        self._ck(self._lib.jpt_set_reflection_params(self.h, None if params is None else C.byref(params)), "jpt_set_reflection_params")

    def reflection_prefilter(self):
        """jpt_reflection_prefilter: queue the GGX-prefiltered mip chain of every probe's strip of the accumulation; the accumulation
        itself is not touched"""
        self._ck(self._lib.jpt_reflection_prefilter(self.h), "jpt_reflection_prefilter")

    def reflection_chain_size(self, level):
        """jpt_get_reflection_chain_size: (face size of the level, where it starts in the chain in texels)"""
        s, off = C.c_int32(0), C.c_uint64(0)
        self._ck(self._lib.jpt_get_reflection_chain_size(self.h, int(level), C.byref(s), C.byref(off)), "jpt_get_reflection_chain_size")
        return s.value, off.value

    def read_reflection(self, level, n_probes=None) -> np.ndarray:
        """jpt_read_reflection_f32: one level of the chain, float32 [n_probes, 6, s, s, 4], (r, g, b, 1) per texel"""
        n = self._n_cubes if n_probes is None else int(n_probes)
        s, _ = self.reflection_chain_size(level)
        out = np.zeros((max(n, 1), 6, s, s, 4), np.float32)
        self._ck(self._lib.jpt_read_reflection_f32(self.h, int(level), _ptr(out)), "jpt_read_reflection_f32")
        return out

    def reflection_timing(self):
        """jpt_get_reflection_timing: (source chain ms, prefilter ms) of the last reflection_prefilter under set_kernel_timing"""
        a, b = C.c_float(0), C.c_float(0)
        self._ck(self._lib.jpt_get_reflection_timing(self.h, C.byref(a), C.byref(b)), "jpt_get_reflection_timing")
        return a.value, b.value

    def set_material_extensions(self, flags):
        """jpt_set_material_extensions: capi.MATERIAL_EXT_NONE (default) or capi.MATERIAL_EXT_TRANSMISSION (padding[0:2] of every
        material are its transmission and ior), for later renders."""
        self._ck(self._lib.jpt_set_material_extensions(self.h, int(flags)), "jpt_set_material_extensions")

    def debug_light_tables(self):
        """jpt_debug_light_tables: (pairs [n, 2] uint32, tri [n, 3, 4] float32, cdf [n], marg [blocks + 1]) of the emitter tables"""
        n = np.zeros(2, np.uint32)
        self._ck(self._lib.jpt_debug_light_tables(self.h, 0, _ptr(n), None, None, None, None), "jpt_debug_light_tables")
        pairs = np.zeros((int(n[0]), 2), np.uint32)
        tri = np.zeros((int(n[0]), 3, 4), np.float32)
        cdf = np.zeros(int(n[0]), np.float32)
        marg = np.zeros(int(n[1]) + 1, np.float32)
        self._ck(self._lib.jpt_debug_light_tables(self.h, int(n[0]), _ptr(n), _ptr(pairs), _ptr(tri), _ptr(cdf), _ptr(marg)),
                 "jpt_debug_light_tables")
        return pairs, tri, cdf, marg

    def debug_light_sample(self, xi4, origins):
        """jpt_debug_light_sample: (points [n, 3], dirs [n, 3], pdf [n]) for randoms xi4 [n, 4] seen from origins [n, 3]"""
        xi4 = np.ascontiguousarray(xi4, np.float32).reshape(-1, 4)
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        n = len(xi4)
        pts, dirs, pdf = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        self._ck(self._lib.jpt_debug_light_sample(self.h, _ptr(xi4), _ptr(o), n, _ptr(pts), _ptr(dirs), _ptr(pdf)), "jpt_debug_light_sample")
        return pts, dirs, pdf

    def debug_light_pdf(self, inst, tri, points, origins, dirs):
        """jpt_debug_light_pdf: p_L [n] of hit points on (instance, triangle) seen from origins along dirs"""
        inst = np.ascontiguousarray(inst, np.uint32).reshape(-1)
        tri = np.ascontiguousarray(tri, np.uint32).reshape(-1)
        p, o, d = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (points, origins, dirs))
        pdf = np.zeros(len(inst), np.float32)
        self._ck(self._lib.jpt_debug_light_pdf(self.h, _ptr(inst), _ptr(tri), _ptr(p), _ptr(o), _ptr(d), len(inst), _ptr(pdf)),
                 "jpt_debug_light_pdf")
        return pdf

    def set_kernel(self, variant):
        self._ck(self._lib.jpt_set_kernel(self.h, variant), "jpt_set_kernel")

    def set_kernel_timing(self, enable: bool):
        self._ck(self._lib.jpt_set_kernel_timing(self.h, 1 if enable else 0), "jpt_set_kernel_timing")

    def set_partition(self, rank, world):
        self._ck(self._lib.jpt_set_partition(self.h, rank, world), "jpt_set_partition")

    def set_camera(self, camera_block: np.ndarray):
        cam = np.ascontiguousarray(camera_block, dtype=wire.CAMERA).reshape(1)
        self._ck(self._lib.jpt_set_camera(self.h, _ptr(cam)), "jpt_set_camera")

    def set_stream(self, hip_stream: Optional[int]):
        self._ck(self._lib.jpt_set_stream(self.h, hip_stream), "jpt_set_stream")

    def get_stream(self) -> int:
        out = C.c_void_p()
        self._ck(self._lib.jpt_get_stream(self.h, C.byref(out)), "jpt_get_stream")
        return int(out.value or 0)

    def render(self, n_frames=1, first_frame_index=1, counted=False, asynchronous=False):
        fn = self._lib.jpt_render_counted if counted else (self._lib.jpt_render_async if asynchronous else self._lib.jpt_render)
        self._ck(fn(self.h, n_frames, first_frame_index), "jpt_render")

    def sync(self):
        self._ck(self._lib.jpt_sync(self.h), "jpt_sync")

    def accum_reset(self):
        self._ck(self._lib.jpt_accum_reset(self.h), "jpt_accum_reset")

    def set_denoising_mode(self, mode: int):
        self._ck(self._lib.jpt_set_denoising_mode(self.h, mode), "jpt_set_denoising_mode")

    def set_temporal_params(self, params: np.ndarray):
        p = np.ascontiguousarray(params, dtype=wire.TEMPORAL_PARAMS).reshape(1)
        self._ck(self._lib.jpt_set_temporal_params(self.h, _ptr(p)), "jpt_set_temporal_params")

    def set_outputs(self, depth: bool = True):
        """jpt_set_outputs: the r32f depth image (main.glsl:435) has one reader, TemporalReprojection; off saves its passes"""
        self._ck(self._lib.jpt_set_outputs(self.h, capi.OUTPUT_DEPTH if depth else 0), "jpt_set_outputs")

    # ---- outputs
    def read_ldr(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._ck(self._lib.jpt_read_ldr_rgba8(self.h, _ptr(out)), "jpt_read_ldr_rgba8")
        return out

    def readback_ldr_begin(self):
        self._ck(self._lib.jpt_readback_ldr_begin(self.h), "jpt_readback_ldr_begin")

    def readback_ldr_end(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._ck(self._lib.jpt_readback_ldr_end(self.h, _ptr(out)), "jpt_readback_ldr_end")
        return out

    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._ck(self._lib.jpt_read_accum_f32(self.h, _ptr(out)), "jpt_read_accum_f32")
        return out

    def read_depth(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), dtype=np.float32)
        self._ck(self._lib.jpt_read_depth_f32(self.h, _ptr(out)), "jpt_read_depth_f32")
        return out

    # ---- spatial denoising (jpt_denoise)
    def set_denoise_params(self, params: Optional[capi.DenoiseParams] = None, **fields):
        """jpt_set_denoise_params: a capi.DenoiseParams, or its fields by name (passes, normal_power_log2, sigma_plane,
        sigma_color; the rest at the defaults); nothing: the defaults"""
        if params is None and fields:
            params = capi.DenoiseParams(**fields)
        self._ck(self._lib.jpt_set_denoise_params(self.h, None if params is None else C.byref(params)), "jpt_set_denoise_params")

    def denoise(self):
        """jpt_denoise: queue the guide pass and the filter passes over the accumulation as it is after the renders queued so
        far; the accumulation itself is not touched"""
        self._ck(self._lib.jpt_denoise(self.h), "jpt_denoise")

    def read_denoised(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._ck(self._lib.jpt_read_denoised_f32(self.h, _ptr(out)), "jpt_read_denoised_f32")
        return out

    def read_denoised_ldr(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._ck(self._lib.jpt_read_denoised_rgba8(self.h, _ptr(out)), "jpt_read_denoised_rgba8")
        return out

    def set_denoise_variance(self, params: Optional[capi.DenoiseVarianceParams] = None, **fields):
        """jpt_set_denoise_variance: a capi.DenoiseVarianceParams, or its fields by name (enable, sigma_variance, variance_floor; the
        rest at the defaults); nothing: the defaults, the guidance off.  With it on, denoise() measures colour differences against
        the variance plane of set_variance() and refuses without one of at least two frames."""
        if params is None and fields:
            params = capi.DenoiseVarianceParams(**fields)
        self._ck(self._lib.jpt_set_denoise_variance(self.h, None if params is None else C.byref(params)), "jpt_set_denoise_variance")

    def read_denoised_variance(self) -> np.ndarray:
        """jpt_read_denoised_variance_f32: float32 [height, width], the variance of the demodulated mean a guided denoise() leaves
        after its last pass"""
        out = np.zeros((self.height, self.width), dtype=np.float32)
        self._ck(self._lib.jpt_read_denoised_variance_f32(self.h, _ptr(out)), "jpt_read_denoised_variance_f32")
        return out

    def set_denoise_history(self, params: Optional[capi.DenoiseHistoryParams] = None, **fields):
        """jpt_set_denoise_history: a capi.DenoiseHistoryParams, or its fields by name (enable, max_history, min_history, sigma_plane;
        the rest at the defaults); nothing: the defaults, the history off.  With it on, each denoise() integrates the frames accumulated
        since the last reset into a reprojected per-pixel history and filters that, guided by the history's own variance."""
        if params is None and fields:
            params = capi.DenoiseHistoryParams(**fields)
        self._ck(self._lib.jpt_set_denoise_history(self.h, None if params is None else C.byref(params)), "jpt_set_denoise_history")

    def denoise_history_reset(self):
        """jpt_denoise_history_reset: the next denoise() starts without history"""
        self._ck(self._lib.jpt_denoise_history_reset(self.h), "jpt_denoise_history_reset")

    def read_denoise_history(self):
        """jpt_read_denoise_history_f32: (float32 [height, width, 4] = (m.rgb demodulated, v_0), float32 [height, width] = the history
        length N) of the last denoise() with the history on"""
        iv, length = np.zeros((self.height, self.width, 4), dtype=np.float32), np.zeros((self.height, self.width), dtype=np.float32)
        self._ck(self._lib.jpt_read_denoise_history_f32(self.h, _ptr(iv), _ptr(length)), "jpt_read_denoise_history_f32")
        return iv, length

    # ---- the display transform (jpt_display)
    def set_display_params(self, params: Optional[capi.DisplayParams] = None, **fields):
        """jpt_set_display_params: a capi.DisplayParams, or its fields by name (source, tonemap, transfer, bloom_levels, exposure,
        white, bloom_threshold, bloom_strength; the rest at the defaults); nothing: the defaults"""
        if params is None and fields:
            params = capi.DisplayParams(**fields)
        self._ck(self._lib.jpt_set_display_params(self.h, None if params is None else C.byref(params)), "jpt_set_display_params")

    def display(self):
        """jpt_display: queue exposure, bloom, tone map and transfer over the accumulation as it is after the renders queued so far
        (or over jpt_denoise's image); neither is touched"""
        self._ck(self._lib.jpt_display(self.h), "jpt_display")

    def read_display(self) -> np.ndarray:
        """the tone-mapped image before the transfer, float32 [height, width, 4] = (r, g, b, 1)"""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._ck(self._lib.jpt_read_display_f32(self.h, _ptr(out)), "jpt_read_display_f32")
        return out

    def read_display_ldr(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._ck(self._lib.jpt_read_display_rgba8(self.h, _ptr(out)), "jpt_read_display_rgba8")
        return out

    # ---- encoded outputs (jpt_encode)
    def encode(self, source, fmt, level=0):
        """jpt_encode: queue the packing of one of the context's float4 images (capi.ENCODE_SOURCE_*; `level` for the reflection chain,
        capi.ENCODE_ALL_LEVELS for all of it) into capi.ENCODE_RGBA16F / _RGB9E5 / _RGBE8, in a buffer of its own: a snapshot that
        stays readable until the next encode"""
        self._ck(self._lib.jpt_encode(self.h, int(source), int(level), int(fmt)), "jpt_encode")

    def encoded_info(self) -> dict:
        """jpt_get_encoded_info: source, format, level, width, height, n_texels, bytes of the snapshot"""
        info = capi.EncodedInfo()
        self._ck(self._lib.jpt_get_encoded_info(self.h, C.byref(info)), "jpt_get_encoded_info")
        return info.as_dict()

    def read_encoded(self) -> np.ndarray:
        """jpt_read_encoded: the snapshot -- float16 [n, 4], uint32 [n] or uint8 [n, 4] by its format (capi.encoded_array), n texels in
        the source's own order; blocking"""
        info = self.encoded_info()
        out = capi.encoded_array(info["format"], info["n_texels"])
        self._ck(self._lib.jpt_read_encoded(self.h, _ptr(out), out.nbytes), "jpt_read_encoded")
        return out

    def readback_encoded_begin(self):
        """jpt_readback_encoded_begin: queue the copy of the snapshot to pinned memory"""
        info = self.encoded_info()
        self._ck(self._lib.jpt_readback_encoded_begin(self.h), "jpt_readback_encoded_begin")
        self._enc_pending = (info["format"], info["n_texels"])

    def readback_encoded_end(self) -> np.ndarray:
        """jpt_readback_encoded_end: wait for that copy alone and return it, as read_encoded returns the snapshot it was begun on"""
        fmt, n = getattr(self, "_enc_pending", None) or (capi.ENCODE_RGBE8, 0)
        out = capi.encoded_array(fmt, n)
        self._ck(self._lib.jpt_readback_encoded_end(self.h, _ptr(out), out.nbytes), "jpt_readback_encoded_end")
        self._enc_pending = None
        return out

    def device_encoded(self):
        """jpt_device_encoded: (device pointer, bytes) of the snapshot; (None, 0) before any encode"""
        n = C.c_size_t()
        p = self._lib.jpt_device_encoded(self.h, C.byref(n))
        return p, n.value

    def encode_timing(self) -> float:
        """jpt_get_encode_timing: kernel ms of the last encode under set_kernel_timing"""
        ms = C.c_float(0)
        self._ck(self._lib.jpt_get_encode_timing(self.h, C.byref(ms)), "jpt_get_encode_timing")
        return ms.value

    # ---- metering and auto-exposure (jpt_meter)
    def set_meter_params(self, params: Optional[capi.MeterParams] = None, **fields):
        """jpt_set_meter_params: a capi.MeterParams, or its fields by name (source, mode, low_permille, high_permille, key,
        min_exposure, max_exposure, adapt; the rest at the defaults); nothing: the defaults.  The metering state is kept."""
        if params is None and fields:
            params = capi.MeterParams(**fields)
        self._ck(self._lib.jpt_set_meter_params(self.h, None if params is None else C.byref(params)), "jpt_set_meter_params")

    def meter(self):
        """jpt_meter: queue the luminance histogram of the accumulation as it is after the renders queued so far (or of jpt_denoise's
        image) and its resolve into the exposure state; neither image is touched"""
        self._ck(self._lib.jpt_meter(self.h), "jpt_meter")

    def meter_reset(self):
        """jpt_meter_reset: the next meter() starts from its target instead of adapting"""
        self._ck(self._lib.jpt_meter_reset(self.h), "jpt_meter_reset")

    def read_meter(self, histogram: bool = True):
        """jpt_read_meter: (the capi.MeterResult as a dict, the 256 bins as uint32 or None)"""
        res = capi.MeterResult()
        hist = np.zeros(256, dtype=np.uint32) if histogram else None
        self._ck(self._lib.jpt_read_meter(self.h, C.byref(res), None if hist is None else _ptr(hist)), "jpt_read_meter")
        return res.as_dict(), hist

    def set_auto_exposure(self, enable: bool):
        """jpt_set_auto_exposure: display() multiplies its exposure by the metered one, read on the device"""
        self._ck(self._lib.jpt_set_auto_exposure(self.h, 1 if enable else 0), "jpt_set_auto_exposure")

    # ---- per-pixel noise (jpt_set_variance, jpt_noise_estimate, jpt_render_converge)
    def set_variance(self, enable=True):
        """jpt_set_variance: renders also keep the second central moment of a pixel's frames, (M2.r, M2.g, M2.b, 0) per pixel.  A
        change of the value resets the accumulation."""
        self._ck(self._lib.jpt_set_variance(self.h, 1 if enable else 0), "jpt_set_variance")

    def read_variance(self) -> np.ndarray:
        """jpt_read_variance_f32: float32 [height, width, 4], the context's rows scattered to image rows as read_accum's.  M2 / (n - 1)
        is the sample variance of a frame, M2 / (n (n - 1)) the variance of the mean."""
        out = np.zeros((max(self.height, 1), max(self.width, 1), 4), dtype=np.float32)   # (without a size the call answers before it writes)
        self._ck(self._lib.jpt_read_variance_f32(self.h, _ptr(out)), "jpt_read_variance_f32")
        return out

    def device_variance(self):
        """jpt_device_variance: (device pointer or None, bytes) of the plane"""
        n = C.c_size_t(0)
        p = self._lib.jpt_device_variance(self.h, C.byref(n))
        return p, int(n.value)

    def set_noise_params(self, params: Optional[capi.NoiseParams] = None, **fields):
        """jpt_set_noise_params: a capi.NoiseParams, or its fields by name (threshold, floor, percentile_permille, allowed_permille;
        the rest at the defaults); nothing: the defaults"""
        if params is None and fields:
            params = capi.NoiseParams(**fields)
        self._ck(self._lib.jpt_set_noise_params(self.h, None if params is None else C.byref(params)), "jpt_set_noise_params")

    def noise_estimate(self):
        """jpt_noise_estimate: queue the reduction of the accumulation and the variance plane, as they are after the renders queued so
        far, to the histogram, the tile map and the result; neither plane is touched"""
        self._ck(self._lib.jpt_noise_estimate(self.h), "jpt_noise_estimate")

    def read_noise(self, histogram: bool = True):
        """jpt_read_noise: (the capi.NoiseResult as a dict, the 256 bins as uint32 or None)"""
        res = capi.NoiseResult()
        hist = np.zeros(256, dtype=np.uint32) if histogram else None
        self._ck(self._lib.jpt_read_noise(self.h, C.byref(res), None if hist is None else _ptr(hist)), "jpt_read_noise")
        return res.as_dict(), hist

    def read_noise_tiles(self) -> np.ndarray:
        """jpt_read_noise_tiles_f32: float32 [ceil(height / 8), ceil(width / 8)], the largest relative error of each 8 x 8 tile"""
        out = np.zeros((max(-(-self.height // 8), 1), max(-(-self.width // 8), 1)), dtype=np.float32)
        self._ck(self._lib.jpt_read_noise_tiles_f32(self.h, _ptr(out)), "jpt_read_noise_tiles_f32")
        return out

    def device_noise_tiles(self):
        """jpt_device_noise_tiles: (device pointer or None, bytes) of the tile map"""
        n = C.c_size_t(0)
        p = self._lib.jpt_device_noise_tiles(self.h, C.byref(n))
        return p, int(n.value)

    def render_converge(self, frames_per_step: int, max_frames: int, first_frame_index: int = 0):
        """jpt_render_converge: render frames_per_step frames at a time until the noise estimate says converged or max_frames are
        done -- (frames rendered, the last capi.NoiseResult as a dict)"""
        done = C.c_int32(0)
        res = capi.NoiseResult()
        self._ck(self._lib.jpt_render_converge(self.h, int(frames_per_step), int(max_frames), int(first_frame_index), C.byref(done), C.byref(res)),
                 "jpt_render_converge")
        return int(done.value), res.as_dict()

    def read_guides(self):
        """jpt_read_guides_f32: (position_t, normal, albedo), float32 [height, width, 4] each"""
        g = [np.zeros((self.height, self.width, 4), dtype=np.float32) for _ in range(3)]
        self._ck(self._lib.jpt_read_guides_f32(self.h, _ptr(g[0]), _ptr(g[1]), _ptr(g[2])), "jpt_read_guides_f32")
        return tuple(g)

    # ---- ray queries (jpt_query_rays / jpt_query_pixels)
    def query_rays(self, origins, dirs, tmax=None, mode=capi.QUERY_CLOSEST):
        """jpt_query_rays: n rays (origins, dirs [n, 3]; tmax a scalar or [n], None: unbounded) against the device's scene, blocking.
        QUERY_CLOSEST: (hits, occluded) -- a wire.RAY_HIT array and uint8 [n]; QUERY_ANY: occluded alone."""
        rays = make_rays(origins, dirs, tmax)
        n = len(rays)
        occ = np.zeros(n, np.uint8)
        hits = np.zeros(n, wire.RAY_HIT) if mode == capi.QUERY_CLOSEST else None
        self._ck(self._lib.jpt_query_rays(self.h, int(mode), _ptr(rays), n, _ptr(hits), _ptr(occ)), "jpt_query_rays")
        return occ if hits is None else (hits, occ)

    def query_pixels(self, xy) -> np.ndarray:
        """jpt_query_pixels: the closest hit of the un-jittered pinhole ray through each raster position xy [n, 2] (x + 0.5, y + 0.5:
        the centre of pixel (x, y)), a wire.RAY_HIT array; blocking"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        hits = np.zeros(len(xy), wire.RAY_HIT)
        self._ck(self._lib.jpt_query_pixels(self.h, _ptr(xy), len(xy), _ptr(hits)), "jpt_query_pixels")
        return hits

    def query_rays_device(self, rays, hits=None, occluded=None, mode=capi.QUERY_CLOSEST, n=None):
        """jpt_query_rays_device: rays already on the device -- a torch tensor (n * 32 bytes of wire.RAY records, any dtype and
        shape, contiguous) or a raw device pointer with `n`.  With `hits` / `occluded` given (tensors or pointers, written in
        place) the call only enqueues on the context's stream and returns None: sync() or work on get_stream()'s stream orders
        against it.  With neither, torch tensors are made for the results, the context is synchronised and they are returned as
        query_rays returns them."""
        def ptr_of(a):
            return None if a is None else int(a) if isinstance(a, int) else int(a.data_ptr())
        if n is None:
            if isinstance(rays, int):
                raise ValueError("a raw pointer needs n")
            n = rays.numel() * rays.element_size() // wire.RAY.itemsize
        own = hits is None and occluded is None
        if own:
            import torch
            occluded = torch.zeros(max(n, 1), dtype=torch.uint8, device=rays.device)
            if mode == capi.QUERY_CLOSEST:
                hits = torch.zeros(max(n, 1) * wire.RAY_HIT.itemsize, dtype=torch.uint8, device=rays.device)
            torch.cuda.synchronize(rays.device)   # (the tensors are made on torch's stream, the query runs on the context's)
        self._ck(self._lib.jpt_query_rays_device(self.h, int(mode), ptr_of(rays), int(n), ptr_of(hits), ptr_of(occluded)),
                 "jpt_query_rays_device")
        if not own:
            return None
        self.sync()
        occ = occluded.cpu().numpy()[:n]
        return occ if hits is None else (hits.cpu().numpy().view(wire.RAY_HIT)[:n], occ)

    def device_accum(self):
        n = C.c_size_t()
        p = self._lib.jpt_device_accum(self.h, C.byref(n))
        return p, n.value

    def device_ldr(self):
        n = C.c_size_t()
        p = self._lib.jpt_device_ldr(self.h, C.byref(n))
        return p, n.value

    def assemble_ldr_from_ranks(self, device_ptr: int, world: int):
        self._ck(self._lib.jpt_assemble_ldr_from_ranks(self.h, device_ptr, world), "jpt_assemble_ldr_from_ranks")

    def local_rows(self) -> int:
        return self._lib.jpt_local_rows(self.h)

    def assemble_from_ranks(self, device_ptr: int, world: int):
        self._ck(self._lib.jpt_assemble_from_ranks(self.h, device_ptr, world), "jpt_assemble_from_ranks")

    def stats(self) -> dict:
        s = capi.Stats()
        self._ck(self._lib.jpt_get_stats(self.h, C.byref(s)), "jpt_get_stats")
        return s.as_dict()


class GeometryGroup3D:
    """geometry_group3d.h:17-95.  `build()` runs the builder + upload; the get_*_buffer() getters return
    the reference-layout byte buffers (valid after a REFERENCE_EXACT build)."""

    def __init__(self, scene: scenes.Scene, builder: int = capi.BUILD_SAH):
        self.scene = scene
        self.builder = builder
        self.ctx: Optional[Context] = None

    def build(self, ctx: Context):                      # geometry_group3d.cpp:228
        self.ctx = ctx
        ctx.build_scene(self.scene, self.builder)
        self._built = [np.array(i.transform, dtype=np.float32) for i in self.scene.instances]

    def update_transforms(self, refit: bool = False, rebuild: bool = False) -> int:
        """Moving nodes without build() again (the reference has no such call; README.md:39-40 wants one): hands
        the changed instance transforms to the library, which redoes BLASInstance records + TLAS only -- on the host
        (rebuild, the default) or, with refit=True, on the device over the topology of the last build; rebuild=True (with refit): with a
        new topology made on the device (jpt_scene_rebuild_tlas), for nodes that swap places."""
        moved = 0
        for i, inst in enumerate(self.scene.instances):
            now = np.asarray(inst.transform, dtype=np.float32)
            if now.tobytes() != self._built[i].tobytes():
                self.ctx.set_instance_transform(i, now)
                self._built[i] = now.copy()
                moved += 1
        if moved:
            if refit and rebuild:
                self.ctx.rebuild_tlas(np.stack(self._built))
            elif refit:
                self.ctx.refit_tlas(np.stack(self._built))
            else:
                self.ctx.update_tlas()
        return moved

    def update_mesh(self, mesh_index: int, mesh: Optional[scenes.Mesh] = None):
        """A deformed mesh without build() again (the reference rebuilds the whole group): `mesh` (default: the scene's own
        mesh object, changed in place) has the vertex counts and index arrays it had at build(); the library refits that mesh's
        triangle records and BLAS boxes on the device (the group must be built with capi.BUILD_SAH_WATERTIGHT)."""
        if mesh is None:
            mesh = self.scene.meshes[mesh_index]
        else:
            self.scene.meshes[mesh_index] = mesh
        self.ctx.update_mesh(mesh_index, mesh)

    def rebuild_mesh(self, mesh_index: int, mesh: Optional[scenes.Mesh] = None):
        """update_mesh with a new BLAS topology made on the device (jpt_scene_rebuild_mesh): for a mesh that deformed far from its
        shape at build()"""
        if mesh is None:
            mesh = self.scene.meshes[mesh_index]
        else:
            self.scene.meshes[mesh_index] = mesh
        self.ctx.rebuild_mesh(mesh_index, mesh)

    def set_mesh_rig(self, mesh_index: int, rigs, influences: int, n_blend_shapes: int, bind: Optional[scenes.Mesh] = None, with_normals: bool = True):
        """The rig of one of the group's meshes (Skeleton3D / Skin and blend shapes): `bind` (default: the scene's own mesh) is its bind pose"""
        self.ctx.set_mesh_rig(mesh_index, self.scene.meshes[mesh_index] if bind is None else bind, rigs, influences, n_blend_shapes, with_normals)

    def pose_mesh(self, mesh_index: int, bone_transforms12=None, blend_weights=None, rebuild: bool = False):
        """A rigged mesh posed on the device, without build() again; the scene's own mesh object keeps its bind pose.  rebuild: with a
        new BLAS topology over the posed vertices"""
        self.ctx.pose_mesh(mesh_index, bone_transforms12, blend_weights, rebuild)

    def clear_mesh_rig(self, mesh_index: int):
        self.ctx.clear_mesh_rig(mesh_index)

    debug_skin = staticmethod(debug_skin)

    def get_triangles_geometry_buffer(self):            # geometry_group3d.cpp:40
        return self.ctx.reference_buffer(capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY)

    def get_triangles_data_buffer(self):                # :45
        return self.ctx.reference_buffer(capi.BUF_TRI_DATA, wire.TRI_DATA)

    def get_materials_buffer(self):                     # :50
        return self.ctx.reference_buffer(capi.BUF_MATERIALS, wire.MATERIAL)

    def get_bvh_buffer(self):                           # :55
        return self.ctx.reference_buffer(capi.BUF_BVH_NODES, wire.BVH_NODE)

    def get_blas_buffer(self):                          # :60
        return self.ctx.reference_buffer(capi.BUF_INSTANCES, wire.BLAS_INSTANCE)

    def get_tlas_buffer(self):                          # :65
        return self.ctx.reference_buffer(capi.BUF_TLAS_NODES, wire.TLAS_NODE)

    def get_triangle_count(self):                       # :17
        return len(self.get_triangles_geometry_buffer())

    def get_blas_count(self):                           # :7
        return len(self.get_blas_buffer())

    def get_bvh_node_count(self):                       # :22
        return len(self.get_bvh_buffer())

    def get_tlas_node_count(self):                      # :27
        return len(self.get_tlas_buffer())


class TemporalReprojection:
    """temporal_reprojection.h:11-60 / temporal_reprojection.cpp:16-73, host half: keeps previous_vp and
    frame_count and produces the 88-byte RenderParameters each frame; the dispatch itself is part of jpt_render."""

    def __init__(self, width: int, height: int):
        self.params = np.zeros((), dtype=wire.TEMPORAL_PARAMS)
        self.params["width"], self.params["height"] = width, height
        self.params["frame_count"] = 1                                   # temporal_reprojection.cpp:25
        self.params["blendFactor"], self.params["nearPlane"], self.params["farPlane"] = 0.75, 0.01, 1000.0
        self.previous_vp = np.eye(4)                                     # Projection() is the identity

    def render(self, vp: np.ndarray) -> np.ndarray:                      # temporal_reprojection.cpp:56-72
        self.params["deltaMatrix"] = scenes.temporal_delta(self.previous_vp, vp)
        self.previous_vp = vp.copy()
        self.params["frame_count"] += 1
        return self.params.copy()


class PathTracingCamera:
    """path_tracing_camera.h:25-112: init() creates the device state, render() advances one frame
    (frame_index pre-incremented, path_tracing_camera.cpp:199) and accumulates progressively; the
    accumulation restarts when the camera transform changes (progressive_rendering.cpp:53-60)."""

    PROGRESSIVE_RENDERING, TEMPORAL_REPROJECTION, NONE = 0, 1, 2   # path_tracing_camera.h:30-34

    def __init__(self, geometry_group: GeometryGroup3D, device: int = 0, max_bounces: int = 4,
                 accum_mode: int = capi.ACCUM_REF_LDR8):
        self.geometry_group = geometry_group
        self.camera_desc = geometry_group.scene.camera
        self.max_bounces = max_bounces
        self.accum_mode = accum_mode
        self.denoising_mode = self.PROGRESSIVE_RENDERING
        self.frame_index = 0          # the reference never initialises it (render_parameters.h:19); 0 here
        self.ctx = Context(device)
        self._prev_transform = None
        self.temporal_reprojection: Optional[TemporalReprojection] = None
        self.width = self.height = 0

    def init(self, width: int, height: int):                        # path_tracing_camera.cpp:111-187
        self.width, self.height = width, height
        self.geometry_group.build(self.ctx)
        self.ctx.set_params(width, height, self.max_bounces, self.accum_mode)

    def render(self, n_frames: int = 1, denoise: bool = False):     # path_tracing_camera.cpp:193-232
        """denoise: the returned screen is jpt_denoise's view of the accumulation (progressive mode only; the accumulation goes on
        unbiased underneath)"""
        self.ctx.set_denoising_mode(self.denoising_mode)            # the switch at :207-225
        self.ctx.set_outputs(depth=self.denoising_mode == self.TEMPORAL_REPROJECTION)   # (main.glsl:435's image has one reader)
        self.ctx.set_camera(scenes.camera_block(self.camera_desc, self.width, self.height))
        first = self.frame_index + 1                                # camera.frame_index++ before the dispatch
        if self.denoising_mode == self.PROGRESSIVE_RENDERING:
            t = np.asarray(self.camera_desc.transform, dtype=np.float32)
            moved = self._prev_transform is None or not np.allclose(self._prev_transform, t, rtol=0, atol=1e-5)
            self._prev_transform = t.copy()
            if moved:
                self.ctx.accum_reset()                              # frame_count = 1 (progressive_rendering.cpp:56-57)
        elif self.denoising_mode == self.TEMPORAL_REPROJECTION:
            if self.temporal_reprojection is None:                  # :216-219
                self.temporal_reprojection = TemporalReprojection(self.width, self.height)
            if n_frames != 1:
                raise ValueError("temporal reprojection advances one frame per render()")
            vp = scenes.view_projection(self.camera_desc, self.width, self.height)
            self.ctx.set_temporal_params(self.temporal_reprojection.render(vp))   # :220
        self.ctx.render(n_frames, first)
        self.frame_index += n_frames
        if denoise:
            self.ctx.denoise()
            return self.ctx.read_denoised_ldr()
        return self.ctx.read_ldr()                                  # get_image_uniform_buffer (:228-229)


class MultiContext:
    """One jpt_multi: one image tiled across several GPUs from this process (jpt.h, jpt_multi_*).  `devices` may name a
    device more than once (rehearsal on a box with fewer GPUs)."""

    def __init__(self, devices):
        self._lib = capi.lib()
        ids = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self._lib.jpt_multi_create(ids, len(devices), C.byref(h))
        if rc != capi.OK:
            msg = self._lib.jpt_multi_last_error(None)
            raise capi.JptError("jpt_multi_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.h = h
        self.world = len(devices)
        self.width = self.height = 0
        _live_contexts.add(self)

    def close(self):
        if getattr(self, "h", None):
            self._lib.jpt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != capi.OK:
            msg = self._lib.jpt_multi_last_error(self.h)
            raise capi.JptError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))

    def ctx(self, rank: int) -> Context:
        return Context(_borrowed=C.c_void_p(self._lib.jpt_multi_ctx(self.h, rank)))

    def build_scene(self, scene, builder=capi.BUILD_SAH):
        self.ctx(0).build_scene(scene, builder)
        self._ck(self._lib.jpt_multi_share_scene(self.h), "jpt_multi_share_scene")

    def upload_reference_layout(self, *arrays, **kw):
        self.ctx(0).upload_reference_layout(*arrays, **kw)
        self._ck(self._lib.jpt_multi_share_scene(self.h), "jpt_multi_share_scene")

    # moving instances: forwarded to every rank's replica
    def set_instance_transform(self, instance: int, transform12):
        t = np.ascontiguousarray(transform12, dtype=np.float32).reshape(12)
        self._ck(self._lib.jpt_multi_set_instance_transform(self.h, instance, _ptr(t)), "jpt_multi_set_instance_transform")

    def update_tlas(self):
        self._ck(self._lib.jpt_multi_update_tlas(self.h), "jpt_multi_update_tlas")

    def refit_tlas(self, transforms12):
        t = np.ascontiguousarray(transforms12, dtype=np.float32).reshape(-1, 12)
        self._ck(self._lib.jpt_multi_refit_tlas(self.h, _ptr(t), t.shape[0]), "jpt_multi_refit_tlas")

    def rebuild_tlas(self, transforms12):
        t = np.ascontiguousarray(transforms12, dtype=np.float32).reshape(-1, 12)
        self._ck(self._lib.jpt_multi_rebuild_tlas(self.h, _ptr(t), t.shape[0]), "jpt_multi_rebuild_tlas")

    def update_reference_tlas(self, instances, tlas_nodes):
        a, b = np.ascontiguousarray(instances), np.ascontiguousarray(tlas_nodes)
        self._ck(self._lib.jpt_multi_update_reference_tlas(self.h, _ptr(a), len(a), _ptr(b), len(b)), "jpt_multi_update_reference_tlas")

    def update_mesh(self, mesh_id: int, mesh: scenes.Mesh, with_normals: bool = True):
        arr = _update_surfaces(mesh, with_normals)
        self._ck(self._lib.jpt_multi_update_mesh(self.h, mesh_id, arr, len(mesh.surfaces)), "jpt_multi_update_mesh")

    def rebuild_mesh(self, mesh_id: int, mesh: scenes.Mesh, with_normals: bool = True):
        """update_mesh with a new BLAS topology (jpt_multi_rebuild_mesh: every rank's replica)"""
        arr = _update_surfaces(mesh, with_normals)
        self._ck(self._lib.jpt_multi_rebuild_mesh(self.h, mesh_id, arr, len(mesh.surfaces)), "jpt_multi_rebuild_mesh")

    def set_mesh_rig(self, mesh_id: int, bind: scenes.Mesh, rigs, influences: int, n_blend_shapes: int, with_normals: bool = True):
        """The rig of a committed mesh, kept on the device (jpt_multi_set_mesh_rig: every rank's replica): `bind` is the bind-pose mesh (same surfaces, vertex
        counts and index arrays as committed; with_normals False: the committed normals stay), `rigs` one SurfaceRig per surface."""
        arr, rarr = _update_surfaces(bind, with_normals), _rig_surfaces(rigs)
        self._ck(self._lib.jpt_multi_set_mesh_rig(self.h, mesh_id, arr, rarr, len(bind.surfaces), influences, n_blend_shapes), "jpt_multi_set_mesh_rig")

    def pose_mesh(self, mesh_id: int, bone_transforms12=None, blend_weights=None, rebuild: bool = False):
        """One pose of a rigged mesh (jpt_multi_pose_mesh: every rank's replica): float32 [n_bones, 12] bone transforms (bone pose x inverse bind, transform12
        layout) and one weight per blend shape; the vertices are computed and the mesh refitted on the device, no synchronisation.
        rebuild: with a new BLAS topology (jpt_multi_pose_mesh_rebuild)."""
        b, nb, w, nw = _pose_arrays(bone_transforms12, blend_weights)
        name = "jpt_multi_pose_mesh_rebuild" if rebuild else "jpt_multi_pose_mesh"
        self._ck(getattr(self._lib, name)(self.h, mesh_id, _ptr(b), nb, _ptr(w), nw), name)

    def clear_mesh_rig(self, mesh_id: int):
        self._ck(self._lib.jpt_multi_clear_mesh_rig(self.h, mesh_id), "jpt_multi_clear_mesh_rig")

    debug_skin = staticmethod(debug_skin)

    def set_params(self, width, height, max_bounces=4, accum_mode=capi.ACCUM_REF_LDR8, sampler_mode=0):
        self._ck(self._lib.jpt_multi_set_params(self.h, width, height, max_bounces, accum_mode, sampler_mode), "jpt_multi_set_params")
        self.width, self.height = width, height

    def set_environment(self, rgb):
        a, w, h = _env_map(rgb)
        self._ck(self._lib.jpt_multi_set_environment(self.h, None if a is None else _ptr(a), w, h), "jpt_multi_set_environment")

    def set_sky(self, params=None, width=2048, height=1024, samples=4):
        self._ck(self._lib.jpt_multi_set_sky(self.h, _sky_ref(params), int(width), int(height), int(samples)), "jpt_multi_set_sky")

    def set_environment_params(self, rotation=None, intensity: float = 1.0):
        r = _env_rotation(rotation)
        self._ck(self._lib.jpt_multi_set_environment_params(self.h, None if r is None else _ptr(r), float(intensity)),
                 "jpt_multi_set_environment_params")

    def set_environment_sampling(self, mode):
        self._ck(self._lib.jpt_multi_set_environment_sampling(self.h, int(mode)), "jpt_multi_set_environment_sampling")

    def set_light_sampling(self, mode):
        self._ck(self._lib.jpt_multi_set_light_sampling(self.h, int(mode)), "jpt_multi_set_light_sampling")

    def set_lens(self, aperture_radius, focus_distance):
        self._ck(self._lib.jpt_multi_set_lens(self.h, float(aperture_radius), float(focus_distance)), "jpt_multi_set_lens")

    def set_camera_model(self, model):
        self._ck(self._lib.jpt_multi_set_camera_model(self.h, int(model)), "jpt_multi_set_camera_model")

    def set_bake_texels(self, position4, normal4):
        if position4 is None and normal4 is None:
            self._ck(self._lib.jpt_multi_set_bake_texels(self.h, None, None, 0, 0), "jpt_multi_set_bake_texels")
            return
        p, n = _bake_images(position4, normal4)
        self._ck(self._lib.jpt_multi_set_bake_texels(self.h, _ptr(p), _ptr(n), p.shape[1], p.shape[0]), "jpt_multi_set_bake_texels")

    def set_material_extensions(self, flags):
        self._ck(self._lib.jpt_multi_set_material_extensions(self.h, int(flags)), "jpt_multi_set_material_extensions")

    def set_camera(self, camera_block):
        cam = np.ascontiguousarray(camera_block, dtype=wire.CAMERA).reshape(1)
        self._ck(self._lib.jpt_multi_set_camera(self.h, _ptr(cam)), "jpt_multi_set_camera")

    def set_gather(self, ldr_only: bool):
        self._ck(self._lib.jpt_multi_set_gather(self.h, 1 if ldr_only else 0), "jpt_multi_set_gather")

    def accum_reset(self):
        self._ck(self._lib.jpt_multi_accum_reset(self.h), "jpt_multi_accum_reset")

    def render(self, n_frames, first_frame_index):
        self._ck(self._lib.jpt_multi_render(self.h, n_frames, first_frame_index), "jpt_multi_render")

    def sync(self):
        self._ck(self._lib.jpt_multi_sync(self.h), "jpt_multi_sync")

    def gather_plan(self) -> dict:
        """what the last render issued for its gather: peer copies, distinct streams they went on, copies of rank 0's own piece"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.jpt_multi_gather_plan(self.h, C.byref(a), C.byref(b), C.byref(c)), "jpt_multi_gather_plan")
        return {"peer_copies": a.value, "distinct_streams": b.value, "own_piece_copies": c.value}

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._ck(self._lib.jpt_multi_read_accum_f32(self.h, _ptr(out)), "jpt_multi_read_accum_f32")
        return out

    def read_ldr(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._ck(self._lib.jpt_multi_read_ldr_rgba8(self.h, _ptr(out)), "jpt_multi_read_ldr_rgba8")
        return out
