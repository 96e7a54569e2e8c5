"""ctypes loader for libjpt_hip.so (the C ABI of include/jpt.h).

There is no CPU fallback: if the HIP library is missing or no GPU is present, calls fail loudly.
`build()` compiles the library in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

# the library keeps six renders in flight where six of its streams get a hardware queue each: GPU_MAX_HW_QUEUES (per stream priority
# level) is read by the HIP runtime at the process's first HIP call and is the host's to export; it is not set here (jpt.h, jpt_create)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JPT_LIB", os.path.join(_HERE, "libjpt_hip.so"))  # JPT_LIB: A/B builds (tools/ab.sh)
CSRC = os.path.join(_HERE, "csrc")

OK = 0
ACCUM_REF_LDR8, ACCUM_HDR_F32 = 0, 1
BUILD_REFERENCE_EXACT, BUILD_SAH, BUILD_SAH_WATERTIGHT = 0, 1, 2
KERNEL_WAVEFRONT, KERNEL_REFERENCE_LAYOUT = 0, 1
SAMPLER_NEAREST_CLAMP, SAMPLER_NEAREST_REPEAT, SAMPLER_LINEAR_CLAMP, SAMPLER_LINEAR_REPEAT = 0, 1, 2, 3
DENOISE_PROGRESSIVE, DENOISE_TEMPORAL, DENOISE_NONE = 0, 1, 2
OUTPUT_DEPTH = 1
ENV_SAMPLING_BRDF, ENV_SAMPLING_MIS = 0, 1
LIGHT_SAMPLING_BRDF, LIGHT_SAMPLING_MIS = 0, 1
MATERIAL_EXT_NONE, MATERIAL_EXT_TRANSMISSION = 0, 1
UPLOAD_NATIVE_TREE, UPLOAD_WALK_AS_GIVEN = 0, 1
DISPLAY_SOURCE_ACCUM, DISPLAY_SOURCE_DENOISED = 0, 1
TONEMAP_ACES_REF, TONEMAP_REINHARD, TONEMAP_CLAMP = 0, 1, 2
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1
METER_AVERAGE, METER_CENTER_WEIGHTED = 0, 1
METER_EMPTY, METER_FIRST = 1, 2
NOISE_EMPTY, NOISE_CONVERGED = 1, 2
STREAM_PRIORITY_DEFAULT, STREAM_PRIORITY_NORMAL, STREAM_PRIORITY_HIGH, STREAM_PRIORITY_LOW = 0, 1, 2, 3
TREE_NONE, TREE_AS_GIVEN, TREE_REFERENCE_EXACT, TREE_NATIVE_REACH, TREE_NATIVE_WATERTIGHT = range(5)
QUERY_CLOSEST, QUERY_ANY = 0, 1
CAMERA_PINHOLE, CAMERA_PROJECTIVE, CAMERA_EQUIRECT = 0, 1, 2
PROBE_RADIANCE, PROBE_IRRADIANCE = 0, 1
ENCODE_RGBA16F, ENCODE_RGB9E5, ENCODE_RGBE8 = 1, 2, 3
ENCODE_SOURCE_MEAN, ENCODE_SOURCE_DENOISED, ENCODE_SOURCE_DISPLAY, ENCODE_SOURCE_LIGHTMAP, ENCODE_SOURCE_REFLECTION, ENCODE_SOURCE_PROBE_SH = range(6)
ENCODE_ALL_LEVELS = -1
SUN_RADIANCE, SUN_IRRADIANCE = 0, 1
HIT_VALID, HIT_FRONT, HIT_BAD_RAY = 1, 2, 4
BUF_TRI_GEOMETRY, BUF_TRI_DATA, BUF_MATERIALS, BUF_BVH_NODES, BUF_INSTANCES, BUF_TLAS_NODES, BUF_TRIANGLES, BUF_REACH_TRIANGLES, BUF_REACH_INSTANCES = range(9)

# every symbol include/jpt.h declares
SYMBOLS = [
    "jpt_abi_version", "jpt_create", "jpt_destroy", "jpt_last_error", "jpt_set_stream", "jpt_get_stream", "jpt_set_stream_priority", "jpt_renders_in_flight", "jpt_set_memory_policy", "jpt_get_workspace_bytes",
    "jpt_scene_upload_reference_layout", "jpt_set_upload_mode", "jpt_scene_tree_kind", "jpt_scene_upload_note", "jpt_scene_ties_exact", "jpt_scene_begin", "jpt_scene_add_mesh", "jpt_scene_add_instance",
    "jpt_scene_set_materials", "jpt_scene_set_textures", "jpt_scene_commit", "jpt_scene_get_reference_buffer",
    "jpt_scene_set_instance_transform", "jpt_scene_update_tlas", "jpt_scene_refit_tlas", "jpt_scene_rebuild_tlas", "jpt_scene_update_reference_tlas", "jpt_scene_update_mesh",
    "jpt_set_params", "jpt_set_kernel", "jpt_set_debug_steps", "jpt_set_kernel_timing", "jpt_set_partition", "jpt_set_camera", "jpt_render", "jpt_render_counted", "jpt_render_async",
    "jpt_sync", "jpt_accum_reset", "jpt_set_progressive_frame_count", "jpt_set_denoising_mode", "jpt_set_temporal_params", "jpt_set_outputs", "jpt_read_ldr_rgba8", "jpt_readback_ldr_begin", "jpt_readback_ldr_end", "jpt_read_accum_f32", "jpt_read_depth_f32",
    "jpt_device_accum", "jpt_assemble_from_ranks", "jpt_device_ldr", "jpt_assemble_ldr_from_ranks", "jpt_local_rows", "jpt_get_stats",
    "jpt_scene_share", "jpt_multi_create", "jpt_multi_destroy", "jpt_multi_last_error", "jpt_multi_world", "jpt_multi_ctx",
    "jpt_multi_share_scene", "jpt_multi_set_instance_transform", "jpt_multi_update_tlas", "jpt_multi_refit_tlas", "jpt_multi_rebuild_tlas",
    "jpt_multi_update_reference_tlas", "jpt_multi_update_mesh", "jpt_multi_set_params", "jpt_multi_set_camera", "jpt_multi_accum_reset", "jpt_multi_set_gather",
    "jpt_multi_render", "jpt_multi_sync", "jpt_multi_gather_plan", "jpt_multi_read_ldr_rgba8", "jpt_multi_read_accum_f32",
    "jpt_debug_quantize_nodes4", "jpt_debug_node_step4", "jpt_debug_last_error", "jpt_debug_mesh_records",
    "jpt_debug_tlas_order", "jpt_debug_tlas_template", "jpt_debug_tlas_records",
    "jpt_set_environment", "jpt_set_environment_params", "jpt_multi_set_environment", "jpt_multi_set_environment_params",
    "jpt_debug_env_lookup",
    "jpt_set_environment_sampling", "jpt_multi_set_environment_sampling", "jpt_debug_env_tables", "jpt_debug_env_sample", "jpt_debug_env_pdf",
    "jpt_set_light_sampling", "jpt_multi_set_light_sampling", "jpt_debug_light_tables", "jpt_debug_light_sample", "jpt_debug_light_pdf",
    "jpt_set_material_extensions", "jpt_multi_set_material_extensions", "jpt_debug_dielectric",
    "jpt_set_lens", "jpt_multi_set_lens", "jpt_debug_lens_rays", "jpt_debug_lens_sample",
    "jpt_set_camera_model", "jpt_multi_set_camera_model", "jpt_debug_camera_rays",
    "jpt_set_bake_texels", "jpt_bake_begin", "jpt_bake_add_surface", "jpt_read_bake_texels", "jpt_multi_set_bake_texels",
    "jpt_debug_bake_rays", "jpt_debug_bake_raster",
    "jpt_set_probes", "jpt_get_probe_image_size", "jpt_read_probes", "jpt_probe_project", "jpt_read_probe_sh_f32",
    "jpt_debug_probe_rays", "jpt_debug_probe_basis", "jpt_debug_probe_project",
    "jpt_set_reflection_probes", "jpt_get_reflection_image_size", "jpt_read_reflection_probes", "jpt_set_reflection_params", "jpt_reflection_prefilter",
    "jpt_get_reflection_chain_size", "jpt_read_reflection_f32", "jpt_get_reflection_timing",
    "jpt_debug_cube_rays", "jpt_debug_reflection_samples", "jpt_debug_reflection_prefilter",
    "jpt_set_bake_finish_params", "jpt_bake_finish", "jpt_read_lightmap_f32", "jpt_debug_bake_finish",
    "jpt_set_bake_directional", "jpt_read_bake_directional_f32", "jpt_device_bake_directional", "jpt_bake_finish_directional",
    "jpt_read_lightmap_directional_f32", "jpt_debug_bake_moments",
    "jpt_set_denoise_params", "jpt_denoise", "jpt_read_denoised_f32", "jpt_read_denoised_rgba8", "jpt_read_guides_f32", "jpt_debug_atrous",
    "jpt_set_denoise_variance", "jpt_read_denoised_variance_f32", "jpt_debug_atrous_variance",
    "jpt_set_denoise_history", "jpt_denoise_history_reset", "jpt_read_denoise_history_f32", "jpt_debug_denoise_history",
    "jpt_set_display_params", "jpt_display", "jpt_read_display_rgba8", "jpt_read_display_f32", "jpt_debug_display", "jpt_debug_display_srgb_table",
    "jpt_set_meter_params", "jpt_meter", "jpt_meter_reset", "jpt_read_meter", "jpt_set_auto_exposure", "jpt_debug_meter",
    "jpt_set_variance", "jpt_read_variance_f32", "jpt_device_variance", "jpt_set_noise_params", "jpt_noise_estimate", "jpt_read_noise",
    "jpt_read_noise_tiles_f32", "jpt_device_noise_tiles", "jpt_render_converge", "jpt_debug_variance_moments", "jpt_debug_noise_estimate",
    "jpt_query_rays", "jpt_query_rays_device", "jpt_query_pixels",
    "jpt_scene_set_mesh_rig", "jpt_scene_pose_mesh", "jpt_scene_clear_mesh_rig", "jpt_multi_set_mesh_rig", "jpt_multi_pose_mesh", "jpt_multi_clear_mesh_rig",
    "jpt_debug_skin",
    "jpt_encode", "jpt_get_encoded_info", "jpt_read_encoded", "jpt_readback_encoded_begin", "jpt_readback_encoded_end", "jpt_device_encoded",
    "jpt_get_encode_timing", "jpt_debug_encode",
    "jpt_scene_rebuild_mesh", "jpt_scene_pose_mesh_rebuild", "jpt_multi_rebuild_mesh", "jpt_multi_pose_mesh_rebuild", "jpt_debug_mesh_order",
    "jpt_sky_defaults", "jpt_set_sky", "jpt_read_environment_f32", "jpt_multi_set_sky", "jpt_debug_sky", "jpt_debug_sky_radiance", "jpt_debug_pow01",
]


class JptError(RuntimeError):
    pass


class Surface(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("normals", C.c_void_p), ("uvs", C.c_void_p), ("indices", C.c_void_p),
                ("n_vertices", C.c_int32), ("n_indices", C.c_int32)]


class SurfaceRig(C.Structure):
    """jpt_surface_rig: one surface's bones, weights and blend-shape deltas (jpt_scene_set_mesh_rig)"""
    _fields_ = [("bones", C.c_void_p), ("weights", C.c_void_p), ("position_deltas", C.c_void_p), ("normal_deltas", C.c_void_p)]


class DenoiseParams(C.Structure):
    """jpt_denoise_params; the defaults are the library's"""
    _fields_ = [("passes", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_plane", C.c_float), ("sigma_color", C.c_float)]

    def __init__(self, passes=5, normal_power_log2=6, sigma_plane=0.02, sigma_color=4.0):
        super().__init__(passes, normal_power_log2, sigma_plane, sigma_color)


class DenoiseVarianceParams(C.Structure):
    """jpt_denoise_variance_params; the defaults are the library's (the guidance off)"""
    _fields_ = [("enable", C.c_int32), ("sigma_variance", C.c_float), ("variance_floor", C.c_float), ("reserved", C.c_int32)]

    def __init__(self, enable=0, sigma_variance=2.0, variance_floor=1e-6, reserved=0):
        super().__init__(enable, sigma_variance, variance_floor, reserved)


class DenoiseHistoryParams(C.Structure):
    """jpt_denoise_history_params; the defaults are the library's (the history off)"""
    _fields_ = [("enable", C.c_int32), ("max_history", C.c_int32), ("min_history", C.c_int32), ("sigma_plane", C.c_float), ("reserved", C.c_int32 * 4)]

    def __init__(self, enable=0, max_history=32, min_history=4, sigma_plane=0.05, reserved=(0, 0, 0, 0)):
        super().__init__(enable, max_history, min_history, sigma_plane, (C.c_int32 * 4)(*reserved))


class BakeFinishParams(C.Structure):
    """jpt_bake_finish_params; the defaults are the library's"""
    _fields_ = [("passes", C.c_int32), ("normal_power_log2", C.c_int32), ("dilate", C.c_int32), ("sigma_distance", C.c_float),
                ("sigma_plane", C.c_float), ("sigma_color", C.c_float)]

    def __init__(self, passes=3, normal_power_log2=4, dilate=4, sigma_distance=4.0, sigma_plane=1.0, sigma_color=4.0):
        super().__init__(passes, normal_power_log2, dilate, sigma_distance, sigma_plane, sigma_color)


class ReflectionParams(C.Structure):
    """jpt_reflection_params; the defaults are the library's (n_levels 0: every level down to 1 x 1)"""
    _fields_ = [("n_levels", C.c_int32), ("samples", C.c_int32)]

    def __init__(self, n_levels=0, samples=64):
        super().__init__(n_levels, samples)


class DisplayParams(C.Structure):
    """jpt_display_params; the defaults are the library's"""
    _fields_ = [("source", C.c_int32), ("tonemap", C.c_int32), ("transfer", C.c_int32), ("bloom_levels", C.c_int32),
                ("exposure", C.c_float), ("white", C.c_float), ("bloom_threshold", C.c_float), ("bloom_strength", C.c_float)]

    def __init__(self, source=DISPLAY_SOURCE_ACCUM, tonemap=TONEMAP_ACES_REF, transfer=TRANSFER_LINEAR, bloom_levels=0, exposure=1.0,
                 white=4.0, bloom_threshold=1.0, bloom_strength=0.25):
        super().__init__(source, tonemap, transfer, bloom_levels, exposure, white, bloom_threshold, bloom_strength)


class MeterParams(C.Structure):
    """jpt_meter_params; the defaults are the library's"""
    _fields_ = [("source", C.c_int32), ("mode", C.c_int32), ("low_permille", C.c_int32), ("high_permille", C.c_int32),
                ("key", C.c_float), ("min_exposure", C.c_float), ("max_exposure", C.c_float), ("adapt", C.c_float)]

    def __init__(self, source=DISPLAY_SOURCE_ACCUM, mode=METER_AVERAGE, low_permille=100, high_permille=900, key=0.18, min_exposure=1.0 / 64.0,
                 max_exposure=64.0, adapt=1.0):
        super().__init__(source, mode, low_permille, high_permille, key, min_exposure, max_exposure, adapt)


class MeterResult(C.Structure):
    """jpt_meter_result (32 bytes)"""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("luminance", C.c_float), ("flags", C.c_uint32),
                ("weight", C.c_uint64), ("used", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class NoiseParams(C.Structure):
    """jpt_noise_params; the defaults are the library's"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("percentile_permille", C.c_int32), ("allowed_permille", C.c_int32)]

    def __init__(self, threshold=0.05, floor=0.01, percentile_permille=950, allowed_permille=0):
        super().__init__(threshold, floor, percentile_permille, allowed_permille)


class NoiseResult(C.Structure):
    """jpt_noise_result (32 bytes)"""
    _fields_ = [("error", C.c_float), ("max_error", C.c_float), ("flags", C.c_uint32), ("tiles_above", C.c_uint32),
                ("counted", C.c_uint64), ("above", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EncodedInfo(C.Structure):
    """jpt_encoded_info"""
    _fields_ = [("source", C.c_int32), ("format", C.c_int32), ("level", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_texels", C.c_uint64), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def encoded_array(fmt: int, n_texels: int):
    """a numpy array for n_texels texels of a jpt_encode format: RGBA16F float16 [n, 4], RGB9E5 uint32 [n], RGBE8 uint8 [n, 4]"""
    import numpy as np
    if fmt == ENCODE_RGBA16F:
        return np.zeros((n_texels, 4), np.float16)
    if fmt == ENCODE_RGB9E5:
        return np.zeros(n_texels, np.uint32)
    if fmt == ENCODE_RGBE8:
        return np.zeros((n_texels, 4), np.uint8)
    raise ValueError("unknown encode format %r" % (fmt,))


class SkySun(C.Structure):
    """jpt_sky_sun: direction (towards the sun, any length), angular_radius (radians), color, energy, mode (SUN_RADIANCE / SUN_IRRADIANCE)"""
    _fields_ = [("direction", C.c_float * 3), ("angular_radius", C.c_float), ("color", C.c_float * 3), ("energy", C.c_float), ("mode", C.c_int32)]


class SkyParams(C.Structure):
    """jpt_sky_params (jpt_set_sky); sky_params() returns one filled with the library's defaults"""
    _fields_ = [("sky_top_color", C.c_float * 3), ("sky_curve", C.c_float), ("sky_horizon_color", C.c_float * 3), ("sky_energy", C.c_float),
                ("ground_bottom_color", C.c_float * 3), ("ground_curve", C.c_float), ("ground_horizon_color", C.c_float * 3), ("ground_energy", C.c_float),
                ("sun_angle_max", C.c_float), ("sun_curve", C.c_float), ("exposure", C.c_float), ("n_suns", C.c_int32), ("suns", SkySun * 4)]


def sky_params(suns=(), **fields) -> "SkyParams":
    """a SkyParams with jpt_sky_defaults' values, then `fields` by name (colours as 3-sequences) and `suns`: up to four dicts or SkySun
    (direction, angular_radius, color, energy, mode)"""
    p = SkyParams()
    lib().jpt_sky_defaults(C.byref(p))
    for name, v in fields.items():
        if name.endswith("_color"):
            setattr(p, name, (C.c_float * 3)(*[float(x) for x in v]))
        else:
            setattr(p, name, v)
    suns = list(suns)
    if len(suns) > 4:
        raise ValueError("at most four suns")
    for k, sun in enumerate(suns):
        if isinstance(sun, SkySun):
            p.suns[k] = sun
            continue
        q = SkySun(energy=1.0, mode=SUN_RADIANCE)
        q.color = (C.c_float * 3)(1.0, 1.0, 1.0)
        for name, v in sun.items():
            if name in ("direction", "color"):
                setattr(q, name, (C.c_float * 3)(*[float(x) for x in v]))
            else:
                setattr(q, name, v)
        p.suns[k] = q
    if suns or "n_suns" not in fields:
        p.n_suns = len(suns)
    return p


class Ray(C.Structure):
    """jpt_ray (wire.RAY)"""
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("dir", C.c_float * 3), ("reserved", C.c_uint32)]


class RayHit(C.Structure):
    """jpt_ray_hit (wire.RAY_HIT)"""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("instance", C.c_int32), ("triangle", C.c_uint32),
                ("material", C.c_int32), ("flags", C.c_uint32), ("position", C.c_float * 3), ("normal", C.c_float * 3),
                ("uv", C.c_float * 2), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("frames", C.c_uint64), ("blas_expand", C.c_uint64), ("tri_tests", C.c_uint64),
                ("tlas_expand", C.c_uint64), ("inst_visits", C.c_uint64), ("shaded_hits", C.c_uint64),
                ("last_render_ms", C.c_double), ("last_trace_ms", C.c_double), ("last_build_ms", C.c_double),
                ("phase", C.c_uint64 * 8), ("sky_culled", C.c_uint64), ("last_primary_ms", C.c_double),
                ("set_aside", C.c_uint64), ("set_aside_dropped", C.c_uint64),
                ("walk_steps_max", C.c_uint64), ("walk_steps_hist", C.c_uint64 * 8), ("zero_throughput", C.c_uint64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["phase"] = list(self.phase)
        d["walk_steps_hist"] = list(self.walk_steps_hist)
        return d


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile libjpt_hip.so in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode:
        print(res.stdout)
    if res.returncode:
        raise JptError("building libjpt_hip.so failed")
    return LIB_PATH


_lib = None


def lib():
    """Load the HIP library; raises JptError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  If this library pulled the system
    # runtime in first, a later `import torch` in the same process finds no GPU; loading torch's first
    # works for both.  Only relevant where torch is used next to the library (tests, bench: plumbing).
    try:
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise JptError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the HIP path)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    L.jpt_abi_version.restype = C.c_int
    L.jpt_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.jpt_destroy.argtypes = [vp]
    L.jpt_destroy.restype = None
    L.jpt_last_error.argtypes = [vp]
    L.jpt_last_error.restype = C.c_char_p
    L.jpt_set_stream.argtypes = [vp, vp]
    L.jpt_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.jpt_set_stream_priority.argtypes = [vp, i32]
    L.jpt_set_memory_policy.argtypes = [vp, i32, C.c_uint64]
    L.jpt_get_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.jpt_scene_upload_reference_layout.argtypes = [vp, vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, i32, i32]
    L.jpt_set_upload_mode.argtypes = [vp, i32]
    L.jpt_scene_tree_kind.argtypes = [vp]
    L.jpt_scene_upload_note.argtypes = [vp]
    L.jpt_scene_upload_note.restype = C.c_char_p
    L.jpt_scene_ties_exact.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.jpt_scene_ties_exact.restype = C.c_int
    L.jpt_scene_begin.argtypes = [vp]
    L.jpt_scene_add_mesh.argtypes = [vp, C.POINTER(Surface), i32, C.POINTER(u32)]
    L.jpt_scene_add_instance.argtypes = [vp, u32, vp, vp, i32]
    L.jpt_scene_set_materials.argtypes = [vp, vp, u32]
    L.jpt_scene_set_textures.argtypes = [vp, vp, i32, i32]
    L.jpt_scene_commit.argtypes = [vp, i32]
    L.jpt_scene_get_reference_buffer.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.jpt_scene_set_instance_transform.argtypes = [vp, u32, vp]
    L.jpt_scene_update_tlas.argtypes = [vp]
    L.jpt_scene_refit_tlas.argtypes = [vp, vp, u32]
    L.jpt_scene_rebuild_tlas.argtypes = [vp, vp, u32]
    L.jpt_scene_update_reference_tlas.argtypes = [vp, vp, u32, vp, u32]
    L.jpt_scene_update_mesh.argtypes = [vp, u32, C.POINTER(Surface), i32]
    L.jpt_set_params.argtypes = [vp, i32, i32, i32, i32, i32]
    L.jpt_set_partition.argtypes = [vp, i32, i32]
    L.jpt_set_kernel.argtypes = [vp, i32]
    L.jpt_set_kernel_timing.argtypes = [vp, i32]
    L.jpt_set_debug_steps.argtypes = [vp, i32]
    L.jpt_set_camera.argtypes = [vp, vp]
    for n in ("jpt_render", "jpt_render_counted", "jpt_render_async"):
        getattr(L, n).argtypes = [vp, i32, u32]
    L.jpt_sync.argtypes = [vp]
    L.jpt_accum_reset.argtypes = [vp]
    L.jpt_set_progressive_frame_count.argtypes = [vp, u32]
    L.jpt_set_denoising_mode.argtypes = [vp, i32]
    L.jpt_set_temporal_params.argtypes = [vp, vp]
    if hasattr(L, "jpt_set_outputs") or "JPT_LIB" not in os.environ:   # (JPT_LIB: an A/B build of an earlier ABI may lack it)
        L.jpt_set_outputs.argtypes = [vp, C.c_uint32]
    if hasattr(L, "jpt_renders_in_flight") or "JPT_LIB" not in os.environ:
        L.jpt_renders_in_flight.argtypes = [vp]
        L.jpt_renders_in_flight.restype = C.c_int
    L.jpt_read_ldr_rgba8.argtypes = [vp, vp]
    L.jpt_read_accum_f32.argtypes = [vp, vp]
    L.jpt_readback_ldr_begin.argtypes = [vp]
    L.jpt_readback_ldr_end.argtypes = [vp, vp]
    L.jpt_read_depth_f32.argtypes = [vp, vp]
    L.jpt_device_accum.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.jpt_device_accum.restype = vp
    L.jpt_assemble_from_ranks.argtypes = [vp, vp, i32]
    L.jpt_device_ldr.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.jpt_device_ldr.restype = vp
    L.jpt_assemble_ldr_from_ranks.argtypes = [vp, vp, i32]
    L.jpt_local_rows.argtypes = [vp]
    L.jpt_local_rows.restype = i32
    L.jpt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.jpt_scene_share.argtypes = [vp, vp]
    L.jpt_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.jpt_multi_destroy.argtypes = [vp]
    L.jpt_multi_destroy.restype = None
    L.jpt_multi_last_error.argtypes = [vp]
    L.jpt_multi_last_error.restype = C.c_char_p
    L.jpt_multi_world.argtypes = [vp]
    L.jpt_multi_ctx.argtypes = [vp, C.c_int]
    L.jpt_multi_ctx.restype = vp
    L.jpt_multi_share_scene.argtypes = [vp]
    L.jpt_multi_set_instance_transform.argtypes = [vp, u32, vp]
    L.jpt_multi_update_tlas.argtypes = [vp]
    L.jpt_multi_refit_tlas.argtypes = [vp, vp, u32]
    L.jpt_multi_rebuild_tlas.argtypes = [vp, vp, u32]
    L.jpt_multi_update_reference_tlas.argtypes = [vp, vp, u32, vp, u32]
    L.jpt_multi_update_mesh.argtypes = [vp, u32, C.POINTER(Surface), i32]
    L.jpt_multi_set_params.argtypes = [vp, i32, i32, i32, i32, i32]
    L.jpt_multi_set_camera.argtypes = [vp, vp]
    L.jpt_multi_accum_reset.argtypes = [vp]
    L.jpt_multi_set_gather.argtypes = [vp, i32]
    L.jpt_multi_render.argtypes = [vp, i32, u32]
    L.jpt_multi_sync.argtypes = [vp]
    L.jpt_multi_gather_plan.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.jpt_multi_read_ldr_rgba8.argtypes = [vp, vp]
    L.jpt_multi_read_accum_f32.argtypes = [vp, vp]
    L.jpt_debug_quantize_nodes4.argtypes = [vp, u32, vp]
    L.jpt_debug_node_step4.argtypes = [C.c_int, vp, u32, vp, u32, i32, vp]
    L.jpt_debug_last_error.restype = C.c_char_p
    L.jpt_debug_mesh_records.argtypes = [vp, u32, vp, vp, u32, vp, vp, u32, C.POINTER(i32)]
    L.jpt_debug_tlas_order.argtypes = [C.c_int, vp, vp, u32, vp, vp]
    L.jpt_debug_tlas_template.argtypes = [u32, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.jpt_debug_tlas_records.argtypes = [vp, vp, vp, u32, C.POINTER(u32), C.POINTER(i32), vp, vp]
    L.jpt_set_environment.argtypes = [vp, vp, i32, i32]
    L.jpt_set_environment_params.argtypes = [vp, vp, C.c_float]
    L.jpt_multi_set_environment.argtypes = [vp, vp, i32, i32]
    L.jpt_multi_set_environment_params.argtypes = [vp, vp, C.c_float]
    L.jpt_debug_env_lookup.argtypes = [C.c_int, vp, i32, i32, vp, C.c_float, vp, u32, vp]
    if hasattr(L, "jpt_set_environment_sampling") or "JPT_LIB" not in os.environ:
        L.jpt_set_environment_sampling.argtypes = [vp, i32]
        L.jpt_multi_set_environment_sampling.argtypes = [vp, i32]
        L.jpt_debug_env_tables.argtypes = [C.c_int, vp, i32, i32, vp, vp, vp]
        L.jpt_debug_env_sample.argtypes = [C.c_int, vp, i32, i32, vp, vp, u32, vp, vp]
        L.jpt_debug_env_pdf.argtypes = [C.c_int, vp, i32, i32, vp, vp, u32, vp]
    if hasattr(L, "jpt_set_light_sampling") or "JPT_LIB" not in os.environ:
        L.jpt_set_light_sampling.argtypes = [vp, i32]
        L.jpt_multi_set_light_sampling.argtypes = [vp, i32]
        L.jpt_debug_light_tables.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.jpt_debug_light_sample.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.jpt_debug_light_pdf.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp]
    if hasattr(L, "jpt_set_material_extensions") or "JPT_LIB" not in os.environ:
        L.jpt_set_material_extensions.argtypes = [vp, u32]
        L.jpt_multi_set_material_extensions.argtypes = [vp, u32]
        L.jpt_debug_dielectric.argtypes = [C.c_int, vp, vp, vp, vp, vp, u32, vp, vp, vp]
    if hasattr(L, "jpt_set_lens") or "JPT_LIB" not in os.environ:
        L.jpt_set_lens.argtypes = [vp, C.c_float, C.c_float]
        L.jpt_multi_set_lens.argtypes = [vp, C.c_float, C.c_float]
        L.jpt_debug_lens_rays.argtypes = [C.c_int, vp, i32, i32, u32, C.c_float, C.c_float, vp, vp]
        L.jpt_debug_lens_sample.argtypes = [vp, C.c_float, C.c_float, vp, vp, vp, u32, vp, vp, vp]
    if hasattr(L, "jpt_set_camera_model") or "JPT_LIB" not in os.environ:
        L.jpt_set_camera_model.argtypes = [vp, i32]
        L.jpt_multi_set_camera_model.argtypes = [vp, i32]
        L.jpt_debug_camera_rays.argtypes = [C.c_int, vp, i32, i32, u32, i32, vp, vp]
    if hasattr(L, "jpt_set_bake_texels") or "JPT_LIB" not in os.environ:
        L.jpt_set_bake_texels.argtypes = [vp, vp, vp, i32, i32]
        L.jpt_bake_begin.argtypes = [vp, i32, i32]
        L.jpt_bake_add_surface.argtypes = [vp, C.POINTER(Surface), vp, vp]
        L.jpt_read_bake_texels.argtypes = [vp, vp, vp]
        L.jpt_multi_set_bake_texels.argtypes = [vp, vp, vp, i32, i32]
        L.jpt_debug_bake_rays.argtypes = [C.c_int, vp, vp, i32, i32, u32, vp, vp, vp]
        L.jpt_debug_bake_raster.argtypes = [C.c_int, C.POINTER(Surface), vp, vp, i32, i32, vp, vp]
    if hasattr(L, "jpt_bake_finish") or "JPT_LIB" not in os.environ:
        L.jpt_set_bake_finish_params.argtypes = [vp, C.POINTER(BakeFinishParams)]
        L.jpt_bake_finish.argtypes = [vp]
        L.jpt_read_lightmap_f32.argtypes = [vp, vp]
        L.jpt_debug_bake_finish.argtypes = [C.c_int, i32, i32, C.POINTER(BakeFinishParams), vp, vp, vp, vp]
    if hasattr(L, "jpt_set_bake_directional") or "JPT_LIB" not in os.environ:
        L.jpt_set_bake_directional.argtypes = [vp, i32]
        L.jpt_read_bake_directional_f32.argtypes = [vp, vp]
        L.jpt_device_bake_directional.restype = vp
        L.jpt_device_bake_directional.argtypes = [vp, i32, C.POINTER(C.c_size_t)]
        L.jpt_bake_finish_directional.argtypes = [vp]
        L.jpt_read_lightmap_directional_f32.argtypes = [vp, vp]
        L.jpt_debug_bake_moments.argtypes = [vp, vp, i32, i32, vp, i32, u32, u32, i32, vp]
    if hasattr(L, "jpt_set_probes") or "JPT_LIB" not in os.environ:
        L.jpt_set_probes.argtypes = [vp, vp, i32, i32, i32, i32]
        L.jpt_get_probe_image_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        L.jpt_read_probes.argtypes = [vp, vp]
        L.jpt_probe_project.argtypes = [vp, i32]
        L.jpt_read_probe_sh_f32.argtypes = [vp, vp]
        L.jpt_debug_probe_rays.argtypes = [C.c_int, vp, i32, i32, i32, i32, u32, vp, vp, vp]
        L.jpt_debug_probe_basis.argtypes = [i32, i32, i32, vp]
        L.jpt_debug_probe_project.argtypes = [C.c_int, vp, u32, i32, i32, i32, i32, vp, vp]
    if hasattr(L, "jpt_set_reflection_probes") or "JPT_LIB" not in os.environ:
        L.jpt_set_reflection_probes.argtypes = [vp, vp, i32, i32, i32]
        L.jpt_get_reflection_image_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        L.jpt_read_reflection_probes.argtypes = [vp, vp]
        L.jpt_set_reflection_params.argtypes = [vp, C.POINTER(ReflectionParams)]
        L.jpt_reflection_prefilter.argtypes = [vp]
        L.jpt_get_reflection_chain_size.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(C.c_uint64)]
        L.jpt_read_reflection_f32.argtypes = [vp, i32, vp]
        L.jpt_get_reflection_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.jpt_debug_cube_rays.argtypes = [C.c_int, vp, i32, i32, i32, u32, vp]
        L.jpt_debug_reflection_samples.argtypes = [i32, i32, i32, i32, vp, vp]
        L.jpt_debug_reflection_prefilter.argtypes = [C.c_int, vp, u32, i32, i32, i32, C.POINTER(ReflectionParams), i32, vp]
    if hasattr(L, "jpt_denoise") or "JPT_LIB" not in os.environ:
        L.jpt_set_denoise_params.argtypes = [vp, C.POINTER(DenoiseParams)]
        L.jpt_denoise.argtypes = [vp]
        L.jpt_read_denoised_f32.argtypes = [vp, vp]
        L.jpt_read_denoised_rgba8.argtypes = [vp, vp]
        L.jpt_read_guides_f32.argtypes = [vp, vp, vp, vp]
        L.jpt_debug_atrous.argtypes = [C.c_int, i32, i32, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp]
    if hasattr(L, "jpt_set_denoise_variance") or "JPT_LIB" not in os.environ:
        L.jpt_set_denoise_variance.argtypes = [vp, C.POINTER(DenoiseVarianceParams)]
        L.jpt_read_denoised_variance_f32.argtypes = [vp, vp]
        L.jpt_debug_atrous_variance.argtypes = [C.c_int, i32, i32, C.POINTER(DenoiseParams), C.POINTER(DenoiseVarianceParams), vp, vp, u32, vp, vp, vp, vp, vp]
    if hasattr(L, "jpt_set_denoise_history") or "JPT_LIB" not in os.environ:
        L.jpt_set_denoise_history.argtypes = [vp, C.POINTER(DenoiseHistoryParams)]
        L.jpt_denoise_history_reset.argtypes = [vp]
        L.jpt_read_denoise_history_f32.argtypes = [vp, vp, vp]
        L.jpt_debug_denoise_history.argtypes = [C.c_int, i32, i32, C.POINTER(DenoiseParams), C.POINTER(DenoiseHistoryParams), vp, u32, vp, vp, vp, vp, i32,
                                                vp, vp, vp, vp, vp, vp]
    if hasattr(L, "jpt_display") or "JPT_LIB" not in os.environ:
        L.jpt_set_display_params.argtypes = [vp, C.POINTER(DisplayParams)]
        L.jpt_display.argtypes = [vp]
        L.jpt_read_display_rgba8.argtypes = [vp, vp]
        L.jpt_read_display_f32.argtypes = [vp, vp]
        L.jpt_debug_display.argtypes = [C.c_int, i32, i32, C.POINTER(DisplayParams), vp, vp, vp]
        L.jpt_debug_display_srgb_table.argtypes = [vp]
    if hasattr(L, "jpt_meter") or "JPT_LIB" not in os.environ:
        L.jpt_set_meter_params.argtypes = [vp, C.POINTER(MeterParams)]
        L.jpt_meter.argtypes = [vp]
        L.jpt_meter_reset.argtypes = [vp]
        L.jpt_read_meter.argtypes = [vp, C.POINTER(MeterResult), vp]
        L.jpt_set_auto_exposure.argtypes = [vp, i32]
        L.jpt_debug_meter.argtypes = [C.c_int, i32, i32, C.POINTER(MeterParams), vp, C.c_float, vp, C.POINTER(MeterResult)]
    if hasattr(L, "jpt_set_variance") or "JPT_LIB" not in os.environ:
        L.jpt_set_variance.argtypes = [vp, i32]
        L.jpt_read_variance_f32.argtypes = [vp, vp]
        L.jpt_device_variance.restype = vp
        L.jpt_device_variance.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.jpt_set_noise_params.argtypes = [vp, C.POINTER(NoiseParams)]
        L.jpt_noise_estimate.argtypes = [vp]
        L.jpt_read_noise.argtypes = [vp, C.POINTER(NoiseResult), vp]
        L.jpt_read_noise_tiles_f32.argtypes = [vp, vp]
        L.jpt_device_noise_tiles.restype = vp
        L.jpt_device_noise_tiles.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.jpt_render_converge.argtypes = [vp, i32, i32, u32, C.POINTER(i32), C.POINTER(NoiseResult)]
        L.jpt_debug_variance_moments.argtypes = [vp, i32, u32, i32, vp, vp, i32, i32]
        L.jpt_debug_noise_estimate.argtypes = [C.c_int, i32, i32, C.POINTER(NoiseParams), vp, vp, u32, vp, vp, vp, C.POINTER(NoiseResult)]
    if hasattr(L, "jpt_query_rays") or "JPT_LIB" not in os.environ:
        L.jpt_query_rays.argtypes = [vp, i32, vp, u32, vp, vp]
        L.jpt_query_rays_device.argtypes = [vp, i32, vp, u32, vp, vp]
        L.jpt_query_pixels.argtypes = [vp, vp, u32, vp]
    if hasattr(L, "jpt_scene_pose_mesh") or "JPT_LIB" not in os.environ:
        for n in ("jpt_scene_set_mesh_rig", "jpt_multi_set_mesh_rig"):
            getattr(L, n).argtypes = [vp, u32, C.POINTER(Surface), C.POINTER(SurfaceRig), i32, i32, i32]
        for n in ("jpt_scene_pose_mesh", "jpt_multi_pose_mesh"):
            getattr(L, n).argtypes = [vp, u32, vp, u32, vp, u32]
        L.jpt_scene_clear_mesh_rig.argtypes = [vp, u32]
        L.jpt_multi_clear_mesh_rig.argtypes = [vp, u32]
        L.jpt_debug_skin.argtypes = [C.c_int, vp, vp, u32, vp, vp, i32, vp, vp, i32, vp, u32, vp, vp, vp]
    if hasattr(L, "jpt_scene_rebuild_mesh") or "JPT_LIB" not in os.environ:
        for n in ("jpt_scene_rebuild_mesh", "jpt_multi_rebuild_mesh"):
            getattr(L, n).argtypes = [vp, u32, C.POINTER(Surface), i32]
        for n in ("jpt_scene_pose_mesh_rebuild", "jpt_multi_pose_mesh_rebuild"):
            getattr(L, n).argtypes = [vp, u32, vp, u32, vp, u32]
        L.jpt_debug_mesh_order.argtypes = [C.c_int, vp, u32, vp, u32, vp, vp]
    if hasattr(L, "jpt_encode") or "JPT_LIB" not in os.environ:
        L.jpt_encode.argtypes = [vp, i32, i32, i32]
        L.jpt_get_encoded_info.argtypes = [vp, C.POINTER(EncodedInfo)]
        L.jpt_read_encoded.argtypes = [vp, vp, C.c_size_t]
        L.jpt_readback_encoded_begin.argtypes = [vp]
        L.jpt_readback_encoded_end.argtypes = [vp, vp, C.c_size_t]
        L.jpt_device_encoded.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.jpt_device_encoded.restype = vp
        L.jpt_get_encode_timing.argtypes = [vp, C.POINTER(C.c_float)]
        L.jpt_debug_encode.argtypes = [C.c_int, vp, C.c_uint64, C.c_float, i32, i32, vp]
    if hasattr(L, "jpt_set_sky") or "JPT_LIB" not in os.environ:
        sp = C.POINTER(SkyParams)
        L.jpt_sky_defaults.argtypes = [sp]
        L.jpt_sky_defaults.restype = None
        L.jpt_set_sky.argtypes = [vp, sp, i32, i32, i32]
        L.jpt_read_environment_f32.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(i32)]
        L.jpt_multi_set_sky.argtypes = [vp, sp, i32, i32, i32]
        L.jpt_debug_sky.argtypes = [C.c_int, sp, i32, i32, i32, vp]
        L.jpt_debug_sky_radiance.argtypes = [sp, vp, u32, vp]
        L.jpt_debug_pow01.argtypes = [vp, vp, u32, vp]
    _lib = L
    return L


def check(ctx, rc: int, what: str):
    if rc != OK:
        msg = lib().jpt_last_error(ctx)
        raise JptError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
