"""The camera models on the CPU (jpt_set_camera_model, csrc/jpt_camera.h): the host's copy of the functions against the numpy
restatement (tests/np_camera.py) bit for bit, the geometry of both models in float64, the scene helper, the API on a host-only
context, and that the views the GPU tests render show both sky and geometry."""
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_camera as nc
import np_lens as nl
import np_path as npp
from test_lens_host import look_at, random_cameras

F = np.float32
EPS = 2.0 ** -23
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # JPT_E_* of include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAMERAS = (look_at((0.3, 0.5, 7.0), (0.0, 0.0, 0.0), fov=70.0), look_at((-4.0, 3.0, -2.5), (1.0, 0.5, 0.0), fov=35.0),
           look_at((2.0, -1.0, 0.5), (2.5, 4.0, -3.0), fov=100.0))
ORTHO_SIZES = (9.0, 3.0, 20.0)   # the vertical extent of the orthographic block of each of CAMERAS


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def camera_blocks(w, h, frame):
    """(name, block) of the three look-at cameras, each as a perspective and as an orthographic block"""
    out = []
    for k, cd in enumerate(CAMERAS):
        out.append(("perspective %d" % k, scenes.camera_block(cd, w, h, frame)))
        out.append(("orthogonal %d" % k, scenes.camera_block_orthogonal(cd, ORTHO_SIZES[k], w, h, frame)))
    return out


# ---- the views of the GPU tests (tests/test_gpu_camera.py) ----------------------------------------------------------------------------------

ORTHO_SIZE = 3.5          # an orthographic view this tall from the soup's +x side, a unit below its middle, is about half triangles, half sky
INSIDE = (0.0, 0.5, 0.0)  # the equirect camera stands inside the soup


def soup_scene():
    """test_gpu_lens.soup_scene: a small untextured soup seen from z = 7 down -z"""
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=14, textured=False, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    return sc


def soup_view(model, w, h, frame=0):
    """(scene, camera block) of the soup under `model`: PROJECTIVE the orthographic view from 7 units away, EQUIRECT the panorama from
    inside"""
    sc = soup_scene()
    if model == nc.EQUIRECT:
        sc.camera = scenes.CameraDesc(scenes.transform12(scenes.rot_y(25.0), INSIDE), fov_deg=70.0)
        return sc, scenes.camera_block(sc.camera, w, h, frame)
    turn = scenes.rot_y(90.0)
    sc.camera = scenes.CameraDesc(scenes.transform12(turn, tuple(turn @ np.array([0.0, -1.0, 7.0]))), fov_deg=70.0)
    return sc, scenes.camera_block_orthogonal(sc.camera, ORTHO_SIZE, w, h, frame)


# ---- 1. the host's functions equal numpy ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(32, 32), (33, 17)])
@pytest.mark.parametrize("model", [nc.PROJECTIVE, nc.EQUIRECT])
def test_host_ray_generation_equals_numpy(model, size):
    """jpt_debug_camera_rays on JPT_DEVICE_HOST_ONLY: camera_ray compiled for the host"""
    w, h = size
    for frame in (1, 78):
        for name, cam in camera_blocks(w, h, frame):
            o, d = host.debug_camera_rays(-1, cam, w, h, frame, model)
            _, wo, wd = nc.camera_rays(cam, w, h, model)
            assert np.array_equal(_u32(o).reshape(-1, 3), _u32(wo)) and np.array_equal(_u32(d).reshape(-1, 3), _u32(wd)), (name, frame)
            assert np.isfinite(o).all() and np.isfinite(d).all()
            pos = np.array([cam["position"][i] for i in range(3)], F)
            if model == nc.EQUIRECT:
                assert (o == pos).all()
            else:
                assert (o != pos).any(axis=-1).all()   # (the origins lie on the near plane)


@pytest.mark.parametrize("size", [(32, 32), (33, 17)])
def test_the_pinhole_model_is_primary_ray(size):
    w, h = size
    for frame in (1, 78):
        for name, cam in camera_blocks(w, h, frame):
            o, d = host.debug_camera_rays(-1, cam, w, h, frame, nc.PINHOLE)
            _, wo, wd = nl.pinhole_rays(cam, w, h)
            assert np.array_equal(_u32(o).reshape(-1, 3), _u32(wo)) and np.array_equal(_u32(d).reshape(-1, 3), _u32(wd)), (name, frame)
            lo, ld = host.debug_lens_rays(-1, cam, w, h, frame, 0.0, 1.0)
            assert np.array_equal(_u32(o), _u32(lo)) and np.array_equal(_u32(d), _u32(ld))


def test_the_models_keep_the_pinhole_seeds_and_the_map_convention():
    """the seeds after the jitter draw are np_lens.pinhole_rays's, and with the identity camera the centre ray of an equirect texel is
    the direction np_env looks that texel up by"""
    import np_env
    cam = scenes.camera_block(CAMERAS[1], 33, 17, 78)
    want = nl.pinhole_rays(cam, 33, 17)[0]
    for model in (nc.PROJECTIVE, nc.EQUIRECT):
        assert np.array_equal(nc.camera_rays(cam, 33, 17, model)[0], want)
    w, h = 16, 8
    ident = scenes.camera_block(scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 0.0))), w, h)
    f, r, u = nl.basis(ident)
    assert np.abs(np.stack([f, r, u]) - np.array([[0, 0, -1], [1, 0, 0], [0, 1, 0]], F)).max() <= 2.0 ** -23   # forward -z, right +x, up +y
    _, d = nc.centre_rays(ident, w, h, nc.EQUIRECT)
    rgb = np.arange(w * h * 3, dtype=F).reshape(h, w, 3)   # every texel its own value
    got = np_env.env_radiance(rgb, d)
    assert np.abs(got.reshape(h, w, 3) - rgb).max() < 1e-3   # (the lookup is bilinear: at a texel's centre, the texel to rounding)
    # row 0 is the up pole, the centre column forward, columns increase to the right
    d = d.reshape(h, w, 3).astype(np.float64)
    assert (d[0, :, 1] > 0.97).all() and (d[-1, :, 1] < -0.97).all()
    mid = nc.raster_rays(ident, w, h, nc.EQUIRECT, np.array([w / 2.0, w / 2.0 + 1.0], F), np.array([h / 2.0, h / 2.0], F))[1].astype(np.float64)
    assert np.abs(mid[0] - [0.0, 0.0, -1.0]).max() < 1e-6 and mid[1, 0] > 0.1


# ---- 2. geometry in float64 ---------------------------------------------------------------------------------------------------------------

GW, GH = 8192, 4096   # equirect: sin(theta) < 1e-3 is a band of 1e-3 / pi of the height at each pole, 1.3 of 4096 rows -- with the 10^4
                      # rays' rows stratified over the height (2.4 rays per row) that is 6 or 7 positions, under 0.1 % (asserted)


def basis64(cd):
    t = np.asarray(cd.transform, np.float64)
    b = t[:9].reshape(3, 3)
    return -b[:, 2], b[:, 0], b[:, 1], t[9:12]


def geometry_cases():
    """10^4 rays: 100 random look-at cameras x 100 random pixels each, the float32 restatement's rays examined in float64"""
    rng = np.random.default_rng(17)
    rows = {k: [] for k in ("ortho_angle", "ortho_plane", "ortho_offset", "persp_angle", "equi_offset", "equi_polar")}
    all_py = ((np.arange(10000) + rng.random(10000)) / 10000.0 * GH).astype(np.int64)   # one row per ray, stratified, dealt at random
    rng.shuffle(all_py)
    for k, cd in enumerate(random_cameras(100, 5)):
        f, r, u, pos = basis64(cd)
        frame = int(rng.integers(0, 1 << 16))
        px, py = rng.integers(0, GW, 100), all_py[100 * k:100 * k + 100]
        aspect = float(GW) / float(GH)
        # PROJECTIVE, an orthographic matrix
        size = float(rng.uniform(0.5, 30.0))
        cam = scenes.camera_block_orthogonal(cd, size, GW, GH, frame)
        _, fx, fy = nc.jitter(cam, GW, GH, px, py)
        o, d = (a.astype(np.float64) for a in nc.raster_rays(cam, GW, GH, nc.PROJECTIVE, fx, fy))
        nx, ny = fx.astype(np.float64) / GW * 2.0 - 1.0, -(fy.astype(np.float64) / GH * 2.0 - 1.0)
        exact = pos[None, :] + f[None, :] * cd.near + r[None, :] * (nx * size * aspect / 2.0)[:, None] + u[None, :] * (ny * size / 2.0)[:, None]
        # one ulp of the quantities an origin is made of: ivp's third column is half the view volume's depth and its fourth the
        # volume's centre, which the near-plane point is the difference of
        scale = EPS * (np.abs(pos).max() + size * aspect / 2.0 + (cd.far + cd.near) / 2.0)
        dn = d / np.linalg.norm(d, axis=1)[:, None]
        rows["ortho_angle"].append(np.linalg.norm(np.cross(dn, f[None, :]), axis=1) / EPS)
        rows["ortho_plane"].append(np.abs((o - pos[None, :]) @ f - cd.near) / scale)
        rows["ortho_offset"].append(np.linalg.norm(o - exact, axis=1) / scale)
        # PROJECTIVE, a perspective matrix: the pinhole's directions
        cam = scenes.camera_block(cd, GW, GH, frame)
        _, d = nc.raster_rays(cam, GW, GH, nc.PROJECTIVE, fx, fy)
        tan = np.tan(np.deg2rad(cd.fov_deg) / 2.0)
        want = f[None, :] + r[None, :] * (nx * tan * aspect)[:, None] + u[None, :] * (ny * tan)[:, None]
        want /= np.linalg.norm(want, axis=1)[:, None]
        dn = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)[:, None]
        rows["persp_angle"].append(np.linalg.norm(np.cross(dn, want), axis=1) / EPS)
        # EQUIRECT: the direction's (phi, theta) over the float64 basis, mapped back to the raster
        _, d = nc.raster_rays(cam, GW, GH, nc.EQUIRECT, fx, fy)
        d = d.astype(np.float64)
        mx, my, mz = d @ r, d @ u, d @ f
        sin_t = np.hypot(mx, mz)
        phi, theta = np.arctan2(mx, mz), np.arctan2(sin_t, my)
        bx, by = (phi / (2.0 * np.pi) + 0.5) * GW, theta / np.pi * GH
        ddx = np.abs(bx - fx.astype(np.float64))
        ddx = np.minimum(ddx, GW - ddx)   # (the seam: column W is column 0)
        rows["equi_offset"].append(np.hypot(ddx, by - fy.astype(np.float64)))
        rows["equi_polar"].append(sin_t < 1e-3)
    return {k: np.concatenate(v) for k, v in rows.items()}


# Measured on these inputs (the float32 restatement against the float64 recomputation above); each bound is twice the worst value.
# Orthographic: directions 1.414 eps from the camera's -z; origins 0.731 ulp off the near plane and 0.880 ulp from the raster
# position's exact point, an ulp being EPS * (|position|_max + half the width + (far + near) / 2).  PROJECTIVE under a perspective
# matrix: 82.8 eps from the float64 pinhole direction (the far-plane point divides by a w that all but cancels, far / near = 4000;
# primary_ray's unprojection carries the same error).  EQUIRECT: 2.08 pixels of an 8192 x 4096 image from the jittered raster
# position, reached next to the polar band (longitude is worth 1 / sin(theta): up to 1000 times the direction's error there), 5 of
# the 10^4 positions polar and left out.
ORTHO_ANGLE_EPS, ORTHO_PLANE_ULPS, ORTHO_OFFSET_ULPS, PERSP_ANGLE_EPS, EQUI_OFFSET_PX = 2.83, 1.47, 1.76, 165.6, 4.15


@pytest.fixture(scope="module")
def geometry():
    return geometry_cases()


def test_orthographic_rays_are_parallel_and_start_on_the_near_plane(geometry):
    g = geometry
    assert len(g["ortho_angle"]) == 10000
    print("orthographic: angle %.3f eps, plane %.3f ulp, offset %.3f ulp" % (g["ortho_angle"].max(), g["ortho_plane"].max(), g["ortho_offset"].max()))
    assert g["ortho_angle"].max() <= ORTHO_ANGLE_EPS
    assert g["ortho_plane"].max() <= ORTHO_PLANE_ULPS
    assert g["ortho_offset"].max() <= ORTHO_OFFSET_ULPS


def test_projective_rays_of_a_perspective_matrix_are_the_pinhole_directions(geometry):
    print("perspective: angle %.3f eps" % geometry["persp_angle"].max())
    assert len(geometry["persp_angle"]) == 10000 and geometry["persp_angle"].max() <= PERSP_ANGLE_EPS


def test_equirect_directions_map_back_to_their_raster_positions(geometry):
    g = geometry
    polar = g["equi_polar"]
    print("equirect: offset %.3e px, %d polar positions left out" % (g["equi_offset"][~polar].max(), int(polar.sum())))
    assert polar.mean() < 1e-3, polar.mean()
    assert g["equi_offset"][~polar].max() <= EQUI_OFFSET_PX


def test_orthogonal_is_godots_matrix():
    p = scenes.orthogonal(6.0, 1.5, 0.05, 200.0)
    want = np.zeros((4, 4))
    want[0, 0], want[1, 1], want[2, 2], want[2, 3], want[3, 3] = 2.0 / 9.0, 2.0 / 6.0, -2.0 / 199.95, -200.05 / 199.95, 1.0
    assert np.allclose(p, want, rtol=1e-15, atol=0.0)
    # the corners of the view volume: x = +-size * aspect / 2, y = +-size / 2, z = -near and -far go to the NDC cube's corners
    for x, y, z, ndc in ((4.5, 3.0, -0.05, (1, 1, -1)), (-4.5, -3.0, -200.0, (-1, -1, 1))):
        c = p @ np.array([x, y, z, 1.0])
        assert np.allclose(c[:3] / c[3], ndc, atol=1e-12)
    cd = CAMERAS[1]
    blk = scenes.camera_block_orthogonal(cd, 6.0, 48, 32, 9)
    assert blk["frame_index"] == 9 and blk["near"] == F(cd.near) and blk["far"] == F(cd.far)
    assert np.allclose(blk["vp"].reshape(4, 4).T.astype(np.float64) @ blk["ivp"].reshape(4, 4).T.astype(np.float64), np.eye(4), atol=1e-4)


# ---- 3. the API ---------------------------------------------------------------------------------------------------------------------------

def test_set_camera_model_checks_its_argument_on_a_host_only_context():
    L = capi.lib()
    assert hasattr(L, "jpt_set_camera_model") and hasattr(L, "jpt_multi_set_camera_model") and hasattr(L, "jpt_debug_camera_rays")
    assert L.jpt_abi_version() == 6
    assert (capi.CAMERA_PINHOLE, capi.CAMERA_PROJECTIVE, capi.CAMERA_EQUIRECT) == (0, 1, 2)
    ctx = host.Context(-1)
    try:
        for model in (-1, 3, 1 << 20):
            assert L.jpt_set_camera_model(ctx.h, model) == E_INVALID, model
            assert b"jpt_set_camera_model" in L.jpt_last_error(ctx.h)
        for model in (capi.CAMERA_PINHOLE, capi.CAMERA_PROJECTIVE, capi.CAMERA_EQUIRECT):
            assert L.jpt_set_camera_model(ctx.h, model) == E_DEVICE, model
        with pytest.raises(capi.JptError):
            ctx.set_camera_model(capi.CAMERA_EQUIRECT)
    finally:
        ctx.close()
    assert L.jpt_set_camera_model(None, 0) == E_INVALID and L.jpt_multi_set_camera_model(None, 0) == E_INVALID


def test_the_header_declares_the_enum_and_the_calls():
    text = open(os.path.join(ROOT, "include", "jpt.h")).read()
    m = re.search(r"enum\s*\{\s*JPT_CAMERA_PINHOLE\s*=\s*(\d+),\s*JPT_CAMERA_PROJECTIVE\s*=\s*(\d+),\s*JPT_CAMERA_EQUIRECT\s*=\s*(\d+)\s*\}", text)
    assert m and tuple(int(x) for x in m.groups()) == (capi.CAMERA_PINHOLE, capi.CAMERA_PROJECTIVE, capi.CAMERA_EQUIRECT)
    assert re.search(r"int jpt_set_camera_model\(jpt_ctx \*ctx, int32_t model\);", text)
    assert re.search(r"int jpt_multi_set_camera_model\(jpt_multi \*m, int32_t model\);", text)
    assert re.search(r"#define JPT_ABI_VERSION 6\b", text)


def test_state_errors_of_the_ray_generation_on_the_host():
    """what a render refuses with JPT_E_STATE, where a host-only call reaches it: EQUIRECT with a basis that is not finite, PROJECTIVE
    with an ivp that is not finite; and the argument checks of the mirror"""
    cam = scenes.camera_block(CAMERAS[0], 8, 8)
    singular = cam.copy()
    singular["ivp"] = 0.0
    L = capi.lib()
    buf = np.zeros((8, 8, 3), F)
    ptr = host._ptr(buf)
    assert L.jpt_debug_camera_rays(-1, singular.tobytes(), 8, 8, 0, capi.CAMERA_EQUIRECT, ptr, ptr) == E_STATE
    assert b"not finite" in L.jpt_debug_last_error()
    host.debug_camera_rays(-1, singular, 8, 8, 0, capi.CAMERA_PINHOLE)   # (the pinhole is not treated specially: whatever it gives)
    for bad in (float("nan"), float("inf")):
        nonfinite = cam.copy()
        ivp = nonfinite["ivp"].copy()
        ivp.reshape(-1)[5] = bad
        nonfinite["ivp"] = ivp
        assert L.jpt_debug_camera_rays(-1, nonfinite.tobytes(), 8, 8, 0, capi.CAMERA_PROJECTIVE, ptr, ptr) == E_STATE
        assert b"ivp" in L.jpt_debug_last_error()
    # a singular but finite ivp under PROJECTIVE is not treated specially: the rays are whatever the arithmetic gives, as numpy's are
    o, d = host.debug_camera_rays(-1, singular, 8, 8, 0, capi.CAMERA_PROJECTIVE)
    _, wo, wd = nc.camera_rays(singular, 8, 8, nc.PROJECTIVE)
    assert np.isnan(o).all() and np.isnan(wo).all() and np.isnan(d).all() and np.isnan(wd).all()
    with pytest.raises(capi.JptError, match="model must be"):
        host.debug_camera_rays(-1, cam, 8, 8, 0, 3)
    with pytest.raises(capi.JptError, match="width and height"):
        host.debug_camera_rays(-1, cam, 0, 8, 0, capi.CAMERA_PROJECTIVE)


# ---- 4. pictures worth testing ----------------------------------------------------------------------------------------------------------------

def test_the_views_of_the_gpu_tests_show_sky_and_geometry(oracle):
    """the orthographic soup view holds at least 25 % sky and 25 % hits, the equirect view from inside the soup at least 10 % of each:
    the GPU tests cannot pass on an empty frame"""
    for model, least in ((nc.PROJECTIVE, 0.25), (nc.EQUIRECT, 0.10)):
        for w, h in ((32, 32), (33, 17)):
            sc, cam = soup_view(model, w, h, 1)
            ref = oracle.build_scene(sc)
            _, o, d = nc.camera_rays(cam, w, h, model)
            with np.errstate(all="ignore"):
                hit = npp._closest_hit(ref, o, d)[0] < F(1e9)
            print("model %d %dx%d: %.1f %% hits" % (model, w, h, 100.0 * hit.mean()))
            assert hit.mean() >= least and (~hit).mean() >= least, (model, w, h, hit.mean())
