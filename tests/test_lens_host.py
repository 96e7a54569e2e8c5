"""The thin-lens camera on the CPU (jpt_set_lens, csrc/jpt_lens.h): the host's copy of the functions against the numpy restatement
(tests/np_lens.py) bit for bit, the geometry and the disk's uniformity in float64, the scene helper, and the API on a host-only
context."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_lens as nl

F = np.float32
EPS = 2.0 ** -23
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # JPT_E_* of include/jpt.h


def look_at(pos, target, up=(0.0, 1.0, 0.0), fov=60.0, near=0.05, far=200.0):
    """a Godot camera at `pos` looking at `target` (its -z axis points there)"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = pos - target
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return scenes.CameraDesc(scenes.transform12(np.stack([x, y, z], axis=1), tuple(pos)), fov_deg=fov, near=near, far=far)


def random_cameras(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pos = rng.uniform(-5.0, 5.0, 3)
        target = pos + rng.standard_normal(3) * 3.0 + np.array([0.0, 0.0, -1e-3])
        d = target - pos
        if abs(d[1]) > 0.95 * np.linalg.norm(d):   # (not along the up axis)
            target[0] += 2.0
        out.append(look_at(pos, target, fov=float(rng.uniform(25.0, 100.0))))
    return out


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. the host's functions equal numpy ------------------------------------------------------------------------------------------------

def test_host_ray_generation_equals_numpy():
    """jpt_debug_lens_rays on JPT_DEVICE_HOST_ONLY: primary_ray and lens_ray compiled for the host"""
    rng = np.random.default_rng(11)
    for k, cd in enumerate(random_cameras(6, 1)):
        w, h = (33, 17) if k % 2 else (32, 32)
        frame = int(rng.integers(0, 1 << 20))
        cam = scenes.camera_block(cd, w, h, frame)
        radius, focus = float(rng.uniform(0.01, 0.5)), float(rng.uniform(0.5, 20.0))
        for r in (0.0, radius):
            o, d = host.debug_lens_rays(-1, cam, w, h, frame, r, focus)
            _, wo, wd = nl.lens_rays(cam, w, h, r, focus)
            assert np.array_equal(_u32(o).reshape(-1, 3), _u32(wo)) and np.array_equal(_u32(d).reshape(-1, 3), _u32(wd)), (k, r)
        o0, d0 = host.debug_lens_rays(-1, cam, w, h, frame, 0.0, focus)
        assert (o0 == np.array([cam["position"][i] for i in range(3)], F)).all()
        assert (o != o0).any(axis=-1).mean() > 0.99 and (d != d0).any(axis=-1).mean() > 0.99


def corner_rays():
    """(o, d, xi) rows: xi0 = 0, the largest xi0 (the largest pcg2d float, 2^32 - 1 scaled and rounded: 1.0) and the largest below 1,
    xi1 at both ends, a ray at right angles to the axis (cf = 0 for the axis-aligned camera), one pointing backwards, one grazing"""
    top = F(4294967295.0) * F(2.32830643654e-10)
    xis = [(0.0, 0.3), (float(top), 0.7), (0.99999994, 0.0), (0.5, float(top)), (0.25, 0.25), (1e-38, 0.5)]
    dirs = [(0.0, 0.0, -1.0), (0.6, 0.0, -0.8), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.6, 0.8), (0.99999994, 0.0, -3.4e-4)]
    o, d, xi = [], [], []
    for x in xis:
        for dd in dirs:
            o.append((0.25, 1.5, 3.0))
            d.append(dd)
            xi.append(x)
    return np.array(o, F), np.array(d, F), np.array(xi, F)


@pytest.mark.parametrize("radius", [0.0, 0.3])
def test_host_lens_step_equals_numpy_on_corner_cases(radius):
    """jpt_debug_lens_sample: lens_basis and lens_apply compiled for the host, on caller-made randoms"""
    cd = scenes.CameraDesc(scenes.transform12(None, (0.25, 1.5, 3.0)), fov_deg=70.0)   # axis-aligned: f = -z exactly
    cam = scenes.camera_block(cd, 32, 32)
    o, d, xi = corner_rays()
    go, gd, gb = host.debug_lens_sample(cam, radius, 2.5, o, d, xi)
    bas = nl.basis(cam)
    wo, wd = nl.lens_apply(bas, radius, 2.5, o, d, xi)
    assert np.array_equal(_u32(gb), _u32(np.stack(bas)))
    assert np.array_equal(_u32(go), _u32(wo)) and np.array_equal(_u32(gd), _u32(wd))
    cf = d @ bas[0]
    kept = ~(cf > 0)
    assert kept.any() and (~kept).any()
    assert np.array_equal(_u32(go[kept]), _u32(o[kept])) and np.array_equal(_u32(gd[kept]), _u32(d[kept]))   # cf <= 0: the pinhole ray
    if radius == 0.0:
        assert np.array_equal(_u32(go), _u32(o))   # radius 0 through the step: the origin stays, bit for bit
    assert np.isfinite(go).all() and np.isfinite(gd).all()


def test_host_basis_over_random_and_near_singular_cameras():
    for cd in random_cameras(40, 2):
        cam = scenes.camera_block(cd, 48, 32)
        _, _, gb = host.debug_lens_sample(cam, 0.1, 1.0, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 2), F))
        assert np.array_equal(_u32(gb), _u32(np.stack(nl.basis(cam))))
        # a Godot camera: forward -z, right +x, up +y of its transform
        t = np.asarray(cd.transform, np.float64)[:9].reshape(3, 3)
        assert np.abs(gb[0] + t[:, 2]).max() < 1e-5 and np.abs(gb[1] - t[:, 0]).max() < 1e-5 and np.abs(gb[2] - t[:, 1]).max() < 1e-5
    # a near-singular ivp (far / near = 1e9: its w row all but cancels) still equals numpy, whatever it gives
    cam = scenes.camera_block(scenes.CameraDesc(scenes.transform12(scenes.rot_y(40.0), (1.0, 2.0, 3.0)), fov_deg=1.0, near=1e-5, far=1e4), 32, 32)
    o, d, xi = corner_rays()
    try:
        go, gd, gb = host.debug_lens_sample(cam, 0.2, 3.0, o, d, xi)
    except capi.JptError:
        assert not np.isfinite(np.stack(nl.basis(cam))).all()
    else:
        bas = nl.basis(cam)
        wo, wd = nl.lens_apply(bas, 0.2, 3.0, o, d, xi)
        assert np.array_equal(_u32(gb), _u32(np.stack(bas))) and np.array_equal(_u32(go), _u32(wo)) and np.array_equal(_u32(gd), _u32(wd))
    # a singular one (ivp of zeros): no finite basis, and the entry says so
    bad = cam.copy()
    bad["ivp"] = 0.0
    assert not np.isfinite(np.stack(nl.basis(bad))).all()
    with pytest.raises(capi.JptError, match="not finite"):
        host.debug_lens_sample(bad, 0.2, 3.0, o, d, xi)
    with pytest.raises(capi.JptError, match="not finite"):
        host.debug_lens_rays(-1, bad, 8, 8, 0, 0.2, 3.0)


# ---- 2. geometry and uniformity in float64 ------------------------------------------------------------------------------------------------

def basis64(cd):
    t = np.asarray(cd.transform, np.float64)
    b = t[:9].reshape(3, 3)
    return -b[:, 2], b[:, 0], b[:, 1], t[9:12]


def geometry_cases():
    """10^4 rays: 100 random look-at cameras x one 10 x 10 frame each, the float32 restatement's rays examined in float64"""
    rng = np.random.default_rng(7)
    rows = {"miss_ratio": [], "plane_ratio": [], "radius_ratio": [], "lens_uv": []}
    for cd in random_cameras(100, 3):
        radius, focus = float(rng.uniform(0.01, 0.5)), float(rng.uniform(0.5, 20.0))
        cam = scenes.camera_block(cd, 10, 10, int(rng.integers(0, 1 << 16)))
        _, o, d = nl.pinhole_rays(cam, 10, 10)
        _, o2, d2 = nl.lens_rays(cam, 10, 10, radius, focus)
        f, r, u, pos = basis64(cd)
        pos32 = np.array([cam["position"][k] for k in range(3)], F).astype(np.float64)
        o, d, o2, d2 = (a.astype(np.float64) for a in (o, d, o2, d2))
        tf = focus / (d @ f)
        p = o + d * tf[:, None]                      # where the pinhole ray meets the focal plane
        rel = p - o2
        dn = d2 / np.linalg.norm(d2, axis=1)[:, None]
        miss = np.linalg.norm(rel - dn * (rel * dn).sum(axis=1)[:, None], axis=1)
        scale = EPS * (np.abs(pos32).max() + tf)      # one ulp of the quantities p and o2 are made of
        off = o2 - pos32
        rows["miss_ratio"].append(miss / scale)
        rows["plane_ratio"].append(np.abs(off @ f) / (EPS * (np.abs(pos32).max() + radius)))
        rows["radius_ratio"].append((np.linalg.norm(off, axis=1) - radius) / (EPS * (np.abs(pos32).max() + radius)))
        rows["lens_uv"].append(np.stack([off @ r, off @ u], axis=1) / radius)
    return {k: np.concatenate(v) for k, v in rows.items()}


# Measured on these inputs (the float32 restatement against the float64 recomputation above), in units of EPS * (|position|_max +
# extent), extent the distance to the focal point or the radius: the largest miss of the focal point 3.43, the largest distance
# from the lens plane 6.10 (the float32 basis is orthonormal to a few ulp, and the plane is the float64 one).  Those two bounds keep a
# margin of about 4x.  No origin was outside the radius (the largest excess was negative); that bound is the rounding of the two
# sums that make the origin, at most 2 ulp of the magnitude, with a margin of 2x.
MISS_ULPS, PLANE_ULPS, RADIUS_ULPS = 14.0, 24.0, 4.0


@pytest.fixture(scope="module")
def geometry():
    return geometry_cases()


def test_lens_rays_start_on_the_disk_and_pass_through_the_focal_point(geometry):
    g = geometry
    assert len(g["miss_ratio"]) == 10000
    print("largest miss %.3f, plane %.3f, radius excess %.3f (units of eps x magnitude)" % (g["miss_ratio"].max(), g["plane_ratio"].max(), g["radius_ratio"].max()))
    assert g["plane_ratio"].max() <= PLANE_ULPS
    assert g["radius_ratio"].max() <= RADIUS_ULPS
    assert g["miss_ratio"].max() <= MISS_ULPS


def test_lens_points_are_uniform_on_the_disk(geometry):
    uv = geometry["lens_uv"]
    n = len(uv)
    # a uniform disk of radius 1: mean 0, var(x) = 1/4; r^2 uniform on [0, 1]: mean 1/2, var 1/12
    se_mean, se_r2 = np.sqrt(0.25 / n), np.sqrt(1.0 / 12.0 / n)
    r2 = (uv ** 2).sum(axis=1)
    print("mean %s (se %.4f), mean r^2 %.5f (se %.4f)" % (uv.mean(axis=0), se_mean, r2.mean(), se_r2))
    assert (np.abs(uv.mean(axis=0)) <= 4.0 * se_mean).all()
    assert abs(r2.mean() - 0.5) <= 4.0 * se_r2


def test_lens_from_physical():
    r, d = scenes.lens_from_physical(50.0, 2.0, 3.5)
    assert r == pytest.approx(0.0125) and d == 3.5
    assert scenes.lens_from_physical(35.0, 16.0, 10.0)[0] == pytest.approx(0.035 / 32.0)
    with pytest.raises(ValueError):
        scenes.lens_from_physical(50.0, 0.0, 1.0)


# ---- 3. the API on a host-only context ----------------------------------------------------------------------------------------------------

def test_set_lens_checks_its_arguments_on_a_host_only_context():
    L = capi.lib()
    assert hasattr(L, "jpt_multi_set_lens") and hasattr(L, "jpt_set_lens") and hasattr(L, "jpt_debug_lens_rays")
    assert L.jpt_abi_version() == 6
    ctx = host.Context(-1)
    try:
        for radius, focus in ((float("nan"), 1.0), (float("inf"), 1.0), (-0.1, 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan")), (0.1, float("inf")),
                              (0.0, float("nan"))):
            assert L.jpt_set_lens(ctx.h, radius, focus) == E_INVALID, (radius, focus)
            assert b"jpt_set_lens" in L.jpt_last_error(ctx.h)
        for radius, focus in ((0.0, 1.0), (0.25, 3.0), (0.0, 0.0)):
            assert L.jpt_set_lens(ctx.h, radius, focus) == E_DEVICE, (radius, focus)
        with pytest.raises(capi.JptError):
            ctx.set_lens(0.1, 2.0)
    finally:
        ctx.close()
    cam = scenes.camera_block(scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 5.0))), 8, 8)
    with pytest.raises(capi.JptError, match="aperture_radius"):
        host.debug_lens_rays(-1, cam, 8, 8, 0, -1.0, 1.0)
    with pytest.raises(capi.JptError, match="focus_distance"):
        host.debug_lens_rays(-1, cam, 8, 8, 0, 0.5, 0.0)


def test_np_transmission_takes_the_lens_rays_of_np_lens(oracle):
    """np_transmission.trace_tx(lens=...) against np_lens.trace_frame, which the device's lens renders are checked with: under the
    sky, with no transmissive material and no texture, the two are one path tracer.  lens=None and radius 0 are the pinhole."""
    import np_transmission as ntx
    sc = scenes.random_scene(3, n_meshes=3, n_instances=5, tris_per_surface=14, textured=False, coincident=False)
    sc.camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.5, 7.0)), fov_deg=70.0)
    ref = oracle.build_scene(sc)
    w, h = 24, 16
    cam = scenes.camera_block(sc.camera, w, h).copy()
    cam["frame_index"] = 3
    lens = (0.25, 6.5)
    want = nl.trace_frame(ref, cam, w, h, 4, *lens)[0]
    got = ntx.trace_tx(ref, cam, w, h, 4, capi.MATERIAL_EXT_TRANSMISSION, lens=lens)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pin = ntx.trace_tx(ref, cam, w, h, 4, capi.MATERIAL_EXT_TRANSMISSION)
    assert np.array_equal(ntx.trace_tx(ref, cam, w, h, 4, capi.MATERIAL_EXT_TRANSMISSION, lens=(0.0, 6.5)).view(np.uint32), pin.view(np.uint32))
    assert np.array_equal(pin.view(np.uint32), nl.trace_frame(ref, cam, w, h, 4, 0.0, 1.0)[0].view(np.uint32))
    assert (got != pin).any(axis=-1).mean() > 0.03
