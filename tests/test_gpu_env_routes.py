"""The environment map and its importance sampling on the routes that decide hits exactly: reach records, the paths set aside
and finished by wf2_finish_env / wf2_finish_mis, exact ties re-decided on the reference's own trees (the tie walk's overflow
included), one TLAS-update step, and the set-aside buffer's overflow rule; then MIS at full size on every route.  The audit kernel
never sets a path aside, so it is the yardstick of the small scenes (the default-sky suite ties it to the oracle there)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

from test_fuzz import SEEDS, forty_coincident_copies
from test_gpu_env_sampling import BRDF, MIS, ROT, make_ctx, sun_map
from test_gpu_environment import assert_same, images
from test_gpu_parity import _moved, _moves_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("commit", "upload", "exact", "audit")   # as test_instance_of_an_empty_mesh_shows_what_the_reference_shows names them


def _route_ctx(route, sc, ref, w, h, bounces, accum, mode):
    """commit: BUILD_SAH, wavefront; upload: upload_reference_layout, wavefront; exact: BUILD_REFERENCE_EXACT, wavefront;
    audit: BUILD_SAH, KERNEL_REFERENCE_LAYOUT -- each with sun_map under ROT in the given map mode"""
    if route != "upload":
        kernel = capi.KERNEL_REFERENCE_LAYOUT if route == "audit" else capi.KERNEL_WAVEFRONT
        builder = capi.BUILD_REFERENCE_EXACT if route == "exact" else capi.BUILD_SAH
        return make_ctx(sc, w, h, builder, accum, bounces, kernel, sun_map(), ROT, 1.3, mode)
    ctx = host.Context(0)
    try:
        ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        ctx.set_environment(sun_map())
        ctx.set_environment_params(ROT, 1.3)
        ctx.set_environment_sampling(mode)
    except Exception:
        ctx.close()
        raise
    return ctx


def _differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


def _all_routes(oracle, sc, mode, what, min_aside=1, step=None):
    """96 x 64, 3 bounces, 2 frames on the four routes, HDR and LDR8 accumulation: every route's accumulation and display equal
    the audit kernel's bit for bit (NaNs in the same places), and the commit route set paths aside and dropped none.
    step(ctx, route), if given, runs between a first render and the compared one (the accumulation is reset after it)."""
    w, h, bounces, frames = 96, 64, 3, 2
    ref = oracle.build_scene(sc)
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        out, st = {}, {}
        for route in ROUTES:
            ctx = _route_ctx(route, sc, ref, w, h, bounces, accum, mode)
            try:
                ctx.render(frames, 1)
                if step is not None:
                    step(ctx, route)
                    ctx.accum_reset()
                    ctx.render(frames, 1)
                out[route], st[route] = images(ctx)[:2], ctx.stats()
            finally:
                ctx.close()
        print("%s, mode %d, accum %d: set aside / dropped %s, pixels differing from the audit kernel's %s" % (
            what, mode, accum, {r: (st[r]["set_aside"], st[r]["set_aside_dropped"]) for r in ROUTES},
            {r: _differing(out[r][0], out["audit"][0]) for r in ROUTES[:-1]}))
        for route in ROUTES[:-1]:
            assert_same(out[route], out["audit"], "%s, mode %d, accum %d, route %s" % (what, mode, accum, route))
        assert st["commit"]["set_aside"] >= min_aside and st["commit"]["set_aside_dropped"] == 0, st["commit"]


# ---- 1. the map and MIS on the exactness routes ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [BRDF, MIS])
@pytest.mark.parametrize("seed", SEEDS)
def test_coincident_soup_under_a_map_is_the_same_on_every_route(oracle, hiplib, seed, mode):
    _all_routes(oracle, scenes.random_scene(seed, coincident=True), mode, "coincident soup %d" % seed)


@pytest.mark.parametrize("mode", [BRDF, MIS])
def test_forty_coincident_copies_under_a_map_are_the_same_on_every_route(oracle, hiplib, mode):
    """the tie walk's overflow: vertices decided by the reference's whole walk of its own trees, inside wf2_finish_*"""
    _all_routes(oracle, forty_coincident_copies(), mode, "forty coincident copies", min_aside=301)


@pytest.mark.parametrize("mode", [BRDF, MIS])
@pytest.mark.parametrize("seed", [1, 4])
def test_moved_coincident_soup_under_a_map_is_the_same_on_every_route(oracle, hiplib, seed, mode):
    """one TLAS-update step (jpt_scene_update_tlas; jpt_scene_update_reference_tlas on the upload route) of the soup of
    test_exact_ties_stay_decided_after_instances_move"""
    sc = scenes.random_scene(seed, coincident=True)
    moves = _moves_for(sc, 11 + seed, 4)
    r1 = oracle.build_scene(_moved(sc, moves))

    def step(ctx, route):
        if route == "upload":
            ctx.update_reference_tlas(r1.instances, r1.tlas_nodes)
        else:
            for i, t in moves.items():
                ctx.set_instance_transform(i, t)
            ctx.update_tlas()
    _all_routes(oracle, sc, mode, "moved coincident soup %d" % seed, step=step)


# ---- 2. the set-aside buffer's overflow under a map --------------------------------------------------------------------------

CHILD = r'''
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from gdpathtracing_amd import capi, scenes
from test_gpu_env_sampling import make_ctx, sun_map, ROT
mode = int(sys.argv[2])
sc = scenes.demo_scene(51200); w, h = 1280, 720
img = {}
for name, builder in (("reach", capi.BUILD_SAH), ("watertight", capi.BUILD_SAH_WATERTIGHT)):
    ctx = make_ctx(sc, w, h, builder, capi.ACCUM_HDR_F32, 3, env=sun_map(256, 512), rot=ROT, intensity=3.0, mode=mode)
    ctx.render(4, 1)
    img[name] = ctx.read_accum(); st = ctx.stats()
    if name == "reach": aside, dropped = st["set_aside"], st["set_aside_dropped"]
    ctx.close()
a, b = img["reach"], img["watertight"]
differing = int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())
print(json.dumps(dict(aside=int(aside), dropped=int(dropped), differing=differing)))
'''


@pytest.mark.parametrize("mode", [BRDF, MIS])
def test_set_aside_overflow_under_a_map_is_counted_not_silent(hiplib, mode):
    """test_set_aside_buffer_overflow_is_counted_not_silent under a map: config C2 (1280x720, 4 spp, 3 bounces), whose reference
    tree has a crack at pixel (688, 551).  The default capacity drops no set-aside path; with the capacity forced to 0 every one
    is counted as dropped and shaded as found, and the image is the watertight builder's bit for bit."""
    res = {}
    for cap in (None, "0"):
        env = dict(os.environ)
        if cap is not None:
            env["JPT_SET_ASIDE_CAP"] = cap
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(mode)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[cap] = json.loads(r.stdout.strip().splitlines()[-1])
    print("C2 under a map, mode %d: set-aside hits %s" % (mode, res))
    assert res[None]["aside"] >= 1 and res[None]["dropped"] == 0
    assert res["0"]["dropped"] == res["0"]["aside"] >= 1
    assert res["0"]["differing"] == 0


# ---- 3. MIS at full size, every route ------------------------------------------------------------------------------------------

def test_mis_full_size_is_the_same_on_every_route(hiplib):
    """demo_scene at 1920 x 1080, 8 frames, 4 bounces, LDR8, under a sun at intensity 3 with MIS: both kernels on the native
    tree with reach records and on the reference-exact tree give one image.  A shadow ray is blocked when some triangle's test
    accepts it (the brute-force answer), whichever tree the route walks."""
    sc = scenes.demo_scene()
    w, h = 1920, 1080
    rgb = sun_map(512, 1024)
    out = {}
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        for builder in (capi.BUILD_SAH, capi.BUILD_REFERENCE_EXACT):
            ctx = make_ctx(sc, w, h, builder, capi.ACCUM_REF_LDR8, 4, kernel, rgb, ROT, 3.0, MIS)
            try:
                ctx.render(8, 1)
                out[(kernel, builder)] = images(ctx)
            finally:
                ctx.close()
    first = (capi.KERNEL_WAVEFRONT, capi.BUILD_SAH)
    print("MIS full size, pixels differing from the wavefront kernel's on BUILD_SAH, per (kernel, builder):",
          {k: _differing(v[0], out[first][0]) for k, v in out.items()})
    for k, v in out.items():
        assert_same(v, out[first], "kernel %d, builder %d" % k)
