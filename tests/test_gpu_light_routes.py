"""Light sampling (JPT_LIGHT_SAMPLING_MIS) on the routes that decide hits exactly: reach records, the paths set aside and finished
by wf2_finish_lt (its inline shadow rays), exact ties re-decided on the reference's own trees, alone and with the map's MIS; then
at full size on both kernels.  The emitter list follows the scene's triangle order, which the native builders choose for
themselves (an upload of the reference layout builds a native tree too): routes are compared within one layout, each wavefront
render against the audit kernel's render of the same scene."""
import pytest

from gdpathtracing_amd import capi, host, scenes

from test_fuzz import forty_coincident_copies
from test_gpu_environment import assert_same, images
from test_gpu_light_sampling import LMIS, make_ctx, sun_map

pytestmark = pytest.mark.gpu


def _route_ctx(route, sc, ref, w, h, bounces, accum, env):
    rgb = sun_map() if env == "map_mis" else None
    if not route.startswith("upload"):
        kernel = capi.KERNEL_REFERENCE_LAYOUT if route.endswith("audit") else capi.KERNEL_WAVEFRONT
        builder = capi.BUILD_SAH if route.startswith("commit") else capi.BUILD_REFERENCE_EXACT
        return make_ctx(sc, w, h, builder, accum, bounces, kernel, rgb, env == "map_mis")
    ctx = host.Context(0)
    try:
        ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT if route.endswith("audit") else capi.KERNEL_WAVEFRONT)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        if rgb is not None:
            ctx.set_environment(rgb)
            ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
        ctx.set_light_sampling(LMIS)
    except Exception:
        ctx.close()
        raise
    return ctx


GROUPS = (("commit", "commit_audit"), ("exact", "exact_audit"), ("upload", "upload_audit"))


def _all_routes(oracle, sc, env, what, min_aside=1):
    w, h, bounces, frames = 96, 64, 3, 2
    ref = oracle.build_scene(sc)
    for accum in (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8):
        out, st = {}, {}
        for group in GROUPS:
            for route in group:
                ctx = _route_ctx(route, sc, ref, w, h, bounces, accum, env)
                try:
                    ctx.render(frames, 1)
                    out[route], st[route] = images(ctx)[:2], ctx.stats()
                finally:
                    ctx.close()
        print("%s, %s, accum %d: set aside / dropped %s" % (what, env, accum, {r: (st[r]["set_aside"], st[r]["set_aside_dropped"]) for r in out}))
        for group in GROUPS:
            for route in group[:-1]:
                assert_same(out[route], out[group[-1]], "%s, %s, accum %d, route %s" % (what, env, accum, route))
        assert st["commit"]["set_aside"] >= min_aside and st["commit"]["set_aside_dropped"] == 0, st["commit"]


@pytest.mark.parametrize("env", ["sky", "map_mis"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_coincident_soup_with_light_sampling_is_the_same_on_every_route(oracle, hiplib, seed, env):
    _all_routes(oracle, scenes.random_scene(seed, coincident=True), env, "coincident soup %d" % seed)


@pytest.mark.parametrize("env", ["sky", "map_mis"])
def test_forty_coincident_copies_with_light_sampling_are_the_same_on_every_route(oracle, hiplib, env):
    _all_routes(oracle, forty_coincident_copies(), env, "forty coincident copies", min_aside=301)


def test_light_sampling_full_size_is_the_same_on_both_kernels(hiplib):
    """demo_scene (its 51 200-triangle emissive blob and the light quad) at 1920 x 1080, 8 frames, 4 bounces, LDR8: the wavefront
    and audit kernels give one image on each tree"""
    sc = scenes.demo_scene()
    w, h = 1920, 1080
    for builder in (capi.BUILD_SAH, capi.BUILD_REFERENCE_EXACT):
        out = {}
        for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
            ctx = make_ctx(sc, w, h, builder, capi.ACCUM_REF_LDR8, 4, kernel)
            try:
                ctx.render(8, 1)
                out[kernel] = images(ctx)
            finally:
                ctx.close()
        assert_same(out[capi.KERNEL_WAVEFRONT], out[capi.KERNEL_REFERENCE_LAYOUT], "builder %d" % builder)
