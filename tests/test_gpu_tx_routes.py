"""Transparent materials (JPT_MATERIAL_EXT_TRANSMISSION, the *_tx kernels) and the thin lens on the routes that decide hits exactly:
reach records, the paths set aside and finished by wf2_finish_tx (the tie walk's overflow included), one TLAS-update step, the upload
of the reference layout (the flag's words arrive in materials["padding"] only), and a scene whose only transmissive material no
instance names (the *_tx kernels launch and must reproduce the family they extend).  The emitter list follows the scene's triangle
order, which every layout numbers its own way: routes are compared within one layout, each wavefront render against the audit
kernel's render of the same tree.  Every render runs at the library's default set-aside capacity."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes

import np_light_sampling as nls
import np_transmission as ntx
from test_fuzz import forty_coincident_copies
from test_gpu_environment import assert_same, images
from test_gpu_light_routes import GROUPS
from test_gpu_parity import _moved, _moves_for
from test_gpu_transmission import LIGHTINGS, glass_random_scene, host_ref, np_sum, sun_map

pytestmark = pytest.mark.gpu

F = np.float32
TX = capi.MATERIAL_EXT_TRANSMISSION
W, H, BOUNCES, FRAMES = 96, 64, 3, 2
ROUTE_LIGHTINGS = ("sky", "map_mis", "map_mis_emitters")
LENSES = (None, (0.15, 4.0))
ACCUMS = (capi.ACCUM_HDR_F32, capi.ACCUM_REF_LDR8)


def all_glass(sc):
    """a copy of `sc` with every material in use transmissive, (0.9, 1.5) and (0.5, 1.33) in turn: a set-aside path meets the lobe with
    high probability"""
    used = sorted({m for i in sc.instances for m in i.material_ids})
    return scenes.with_transmissive_materials(sc, used, transmission=[(0.9, 0.5)[k % 2] for k in range(len(used))],
                                              ior=[(1.5, 1.33)[k % 2] for k in range(len(used))])


def _light(ctx, lighting, lens, flags):
    if lighting.startswith("map"):
        ctx.set_environment(sun_map())
        if "mis" in lighting:
            ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
    if "emitters" in lighting:
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_MIS)
    ctx.set_material_extensions(flags)
    if lens is not None:
        ctx.set_lens(*lens)


def _route_ctx(route, sc, ref, accum, lighting, lens, flags=TX, w=W, h=H, bounces=BOUNCES):
    """commit: BUILD_SAH; exact: BUILD_REFERENCE_EXACT; upload: upload_reference_layout of the oracle's arrays -- on the wavefront
    kernels, or with _audit on the audit kernel"""
    ctx = host.Context(0)
    try:
        if route.startswith("upload"):
            ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures)
        else:
            ctx.build_scene(sc, capi.BUILD_SAH if route.startswith("commit") else capi.BUILD_REFERENCE_EXACT)
        ctx.set_params(w, h, bounces, accum)
        ctx.set_kernel(capi.KERNEL_REFERENCE_LAYOUT if route.endswith("audit") else capi.KERNEL_WAVEFRONT)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        _light(ctx, lighting, lens, flags)
    except Exception:
        ctx.close()
        raise
    return ctx


def _differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


def _share(a, b):
    return 100.0 * _differing(a, b) / (a.shape[0] * a.shape[1])


def _render(route, sc, ref, accum, lighting, lens, flags=TX, step=None):
    ctx = _route_ctx(route, sc, ref, accum, lighting, lens, flags)
    try:
        ctx.render(FRAMES, 1)
        if step is not None:
            step(ctx, route)
            ctx.accum_reset()
            ctx.render(FRAMES, 1)
        return images(ctx)[:2], ctx.stats()
    finally:
        ctx.close()


def _all_routes(oracle, sc, lighting, lens, what, min_aside=1, step=None):
    """96 x 64, 3 bounces, 2 frames on the six routes, HDR and LDR8 accumulation: every wavefront route's accumulation and display
    equal its layout's audit render bit for bit (NaNs in the same places), and the commit route set paths aside and dropped none.
    step(ctx, route), if given, runs between a first render and the compared one (the accumulation is reset after it)."""
    ref = oracle.build_scene(sc)
    what = "%s, %s, lens %s" % (what, lighting, lens)
    for accum in ACCUMS:
        out, st = {}, {}
        for group in GROUPS:
            for route in group:
                out[route], st[route] = _render(route, sc, ref, accum, lighting, lens, step=step)
        print("%s, accum %d: set aside / dropped %s, pixels differing from the layout's audit kernel %s" % (
            what, accum, {r: (st[r]["set_aside"], st[r]["set_aside_dropped"]) for r in out},
            {r: _differing(out[r][0], out[g[-1]][0]) for g in GROUPS for r in g[:-1]}))
        if accum == capi.ACCUM_HDR_F32:
            off = _render("commit", sc, ref, accum, lighting, lens, capi.MATERIAL_EXT_NONE, step)[0]
            flag = _share(out["commit"][0], off[0])
            print("%s: the flag changed %.1f %% of the pixels" % (what, flag))
            assert flag > 0.0, flag
            if lens is not None:
                pin = _render("commit", sc, ref, accum, lighting, None, step=step)[0]
                changed = _share(out["commit"][0], pin[0])
                print("%s: the lens changed %.1f %% of the pixels" % (what, changed))
                assert changed > 0.0, changed
        for group in GROUPS:
            for route in group[:-1]:
                assert_same(out[route], out[group[-1]], "%s, accum %d, route %s" % (what, accum, route))
        assert st["commit"]["set_aside"] >= min_aside and st["commit"]["set_aside_dropped"] == 0, st["commit"]


# ---- 1. the set-aside and tie routes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lens", LENSES, ids=["pinhole", "lens"])
@pytest.mark.parametrize("lighting", ROUTE_LIGHTINGS)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_coincident_glass_soup_is_the_same_on_every_route(oracle, hiplib, seed, lighting, lens):
    _all_routes(oracle, all_glass(scenes.random_scene(seed, coincident=True)), lighting, lens, "coincident glass soup %d" % seed)


@pytest.mark.parametrize("lens", LENSES, ids=["pinhole", "lens"])
@pytest.mark.parametrize("lighting", ROUTE_LIGHTINGS)
def test_forty_coincident_glass_copies_are_the_same_on_every_route(oracle, hiplib, lighting, lens):
    """the tie walk's overflow: vertices decided by the reference's whole walk of its own trees, inside wf2_finish_tx, then given to
    the lobe.  A tie at bounce 0 does not depend on the materials: the flag-off render of the same scene alone sets aside as many
    paths as the env and light versions of this test ask for."""
    sc = all_glass(forty_coincident_copies())
    off = _render("commit", sc, None, capi.ACCUM_HDR_F32, lighting, lens, capi.MATERIAL_EXT_NONE)[1]
    print("forty coincident glass copies, %s, lens %s, flag off: set aside / dropped (%d, %d)" % (
        lighting, lens, off["set_aside"], off["set_aside_dropped"]))
    assert off["set_aside"] >= 301 and off["set_aside_dropped"] == 0, off
    _all_routes(oracle, sc, lighting, lens, "forty coincident glass copies", min_aside=301)


@pytest.mark.parametrize("lens", LENSES, ids=["pinhole", "lens"])
@pytest.mark.parametrize("lighting", ROUTE_LIGHTINGS)
@pytest.mark.parametrize("seed", [1, 4])
def test_moved_coincident_glass_soup_is_the_same_on_every_route(oracle, hiplib, seed, lighting, lens):
    """one TLAS-update step (jpt_scene_update_tlas; jpt_scene_update_reference_tlas on the upload routes) of the soup of
    test_exact_ties_stay_decided_after_instances_move"""
    sc = all_glass(scenes.random_scene(seed, coincident=True))
    moves = _moves_for(sc, 11 + seed, 4)
    r1 = oracle.build_scene(_moved(sc, moves))

    def step(ctx, route):
        if route.startswith("upload"):
            ctx.update_reference_tlas(r1.instances, r1.tlas_nodes)
        else:
            for i, t in moves.items():
                ctx.set_instance_transform(i, t)
            ctx.update_tlas()
    _all_routes(oracle, sc, lighting, lens, "moved coincident glass soup %d" % seed, step=step)


# ---- 2. the upload route carries the flag -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ROUTE_LIGHTINGS)
@pytest.mark.parametrize("which", ["glass_cornell", "glass_random"])
def test_uploaded_glass_renders_as_glass(oracle, hiplib, which, lighting):
    """jpt_scene_upload_reference_layout gets transmission and ior in materials["padding"] and nowhere else: the flag changes the
    render, the wavefront kernels equal the audit kernel on the uploaded tree, and, where no emitter order enters, both equal
    BUILD_REFERENCE_EXACT committed from the Scene"""
    sc = scenes.glass_cornell_scene() if which == "glass_cornell" else glass_random_scene()
    ref = oracle.build_scene(sc)
    for lens in LENSES:
        what = "uploaded %s, %s, lens %s" % (which, lighting, lens)
        for accum in ACCUMS:
            on, st = _render("upload", sc, ref, accum, lighting, lens)
            off = _render("upload", sc, ref, accum, lighting, lens, capi.MATERIAL_EXT_NONE)[0]
            audit = _render("upload_audit", sc, ref, accum, lighting, lens)[0]
            print("%s, accum %d: set aside / dropped (%d, %d), %d pixels differ from the audit kernel, the flag changed %.1f %% of the pixels" % (
                what, accum, st["set_aside"], st["set_aside_dropped"], _differing(on[0], audit[0]), _share(on[0], off[0])))
            assert _share(on[0], off[0]) > 0.0, "the flag changed nothing"
            assert st["set_aside_dropped"] == 0, st
            assert_same(on, audit, what + ", accum %d, the audit kernel" % accum)
            if "emitters" not in lighting:
                exact = _render("exact", sc, ref, accum, lighting, lens)[0]
                print("%s, accum %d: %d pixels differ from BUILD_REFERENCE_EXACT" % (what, accum, _differing(on[0], exact[0])))
                assert_same(on, exact, what + ", accum %d, BUILD_REFERENCE_EXACT" % accum)


# ---- 3. the *_tx kernels where no path takes the lobe -------------------------------------------------------------------------------------

def _with_unused_glass(sc):
    import copy
    out = copy.deepcopy(sc)
    out.materials = np.concatenate([sc.materials, scenes.material(transmission=1.0, ior=1.5)[None]])
    assert all(m < len(sc.materials) for i in out.instances for m in i.material_ids)
    return out


def _numpy_sum(sc, ref, lighting, accum):
    tabs = nls.tables(host_ref(sc, capi.BUILD_SAH)) if "emitters" in lighting else None
    cam = scenes.camera_block(sc.camera, W, H).copy()
    frames = []
    for f in range(FRAMES):
        cam["frame_index"] = 1 + f
        frames.append(ntx.trace_tx(ref, cam, W, H, BOUNCES, TX, rgb=sun_map() if lighting.startswith("map") else None,
                                   env_mis="mis" in lighting, light_tabs=tabs, textures=sc.textures))
    return np_sum(frames, accum == capi.ACCUM_REF_LDR8)


@pytest.mark.parametrize("lighting", LIGHTINGS)
@pytest.mark.parametrize("which", ["cornell", "random"])
def test_an_unused_glass_material_changes_nothing(oracle, hiplib, which, lighting):
    """One more material (transmission 1, ior 1.5) that no instance names: with the flag on lighting_bound finds a transmissive
    material and the *_tx kernels launch, yet no vertex's material transmits and transmission_step returns before it touches
    anything -- the images equal the flag-off render's, which the plain, _env, _mis and _lt kernels make.  A *_tx render under the
    sky or a map without MIS carves per-path densities the plain render has no use for (wf2_layout): its workspace is larger, which
    shows that the other family ran."""
    sc = _with_unused_glass(scenes.cornell_scene() if which == "cornell" else scenes.random_scene(2))
    ref = oracle.build_scene(sc)
    for kernel in (capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT):
        route = "commit_audit" if kernel == capi.KERNEL_REFERENCE_LAYOUT else "commit"
        for accum in ACCUMS:
            out, size = {}, {}
            for flags in (capi.MATERIAL_EXT_NONE, TX):
                ctx = _route_ctx(route, sc, ref, accum, lighting, None, flags)
                try:
                    ctx.render(FRAMES, 1)
                    out[flags], size[flags] = images(ctx)[:2], ctx.workspace_bytes()
                finally:
                    ctx.close()
            differing = _differing(out[TX][0], out[0][0])
            print("unused glass, %s, %s, kernel %d, accum %d: %d pixels differ between flag on and off; workspace %d and %d bytes" % (
                which, lighting, kernel, accum, differing, size[TX], size[0]))
            if differing:
                want = _numpy_sum(sc, ref, lighting, accum)
                print("... pixels differing from numpy: flag on %d, flag off %d" % (
                    _differing(out[TX][0][..., :3], want), _differing(out[0][0][..., :3], want)))
            assert_same(out[TX], out[0], "unused glass, %s, %s, kernel %d, accum %d" % (which, lighting, kernel, accum))
            if kernel == capi.KERNEL_WAVEFRONT and lighting in ("sky", "map"):
                assert size[TX] > size[0], size
