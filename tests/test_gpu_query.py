"""jpt_query_rays / jpt_query_rays_device / jpt_query_pixels on the device against the numpy restatement (np_query: brute force over
every triangle, no tree): every ray of every case is checked, bit for bit; the queries follow the device's scene through refits and
mesh updates, and move nothing a render or a read-back reads."""
import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_denoise as nd
import np_query as nq

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 24, 16
N_RANDOM = 2000          # + W * H pixel-centre rays = 2 384 rays: 37 waves and a quarter
SCENES = {"cornell": scenes.cornell_scene, "demo800": lambda: scenes.demo_scene(800)}
E_INVALID = -1

_cache = {}


def case(oracle, name):
    """(scene, the oracle's arrays, camera block, origins, dirs, brute-force minimum): made once per scene and left unchanged"""
    if name not in _cache:
        sc = SCENES[name]()
        ref = oracle.build_scene(sc)
        cam = scenes.camera_block(sc.camera, W, H)
        ro, rd = nq.random_rays(N_RANDOM, seed=20260 + len(name))
        co, cd = nd.centre_rays(cam, W, H)
        o, d = np.concatenate([ro, co]).astype(F), np.concatenate([rd, cd]).astype(F)
        assert len(o) % 64 != 0
        best = nq.brute_force_t(ref, o, d)        # (asserts that no accepted test has a NaN t)
        for a in (o, d, best):
            a.setflags(write=False)
        _cache[name] = (sc, ref, cam, o, d, best)
    return _cache[name]


def make_ctx(sc, ref, route, w=W, h=H):
    ctx = host.Context(0)
    if route in ("native_upload", "as_given"):
        ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures,
                                    as_given=route == "as_given")
    else:
        ctx.build_scene(sc, dict(sah=capi.BUILD_SAH, watertight=capi.BUILD_SAH_WATERTIGHT, reference_exact=capi.BUILD_REFERENCE_EXACT)[route])
    ctx.set_params(w, h, 3, capi.ACCUM_HDR_F32)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    return ctx


def same_records(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. closest equals brute force ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["sah", "watertight", "native_upload"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_hits_on_native_trees_equal_brute_force_for_every_ray(oracle, hiplib, name, route):
    """t is the brute-force minimum bit for bit; the (instance, triangle) named, re-intersected in numpy from the buffers
    jpt_scene_get_reference_buffer hands out, gives the t, u, v returned, and np_path's shading record of it the position, normal,
    uv, material and front flag; misses carry the miss encoding; the byte says which is which.  2 384 of 2 384 rays checked."""
    sc, ref, cam, o, d, best = case(oracle, name)
    ctx = make_ctx(sc, ref, route)
    try:
        assert ctx.tree_kind() in (capi.TREE_NATIVE_REACH, capi.TREE_NATIVE_WATERTIGHT)
        view = nq.scene_view(ctx)
        hits, occ = ctx.query_rays(o, d)
    finally:
        ctx.close()
    bad, _ = nq.closest_mismatches(view, o, d, None, hits, best=best)
    n_hit = int((best < nq.MISS_T).sum())
    print("%s %s: %d rays, %d hits, %d mismatches" % (name, route, len(o), n_hit, int(bad.sum())))
    assert not bad.any(), "rays whose hit is not the pin's: %s" % np.nonzero(bad)[0][:8].tolist()
    assert np.array_equal(hits["t"][best < nq.MISS_T].view(np.uint32), best[best < nq.MISS_T].view(np.uint32))
    assert np.array_equal(occ, (best < nq.MISS_T).astype(np.uint8))
    assert n_hit > 1000 and len(o) - n_hit > 30
    assert (hits["flags"][best < nq.MISS_T] & capi.HIT_FRONT).any() and not (hits["flags"][best < nq.MISS_T] & capi.HIT_FRONT).all()


# ---- 2. the reference's own trees -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["reference_exact", "as_given"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_hits_on_reference_trees_differ_from_brute_force_only_through_cracks(oracle, hiplib, name, route):
    """the two-child records give that tree's answer; the reference's boxes have float cracks: as for the guides, at most 0.1 % of
    the rays (2 of 2 384) may differ from brute force, each one with a farther hit or a miss -- a crack loses a triangle, it never
    invents one.  The count found is printed."""
    sc, ref, cam, o, d, best = case(oracle, name)
    ctx = make_ctx(sc, ref, route)
    try:
        assert ctx.tree_kind() in (capi.TREE_REFERENCE_EXACT, capi.TREE_AS_GIVEN)
        view = nq.scene_view(ctx)
        hits, occ = ctx.query_rays(o, d)
    finally:
        ctx.close()
    bad, _ = nq.closest_mismatches(view, o, d, None, hits, best=best)
    idx = np.nonzero(bad)[0]
    print("%s %s: %d of %d rays differ from brute force" % (name, route, len(idx), len(o)))
    assert len(idx) <= 2
    for k in idx:
        assert hits["t"][k] == -1 or hits["t"][k] > best[k], "ray %d: t %r, brute force %r" % (k, hits["t"][k], best[k])
    assert np.array_equal(occ, (hits["flags"] & capi.HIT_VALID).astype(np.uint8))


# ---- 3. tmax ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_tmax_bounds_the_walk_from_above_exclusively(oracle, hiplib, name):
    sc, ref, cam, o, d, best = case(oracle, name)
    hit = best < nq.MISS_T
    ho, hd, ht = o[hit], d[hit], best[hit]
    above = np.nextafter(ht, F(np.inf))
    ctx = make_ctx(sc, ref, "sah")
    try:
        view = nq.scene_view(ctx)
        at_t, occ_at = ctx.query_rays(ho, hd, ht)
        over, occ_over = ctx.query_rays(ho, hd, above)
        sentinel = [ctx.query_rays(o, d, v)[0] for v in (0.0, -1.0, np.nan, np.inf, 1e9, 2e9)]
        any_cases = [0.0, 3.0, np.where(hit, best, F(2.5)), np.where(hit, np.nextafter(best, F(np.inf)), F(2.5))]
        any_got = [ctx.query_rays(o, d, v, mode=capi.QUERY_ANY) for v in any_cases]
    finally:
        ctx.close()
    # tmax = the hit's own t: never the same t again -- the minimum is not under it, so a miss (a strictly nearer tie partner cannot
    # exist below the minimum)
    assert not (at_t["t"] == ht).any()
    assert not nq.closest_mismatches(view, ho, hd, ht, at_t, best=ht)[0].any() and not occ_at.any()
    # one float above: the hit again, same bits
    assert np.array_equal(over["t"].view(np.uint32), ht.view(np.uint32)) and occ_over.all()
    assert not nq.closest_mismatches(view, ho, hd, above, over, best=ht)[0].any()
    # NaN, <= 0, >= 1e9 and infinity are all the unbounded query
    for other in sentinel[1:]:
        assert same_records(other, sentinel[0])
    assert not nq.closest_mismatches(view, o, d, None, sentinel[0], best=best)[0].any()
    # any-hit: occluded == (the brute-force minimum is under tmax)
    for v, got in zip(any_cases, any_got):
        want = best < nq.effective_tmax(v, len(o))
        assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), "tmax %r: %d rays differ" % (v, int((got != want).sum()))
    assert 0 < int((best < F(3.0)).sum()) < int(hit.sum())


# ---- 4. bad rays ------------------------------------------------------------------------------------------------------------------

def test_bad_rays_are_flagged_and_their_neighbours_unaffected(oracle, hiplib):
    sc, ref, cam, o, d, best = case(oracle, "cornell")
    o2, d2 = o[:200].copy(), d[:200].copy()
    o2[7, 0] = np.nan
    d2[64, 2] = np.inf
    d2[65] = 0.0
    d2[130, 1] = -np.inf
    o2[199] = np.inf
    where = [7, 64, 65, 130, 199]
    ctx = make_ctx(sc, ref, "sah")
    try:
        view = nq.scene_view(ctx)
        hits, occ = ctx.query_rays(o2, d2)
        any_occ = ctx.query_rays(o2, d2, mode=capi.QUERY_ANY)
        good, _ = ctx.query_rays(o[:200], d[:200])
    finally:
        ctx.close()
    assert same_records(hits[where], nq.miss_record(len(where), capi.HIT_BAD_RAY))
    assert not occ[where].any() and not any_occ[where].any()
    keep = np.setdiff1d(np.arange(200), where)
    assert same_records(hits[keep], good[keep]) and np.array_equal(any_occ[keep], occ[keep])
    assert not nq.closest_mismatches(view, o2, d2, None, hits)[0].any()


# ---- 5. pixels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_pixel_queries_equal_the_guide_images_and_ignore_the_lens(oracle, hiplib, name):
    sc, ref, cam, o, d, best = case(oracle, name)
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=1).astype(F)
    off = np.array([[-3.5, 7.25], [30.0, 20.0], [11.75, -2.0], [0.0, 0.0], [W, H], [np.nan, 3.0], [4.0, np.inf]], F)
    ctx = make_ctx(sc, ref, "sah")
    try:
        view = nq.scene_view(ctx)
        ctx.render(1, 1)
        ctx.denoise()
        position_t, normal, _ = ctx.read_guides()
        hits = ctx.query_pixels(centres)
        ctx.set_lens(0.2, 5.0)
        with_lens = ctx.query_pixels(centres)
        # a camera inside the box, where the rays around the screen hit its walls too
        near = scenes.camera_block(scenes.CameraDesc(scenes.transform12(None, (0, 0, 2.0))), W, H)
        ctx.set_camera(near)
        off_hits = ctx.query_pixels(off)
        oo, od = nq.raster_rays(near, W, H, off[:5, 0], off[:5, 1])
        off_rays, _ = ctx.query_rays(oo, od)
    finally:
        ctx.close()
    pt, nr = position_t.reshape(-1, 4), normal.reshape(-1, 4)
    valid = (hits["flags"] & capi.HIT_VALID) != 0
    assert np.array_equal(valid, pt[:, 3] >= 0) and valid.any()
    assert np.array_equal(hits["position"][valid].view(np.uint32), pt[valid, :3].view(np.uint32))
    assert np.array_equal(hits["normal"][valid].view(np.uint32), nr[valid, :3].view(np.uint32))
    assert same_records(hits[~valid], nq.miss_record(int((~valid).sum())))
    assert not nq.closest_mismatches(view, o[N_RANDOM:], d[N_RANDOM:], None, hits, best=best[N_RANDOM:])[0].any()
    # off-screen coordinates: a ray is a ray
    assert same_records(off_hits[:5], off_rays) and not nq.closest_mismatches(view, oo, od, None, off_hits[:5])[0].any()
    assert (off_hits["flags"][:5] & capi.HIT_VALID).all()
    assert same_records(off_hits[5:], nq.miss_record(2, capi.HIT_BAD_RAY))
    assert same_records(with_lens, hits)


def test_pixel_queries_need_params_and_a_camera(hiplib):
    ctx = host.Context(0)
    try:
        with pytest.raises(capi.JptError, match=r"\(-4\).*no scene"):
            ctx.query_pixels([[0.5, 0.5]])
        with pytest.raises(capi.JptError, match=r"\(-4\).*no scene"):
            ctx.query_rays([[0, 0, 0]], [[0, 0, -1]])
        ctx.build_scene(scenes.cornell_scene(), capi.BUILD_SAH)
        with pytest.raises(capi.JptError, match=r"\(-4\).*jpt_set_params"):
            ctx.query_pixels([[0.5, 0.5]])
        hits, occ = ctx.query_rays([[0, 0, 0]], [[0, 0, -1]])         # rays need neither
        assert hits["flags"][0] & capi.HIT_VALID and occ[0] == 1
    finally:
        ctx.close()


# ---- 6. the queries follow the device's scene ---------------------------------------------------------------------------------------

def test_queries_follow_a_device_refit_of_the_instances(oracle, hiplib):
    sc, ref, cam, o, d, best = case(oracle, "cornell")
    moved = scenes.cornell_scene()
    moved.instances[2].transform = scenes.transform12(scenes.rot_y(31.0), (0.4, -3.0 + 0.85, 1.2))
    ctx = make_ctx(sc, ref, "sah")
    try:
        before, _ = ctx.query_rays(o, d)
        ctx.refit_tlas(np.stack([i.transform for i in moved.instances]))
        after, _ = ctx.query_rays(o, d)
    finally:
        ctx.close()
    assert not nq.closest_mismatches(ref, o, d, None, before, indexed=False, best=best)[0].any()
    assert not nq.closest_mismatches(oracle.build_scene(moved), o, d, None, after, indexed=False)[0].any()
    assert not same_records(before, after)


def test_queued_device_queries_around_a_mesh_update_each_see_their_own_scene(oracle, hiplib):
    """query, jpt_scene_update_mesh, query -- the asynchronous form, nothing synchronised in between: the update waits on the device
    for the query queued before it, the query queued after it waits for the update"""
    import torch
    sc, ref, cam, o, d, best = case(oracle, "cornell")
    grown = scenes.cornell_scene()
    grown.meshes[2] = scenes.box_mesh(2.2, 2.6, 1.2)
    ctx = make_ctx(sc, ref, "watertight")
    try:
        ctx.update_mesh(2, sc.meshes[2])          # (the first update after a commit sets the refit up and drains; this one moves nothing)
        ctx.sync()
        rays = torch.from_numpy(host.make_rays(o, d).view(np.uint8)).cuda()
        h1, h2 = (torch.zeros(len(o) * 64, dtype=torch.uint8, device="cuda") for _ in range(2))
        o1, o2 = (torch.zeros(len(o), dtype=torch.uint8, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        assert ctx.query_rays_device(rays, hits=h1, occluded=o1) is None
        ctx.update_mesh(2, grown.meshes[2])
        assert ctx.query_rays_device(rays, hits=h2, occluded=o2) is None
        ctx.sync()
        before, after = (h.cpu().numpy().view(wire.RAY_HIT) for h in (h1, h2))
        occ_after = o2.cpu().numpy()
    finally:
        ctx.close()
    assert not nq.closest_mismatches(ref, o, d, None, before, indexed=False, best=best)[0].any()
    bad, best_grown = nq.closest_mismatches(oracle.build_scene(grown), o, d, None, after, indexed=False)
    assert not bad.any()
    assert np.array_equal(occ_after, (best_grown < nq.MISS_T).astype(np.uint8))
    assert not same_records(before, after)


# ---- 7. chunking ------------------------------------------------------------------------------------------------------------------

def test_more_rays_than_one_chunk(oracle, hiplib):
    """2^20 + 77 rays (one full trip through the staging buffers and a ragged one) on four triangles: the t bits and the instance
    of every ray"""
    n = (1 << 20) + 77
    sc = scenes.Scene("two_planes", [scenes.plane_mesh(4.0)],
                      [scenes.Instance(0, scenes.transform12(None, (0, -1, 0)), [2]), scenes.Instance(0, scenes.transform12(scenes.rot_y(30.0), (0.5, 1, 0)), [3])],
                      scenes.cornell_scene().materials, scenes.cornell_scene().camera)
    ref = oracle.build_scene(sc)
    o, d = nq.random_rays(n, seed=7, extent=2.5)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT)
        hits, occ = ctx.query_rays(o, d)
        any_occ = ctx.query_rays(o, d, mode=capi.QUERY_ANY)
    finally:
        ctx.close()
    with np.errstate(all="ignore"):
        best = np.full(n, nq.MISS_T, F)
        tests = [(i, ok, t) for i, _, ok, t, *_ in nd._tri_tests(ref, o, d)]
        for _, ok, t in tests:
            assert not (ok & np.isnan(t)).any()
            best = np.where(ok & (t < best), t, best)
        hit = best < nq.MISS_T
        inst_ok = ~hit & (hits["instance"] == -1)
        for i, ok, t in tests:
            inst_ok |= hit & ok & (t == best) & (hits["instance"] == i)
    want_t = np.where(hit, best, F(-1.0))
    assert np.array_equal(hits["t"].view(np.uint32), want_t.view(np.uint32)), "%d rays" % int((hits["t"] != want_t).sum())
    assert inst_ok.all()
    assert np.array_equal(occ, hit.astype(np.uint8)) and np.array_equal(any_occ, occ)
    assert 1000 < int(hit.sum()) < n - 1000 and hit[1 << 20:].any()


# ---- 8. nothing else moves --------------------------------------------------------------------------------------------------------

def _images(ctx):
    return ctx.read_accum(), ctx.read_ldr(), ctx.read_depth()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("accumulation", "display", "depth")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs" % (what, name)


def test_queries_change_no_buffer_no_later_render_and_no_statistic(oracle, hiplib):
    import torch
    sc, ref, cam, o, d, best = case(oracle, "demo800")
    a, b = make_ctx(sc, ref, "sah", 96, 64), make_ctx(sc, ref, "sah", 96, 64)
    try:
        a.render(2, 1, counted=True)
        before, stats = _images(a), a.stats()
        a.query_rays(o, d)
        a.query_rays(o, d, 2.0, mode=capi.QUERY_ANY)
        a.query_pixels([[10.5, 10.5], [95.5, 0.5]])
        a.query_rays_device(torch.from_numpy(host.make_rays(o, d).view(np.uint8)).cuda())
        _same(_images(a), before, "read-backs around the queries")
        assert a.stats() == stats
        a.render(2, 3, asynchronous=True)
        a.query_rays(o[:100], d[:100])
        a.render(2, 5, asynchronous=True)
        b.render(2, 1, counted=True)
        b.render(2, 3, asynchronous=True)
        b.render(2, 5, asynchronous=True)
        _same(_images(a), _images(b), "a context that never queried")
    finally:
        a.close()
        b.close()


# ---- 9. the device form -----------------------------------------------------------------------------------------------------------

def test_device_form_equals_host_form_and_refuses_misaligned_pointers(oracle, hiplib):
    import torch
    sc, ref, cam, o, d, best = case(oracle, "demo800")
    tmax = np.where(np.arange(len(o)) % 3 == 0, F(2.0), F(0.0))
    ctx = make_ctx(sc, ref, "sah")
    try:
        host_hits, host_occ = ctx.query_rays(o, d, tmax)
        host_any = ctx.query_rays(o, d, tmax, mode=capi.QUERY_ANY)
        rays = torch.from_numpy(host.make_rays(o, d, tmax).view(np.uint8)).cuda()
        dev_hits, dev_occ = ctx.query_rays_device(rays)
        dev_any = ctx.query_rays_device(rays, mode=capi.QUERY_ANY)
        # closest without the byte; raw pointers
        hits_only = torch.zeros(len(o) * 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.query_rays_device(rays.data_ptr(), hits=hits_only.data_ptr(), n=len(o))
        ctx.sync()
        L = hiplib
        p, h = rays.data_ptr(), hits_only.data_ptr()
        assert p % 16 == 0 and h % 16 == 0
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, p + 4, len(o) - 1, h, None) == E_INVALID and b"aligned" in L.jpt_last_error(ctx.h)
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, p, len(o) - 1, h + 32 + 8, None) == E_INVALID
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, p, len(o) - 1, h, h + 1) == E_INVALID
        pageable = host.make_rays(o, d, tmax)      # host memory is not device memory
        assert pageable.ctypes.data % 16 == 0
        assert L.jpt_query_rays_device(ctx.h, capi.QUERY_CLOSEST, pageable.ctypes.data, len(o), h, None) == E_INVALID and b"device memory" in L.jpt_last_error(ctx.h)
        ctx.sync()
        assert same_records(hits_only.cpu().numpy().view(wire.RAY_HIT), host_hits)      # (the refused calls wrote nothing)
    finally:
        ctx.close()
    assert same_records(dev_hits, host_hits) and np.array_equal(dev_occ, host_occ)
    assert np.array_equal(dev_any, host_any) and np.array_equal(host_any, host_occ)
    assert (host_hits["flags"] & capi.HIT_VALID).sum() < (best < nq.MISS_T).sum()        # (tmax = 2 cut some hits off)
