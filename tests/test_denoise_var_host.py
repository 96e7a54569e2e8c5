"""The variance guidance of jpt_denoise without a GPU: the host form of the guided filter (jpt_debug_atrous_variance, device -1) against
the float32 numpy restatement bit for bit, the exact propagation of a unit variance, what the guidance gains on a wall whose only edge
is one of light and on few-frame renders of the oracle, the C ABI's refusals on a host-only context, and the header and bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_denoise as nd
import np_denoise_var as nv

F = np.float32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jpt_set_denoise_variance", "jpt_read_denoised_variance_f32", "jpt_debug_atrous_variance")


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def guided(**fields):
    return capi.DenoiseVarianceParams(enable=1, **fields)


# ---- 1. the host form equals the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes", range(1, 7))
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (33, 9), (70, 21)], ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_numpy_restatement_bit_for_bit(size, passes):
    """np_denoise's synthetic guides and colours (a depth step, a crease, a miss region, NaN / +-inf / 1e30 colours) with a plane of
    second moments that has zero, negative, NaN, inf and huge entries: 1 x 1 and 5 x 3 are all border, 33 x 9 crosses both tile edges
    (32 x 8), 70 x 21 has three tile columns and rows; passes 1..6 cover first = last, the two tiled steps and the gathered ones"""
    w, h = size
    for frames, vprm in ((4, {}), (2, dict(sigma_variance=0.5, variance_floor=1e-3))):
        case = nv.synthetic_case(w, h, seed=w * 10 + passes, frame_count=frames)
        got, got_v = host.debug_atrous_variance(HOST_ONLY, case[0], case[1], frames, *case[2:], params=capi.DenoiseParams(passes=passes), vparams=guided(**vprm))
        want, want_v = nv.denoise(case[0], case[1], frames, *case[2:], passes=passes, **vprm)
        bad, bad_v = ~nd.same_bits(got, want), ~nd.same_bits(got_v, want_v)
        assert not bad.any(), "%d colour values differ, first %s" % (int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert not bad_v.any(), "%d variances differ, first %s" % (int(bad_v.sum()), np.argwhere(bad_v)[:4].tolist())
        assert (got[..., 3] == 1).all()
    # the defaults are the library's, and sigma_color is not read
    case = nv.synthetic_case(w, h, seed=5)
    a = host.debug_atrous_variance(HOST_ONLY, case[0], case[1], 4, *case[2:])
    b = host.debug_atrous_variance(HOST_ONLY, case[0], case[1], 4, *case[2:], params=capi.DenoiseParams(sigma_color=0.125))
    want = nv.denoise(case[0], case[1], 4, *case[2:], **nv.DEFAULTS)
    for got in (a, b):
        assert nd.same_bits(got[0], want[0]).all() and nd.same_bits(got[1], want[1]).all()


# ---- 2. exact variance propagation ---------------------------------------------------------------------------------------------------

def flat_wall(w, h):
    """(position_t, normal, albedo) of a wall facing the camera, albedo 1"""
    ys, xs = np.mgrid[0:h, 0:w]
    pos = np.zeros((h, w, 4), F)
    pos[..., 0], pos[..., 1], pos[..., 2] = (xs - w / 2) * 0.02, (ys - h / 2) * 0.02, -4.0
    pos[..., 3] = np.sqrt((pos[..., :3].astype(np.float64) ** 2).sum(-1))
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = 1.0
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = 1.0
    return pos, nrm, alb


@pytest.mark.parametrize("form", ["restatement", "host"])
def test_a_unit_variance_on_a_constant_image_propagates_exactly(form):
    """a constant image with v = 1 everywhere on one flat surface: every weight is the binomial one, so the colour stays what it is,
    exactly, and after one pass an interior pixel holds sum h^2 / (sum h)^2 = ((1 + 16 + 36 + 16 + 1) / 256)^2 = 4900 / 65536, exactly
    (every product and partial sum is a small integer over a power of two)"""
    w, h = 40, 12
    pos, nrm, alb = flat_wall(w, h)
    accum = np.ones((h, w, 4), F)
    accum[..., :3] = 1.0                    # two frames: the mean is 0.5
    m2 = np.zeros((h, w, 4), F)
    m2[..., 0] = 2.0                        # v_0 = 2 / (2 * 1) / 1 + 0 + 0 = 1
    for passes in (1, 3, 6):
        if form == "host":
            out, v = host.debug_atrous_variance(HOST_ONLY, accum, m2, 2, pos, nrm, alb, params=capi.DenoiseParams(passes=passes), vparams=guided())
        else:
            out, v = nv.denoise(accum, m2, 2, pos, nrm, alb, passes=passes)
        assert np.array_equal(out[..., :3], np.full((h, w, 3), 0.5, F)), passes
        if passes == 1:
            assert (v[2:-2, 2:-2] == F(4900.0 / 65536.0)).all()
            assert (v[0, :] > v[5, 5]).all()          # fewer taps at the border: less averaging
    i0, v0 = nv.first(accum, m2, 2, alb)
    assert (v0 == 1).all() and (i0 == 0.5).all()


# ---- 3. a wall whose only edge is one of light -----------------------------------------------------------------------------------------

# (frames, sigma) -> RMSE against the noiseless image of (the raw mean, jpt_denoise with the defaults, the guided filter with the
# defaults), measured with the pinned restatement, seed 0, 70 x 21
WALL_MEASURED = {(4, 0.2): (0.09891, 0.04012, 0.00611), (16, 0.2): (0.05029, 0.04081, 0.00292), (4, 0.05): (0.02473, 0.04044, 0.00131)}


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


@pytest.mark.parametrize("row", sorted(WALL_MEASURED), ids=lambda r: "%dframes-sigma%g" % r)
def test_a_shadow_edge_on_a_flat_wall_is_kept_and_the_noise_beside_it_is_not(row):
    """A flat wall with one albedo, a luminance step 1.0 -> 0.5 at the middle column and Gaussian noise of standard deviation sigma per
    frame and channel; sum and M2 by the library's own update.  No guide has an edge there: the fixed tolerance blurs the step (an
    RMSE of 0.040 whatever the noise -- in the third row worse than not filtering), the guided filter does not.  Asserted: the guided
    RMSE is below both others, and at most the midpoint between its measured value and the smaller of the other two measured."""
    frames, sigma = row
    w, h = 70, 21
    pos, nrm, alb = flat_wall(w, h)
    alb[..., :3] = 0.5
    xs = np.mgrid[0:h, 0:w][1]
    clean = np.where((xs < w // 2)[..., None], F(1.0), F(0.5)) * np.ones((h, w, 3), F)
    rad = (clean[None] + sigma * np.random.default_rng(0).standard_normal((frames, h, w, 3))).astype(F)
    s, m2 = host.debug_variance_moments(rad, capi.ACCUM_HDR_F32)
    raw = rmse(s[..., :3] / F(frames), clean)
    today = rmse(nd.denoise(s, frames, pos, nrm, alb)[..., :3], clean)
    got = rmse(nv.denoise(s, m2, frames, pos, nrm, alb)[0][..., :3], clean)
    m_raw, m_today, m_guided = WALL_MEASURED[row]
    print("%d frames, sigma %g: RMSE raw %.5f, jpt_denoise %.5f, guided %.5f (measured %.5f %.5f %.5f)" % (frames, sigma, raw, today, got, m_raw, m_today, m_guided))
    assert got < today and got < raw
    assert got <= (m_guided + min(m_raw, m_today)) / 2


# ---- 4. the oracle's scenes ------------------------------------------------------------------------------------------------------------

# (scene, frames) -> RMSE(denoised) / RMSE(raw mean) against 1024 other oracle frames of (jpt_denoise with the defaults, the guided filter
# with the defaults), measured with the pinned restatement at 96 x 64, 4 bounces.  sigma_variance 1 gives 0.5425, 0.5348, 0.5436, 0.5733
# and sigma_variance 4 gives 0.5318, 0.6840, 0.5408, 0.6917 in the order below: 2 is the default.
ORACLE_MEASURED = {("cornell", 4): (0.5358, 0.5016), ("cornell", 16): (0.5680, 0.5380), ("demo800", 4): (0.5880, 0.5169), ("demo800", 16): (0.5911, 0.5718)}
W, H, BOUNCES, TRUTH_FRAMES = 96, 64, 4, 1024


@pytest.fixture(scope="module")
def oracle_cases(oracle):
    """per scene, computed once: (truth float64 [H, W, 3], the radiance of frames 1..16 float32 [16, H, W, 3], the guides)"""
    out = {}
    for name in ("cornell", "demo800"):
        sc = scenes.cornell_scene() if name == "cornell" else scenes.demo_scene(800)
        cam = scenes.camera_block(sc.camera, W, H)
        ref = oracle.build_scene(sc)
        truth = oracle.render(ref, cam, W, H, max_bounces=BOUNCES, n_frames=TRUTH_FRAMES, first_frame_index=1000, accum_mode=wire.ACCUM_HDR_F32)[0]
        rad = np.stack([oracle.trace_frame(ref, scenes.camera_block(sc.camera, W, H, frame_index=k), W, H, BOUNCES)[0][..., :3] for k in range(1, 17)])
        out[name] = (truth[..., :3].astype(np.float64) / TRUTH_FRAMES, rad, nd.guides(ref, cam, W, H))
    return out


@pytest.mark.parametrize("case", sorted(ORACLE_MEASURED), ids=lambda c: "%s-%d" % c)
def test_few_frames_guided_are_closer_to_a_long_render_than_jpt_denoise_leaves_them(oracle_cases, case):
    """test_denoise_host's set-up (Cornell and demo_scene(800), 96 x 64, ACCUM_HDR_F32, 4 bounces, truth = frames 1000..2023) with 4
    and 16 frames; the sum and M2 of the frames by the library's own update (jpt_debug_variance_moments).  Asserted: the guided ratio
    is strictly below jpt_denoise's, computed here, and at most the midpoint of the two measured ratios."""
    name, frames = case
    truth, rad, guides = oracle_cases[name]
    s, m2 = host.debug_variance_moments(rad[:frames], capi.ACCUM_HDR_F32)
    raw = rmse(s[..., :3] / F(frames), truth)
    today = rmse(nd.denoise(s, frames, *guides)[..., :3], truth) / raw
    got = rmse(nv.denoise(s, m2, frames, *guides)[0][..., :3], truth) / raw
    m_today, m_guided = ORACLE_MEASURED[case]
    print("%s, %d frames: RMSE raw %.4f, ratio jpt_denoise %.4f, guided %.4f (measured %.4f %.4f)" % (name, frames, raw, today, got, m_today, m_guided))
    assert got < today
    assert got <= (m_today + m_guided) / 2


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

BAD = [dict(enable=2), dict(enable=-1), dict(sigma_variance=0.0), dict(sigma_variance=-2.0), dict(sigma_variance=float("nan")), dict(sigma_variance=float("inf")),
       dict(variance_floor=0.0), dict(variance_floor=-1e-6), dict(variance_floor=float("nan")), dict(variance_floor=float("inf")), dict(reserved=1)]


def test_refusals_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_denoise_variance
        for fields in BAD:
            assert S(ctx.h, C.byref(capi.DenoiseVarianceParams(**fields))) == E_INVALID, fields
            assert b"jpt_denoise_variance_params" in L.jpt_last_error(ctx.h)
        assert S(ctx.h, None) == E_DEVICE and S(ctx.h, C.byref(guided())) == E_DEVICE   # checks passed: no device
        assert b"host-only" in L.jpt_last_error(ctx.h)
        assert S(None, None) == E_INVALID
        out = np.zeros(4, F)
        assert L.jpt_read_denoised_variance_f32(None, out.ctypes.data) == E_INVALID
        assert L.jpt_read_denoised_variance_f32(ctx.h, None) == E_INVALID and b"null output" in L.jpt_last_error(ctx.h)
        assert L.jpt_read_denoised_variance_f32(ctx.h, out.ctypes.data) == E_DEVICE
        with pytest.raises(capi.JptError, match="host-only"):
            ctx.set_denoise_variance(enable=1)
        with pytest.raises(capi.JptError, match="host-only"):
            ctx.read_denoised_variance()
        assert L.jpt_denoise(ctx.h) == E_DEVICE     # (as before: the guidance was never set)
    finally:
        ctx.close()


def test_the_debug_call_checks_its_arguments(L):
    case = nv.synthetic_case(8, 8)
    out, var = np.zeros((8, 8, 4), F), np.zeros((8, 8), F)
    ptrs = [a.ctypes.data for a in case]

    def call(w=8, h=8, prm=None, vprm=None, frames=4, arrays=ptrs, o=out.ctypes.data, v=var.ctypes.data):
        return L.jpt_debug_atrous_variance(HOST_ONLY, w, h, prm, vprm, arrays[0], arrays[1], frames, *arrays[2:], o, v)

    assert call() == 0
    assert call(w=0) == E_INVALID and call(h=-1) == E_INVALID and call(w=65537) == E_INVALID
    assert call(frames=1) == E_INVALID and call(frames=0) == E_INVALID and call(frames=2) == 0
    assert call(o=None) == E_INVALID and call(v=None) == E_INVALID
    for k in range(5):
        assert call(arrays=ptrs[:k] + [None] + ptrs[k + 1:]) == E_INVALID, k
    assert call(prm=C.byref(capi.DenoiseParams(passes=9))) == E_INVALID
    for fields in BAD:
        assert call(vprm=C.byref(capi.DenoiseVarianceParams(**fields))) == E_INVALID, fields
    assert call(vprm=C.byref(capi.DenoiseVarianceParams())) == 0          # (enable is checked and otherwise ignored)
    with pytest.raises(capi.JptError, match=r"\(-1\)"):
        host.debug_atrous_variance(HOST_ONLY, case[0], case[1], 1, *case[2:])


# ---- 6. the header and the bindings ----------------------------------------------------------------------------------------------------

def test_the_header_and_the_bindings_carry_the_three_functions(L):
    header = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for pattern in (r"int jpt_set_denoise_variance\(jpt_ctx \*ctx, const jpt_denoise_variance_params \*params\);",
                    r"int jpt_read_denoised_variance_f32\(jpt_ctx \*ctx, float \*out\);",
                    r"int jpt_debug_atrous_variance\(int device_id, int32_t width, int32_t height, const jpt_denoise_params \*params,\s+"
                    r"const jpt_denoise_variance_params \*vparams, const float \*sum4, const float \*m2_4, uint32_t frame_count,\s+"
                    r"const float \*position_t, const float \*normal, const float \*albedo, float \*out4, float \*var_out\);",
                    r"typedef struct jpt_denoise_variance_params \{\s+int32_t enable;[^}]*float   sigma_variance;[^}]*float   variance_floor;[^}]*int32_t reserved;[^}]*\}"):
        assert re.search(pattern, header), pattern
    for name in NAMES:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert C.sizeof(capi.DenoiseVarianceParams) == 16
    d = capi.DenoiseVarianceParams()
    assert (d.enable, d.sigma_variance, d.reserved) == (0, 2.0, 0) and d.variance_floor == F(1e-6)
    assert L.jpt_abi_version() == 6 and "#define JPT_ABI_VERSION 6" in header
    assert not any("denoise" in s for s in capi.SYMBOLS if s.startswith("jpt_multi"))
