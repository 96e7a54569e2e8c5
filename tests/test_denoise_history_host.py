"""The history stage of jpt_denoise (jpt_set_denoise_history) without a GPU: the host form of the stage (jpt_debug_denoise_history,
device -1) against the float32 numpy restatement bit for bit over synthetic planes, the integration and its variance against float64,
the reprojection of a pixel onto itself, the C ABI's refusals on a host-only context, and the header and bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdpathtracing_amd import capi, host

import np_denoise as nd
import np_denoise_history as nh

F = np.float32
U = 2.0 ** -24                               # the unit roundoff of binary32
HOST_ONLY = -1
E_INVALID, E_DEVICE, E_STATE = -1, -2, -4   # include/jpt.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jpt_set_denoise_history", "jpt_denoise_history_reset", "jpt_read_denoise_history_f32", "jpt_debug_denoise_history")
SIZES = [(37, 19), (33, 9), (1, 1)]


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def both(device, accum, frames, guides, prev=None, prev_vp=None, same_view=False, npow=6, **hp):
    """the library's form on `device` and the restatement of one call; asserts the three planes equal bit for bit and returns them"""
    got = host.debug_denoise_history(device, accum, frames, *guides, prev=prev, prev_vp=prev_vp, same_view=same_view,
                                     params=capi.DenoiseParams(normal_power_log2=npow), hparams=capi.DenoiseHistoryParams(enable=1, **hp))
    want = nh.step(accum, frames, *guides, prev=prev, prev_vp=prev_vp, same_view=same_view, normal_power_log2=npow, **hp)
    for name, g, w in zip(("(m, v_0)", "(m, N)", "(n, S)"), got, want):
        bad = ~nd.same_bits(g, w)
        assert not bad.any(), "%s: %d values differ, first %s" % (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got


def stage_cases(device, w, h):
    """every case of the issue at one size, on `device` (the GPU test runs the same list): what each left, for the checks that follow"""
    cam0, cam1 = nh.camera(w, h), nh.camera(w, h, yaw_deg=0.9, origin=(0.07, 0.013, 0.02))   # a fraction of a pixel apart at these sizes
    bare0, bare1 = nh.plane_guides(cam0, w, h), nh.plane_guides(cam1, w, h)
    fore0, fore1 = nh.plane_guides(cam0, w, h, foreground=True), nh.plane_guides(cam1, w, h, foreground=True)
    out = {}
    # no history: misses, a NaN, an Inf and a 1e30 sample; the variance is the neighbourhood's everywhere
    first = both(device, nh.samples(w, h, 1, 1), 1, fore0)
    out["first"] = first
    # the identical view, six calls: the history passes min_history = 4 on the way, and max_history = 5 caps it
    prev = (first[1], first[2], fore0[0])
    for k in range(6):
        got = both(device, nh.samples(w, h, 1, 10 + k, spoil=k == 2), 1, fore0, prev=prev, same_view=True, max_history=5)
        prev = (got[1], got[2], fore0[0])
    out["standing"] = got
    # another view of the same surfaces: all four taps count, some fall outside the image; history lengths 0 at the spoilt pixels
    out["moved"] = both(device, nh.samples(w, h, 1, 20), 1, fore1, prev=prev, prev_vp=cam0["vp"])
    # the foreground object gone (disocclusion), and come (occlusion)
    out["gone"] = both(device, nh.samples(w, h, 1, 21), 1, bare1, prev=prev, prev_vp=cam0["vp"])
    bare_prev = both(device, nh.samples(w, h, 1, 22), 1, bare0)
    out["come"] = both(device, nh.samples(w, h, 1, 23), 1, fore1, prev=(bare_prev[1], bare_prev[2], bare0[0]), prev_vp=cam0["vp"])
    # a previous set whose every other texel has length 0; three frames per call; more frames than max_history; other parameters
    holes = prev[0].copy()
    holes.reshape(-1, 4)[::2, 3] = 0.0
    out["holes"] = both(device, nh.samples(w, h, 3, 24), 3, fore1, prev=(holes, prev[1], prev[2]), prev_vp=cam0["vp"])
    out["long"] = both(device, nh.samples(w, h, 7, 25), 7, fore0, prev=prev, same_view=True, max_history=4, min_history=2)
    out["params"] = both(device, nh.samples(w, h, 2, 26), 2, fore1, prev=prev, prev_vp=cam0["vp"], npow=2, sigma_plane=0.3, min_history=1, max_history=65536)
    # a window with fewer than two accepted taps: every pixel lies 3 or more off the tangent plane of each of its 24 neighbours
    lone = [a.copy() for a in bare0]
    ys, xs = np.mgrid[0:h, 0:w]
    lone[0][..., :3] = np.stack([xs * 0.1, ys * 0.1, -5.0 - 3.0 * ((xs % 5) + 5 * (ys % 5))], axis=-1)
    lone[0][..., 3] = -lone[0][..., 2]
    lone[1][...] = np.array([0.0, 0.0, 1.0, 0.0], F)
    out["lone"] = both(device, nh.samples(w, h, 1, 27, spoil=False), 1, lone, sigma_plane=0.01)
    out["guides"] = (fore0, fore1, bare1)
    return out


# ---- 1. the host form equals the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_numpy_restatement_bit_for_bit(size):
    """37 x 19 has two tile columns and three tile rows with ragged edges, 33 x 9 one pixel past each tile edge, 1 x 1 is all border.
    Beside the bits: the cases exercise what they are named for."""
    w, h = size
    out = stage_cases(HOST_ONLY, w, h)
    fore0, fore1, bare1 = out["guides"]
    hit0 = fore0[0][..., 3] >= 0
    iv, a, b = out["first"]
    assert (a[..., 3][~hit0] == 0).all() and (iv[..., 3][~hit0] == 0).all()                 # a miss leaves no history
    assert set(np.unique(a[..., 3][hit0])) <= {0.0, 1.0}
    iv, a, b = out["standing"]
    assert a[..., 3].max() == 5.0                                                             # capped at max_history
    assert np.isfinite(a[..., :3][a[..., 3] > 0]).all()                                       # no NaN or Inf sample ever entered m
    n_long = out["long"][1][..., 3][hit0]
    assert set(np.unique(n_long)) <= {0.0, 7.0} and (n_long == 0).sum() <= 5                  # n > max_history: N = n (0: the spoilt samples)
    if w > 1:
        assert (iv[..., 3] > 0).sum() > 0.8 * hit0.sum()                                      # the history's own variance
        n_moved, n_gone, n_come = (out[k][1][..., 3] for k in ("moved", "gone", "come"))
        assert ((n_moved > 5.5) & (n_moved < 6.5)).sum() > 0.6 * (fore1[0][..., 3] >= 0).sum()   # reprojected: N = N_h + 1, N_h = 5
        was_fg = (fore1[1][..., 2] == 1) & (fore1[0][..., 3] >= 0)
        assert was_fg.any() and (n_gone[was_fg & (bare1[0][..., 3] >= 0)] == 1).any()          # disoccluded: texels of the object are rejected
        assert set(np.unique(n_come[was_fg])) <= {0.0, 1.0}                                   # the new object has no history (0: a spoilt sample)
        assert (out["lone"][0][..., 3] == 0).all() and (out["lone"][1][..., 3].max() == 1)    # one accepted tap: v_0 = +0


# ---- 2. against float64 ----------------------------------------------------------------------------------------------------------------

def wall(w, h):
    """guides of one flat wall facing the camera, albedo 1"""
    ys, xs = np.mgrid[0:h, 0:w]
    pos = np.zeros((h, w, 4), F)
    pos[..., 0], pos[..., 1], pos[..., 2], pos[..., 3] = (xs - w / 2) * 0.02, (ys - h / 2) * 0.02, -4.0, 4.0
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = 1.0
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = 1.0
    return pos, nrm, alb


@pytest.mark.parametrize("frames", [1, 3])
def test_identical_view_calls_give_the_mean_and_its_variance(frames):
    """k = 12 identical-view calls of n frames over seeded samples c in [0, B), B = 2 (albedo 1, so c = sum / n in binary32, taken as the
    float64 reference's input): m against the float64 mean, v_0 against m2 / (k (k - 1)) (n = 1; for n frames per call the same West
    update in float64).  The bounds, with u = 2^-24 and every intermediate of a step below 2 B:
      m: a step computes al = n / N (u), d = c - m_h (u), al * d (u) and the sum (u) on values <= 2 B, and passes the error of m_h on
         times (1 - al) <= 1: e_k <= e_k-1 + 4 u 2 B, so |m - mean| <= 8 k u B.
      S: a sum of non-negative terms through 7 roundings per step (the three squares and two sums of |d|^2, al * ., S_h + ., (1 - al), the
         product) -- at most 9 k u S relative -- plus what the error of d, e_k-1 + u |d| <= 8 k u B, does to |d|^2 <= 3 (2 B)^2: per step
         al * 2 * sqrt(3) * 2 B * 8 k u B * sqrt(3) <= 96 al k u B^2, summed over the steps with al = 1 / j: <= 96 k u B^2 (1 + ln k).
         v_0 = S al / (1 - al) adds three roundings and multiplies by al / (1 - al) = 1 / (k - 1):
         |v_0 - ref| <= (9 k + 3) u ref + 96 k (1 + ln k) u B^2 / (k - 1)."""
    w, h, k, B = 16, 8, 12, 2.0
    guides = wall(w, h)
    prev, cs = None, []
    for j in range(k):
        acc = nh.samples(w, h, frames, 100 + j, spoil=False)
        cs.append((acc[..., :3] / F(frames)).astype(F))
        iv, a, b = host.debug_denoise_history(HOST_ONLY, acc, frames, *guides, prev=prev, same_view=True,
                                              hparams=capi.DenoiseHistoryParams(enable=1, max_history=65536, min_history=1))
        prev = (a, b, guides[0])
        assert (a[..., 3] == frames * (j + 1)).all()                  # N grows by n per call
    m64, S64, N64, v64 = nh.integrate64(np.stack(cs), n=frames)
    if frames == 1:
        c64 = np.stack(cs).astype(np.float64)
        assert np.allclose(m64, c64.mean(0), rtol=1e-13) and np.allclose(v64, ((c64 - c64.mean(0)) ** 2).sum((0, -1)) / (k * (k - 1)), rtol=1e-12)
    err_m = np.abs(iv[..., :3] - m64).max()
    err_v = np.abs(iv[..., 3] - v64)
    tol_v = (9 * k + 3) * U * v64 + 96 * k * (1 + np.log(k)) * U * B * B / (k - 1)
    print("n = %d: |m - mean| max %.3g (bound %.3g), |v_0 - ref| max %.3g (bound min %.3g)" % (frames, err_m, 8 * k * U * B, err_v.max(), tol_v.min()))
    assert err_m <= 8 * k * U * B
    assert (err_v <= tol_v).all() and (iv[..., 3] > 0).all()


def test_the_length_grows_by_n_per_call_and_stops_at_max_history(L):
    w, h = 8, 4
    guides = wall(w, h)
    prev, lengths = None, []
    for j in range(9):
        iv, a, b = host.debug_denoise_history(HOST_ONLY, nh.samples(w, h, 2, 200 + j, spoil=False), 2, *guides, prev=prev, same_view=True,
                                              hparams=capi.DenoiseHistoryParams(enable=1, max_history=7, min_history=1))
        prev = (a, b, guides[0])
        lengths.append(float(a[0, 0, 3]))
        assert (a[..., 3] == a[0, 0, 3]).all()
    assert lengths == [2.0, 4.0, 6.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0]


def test_a_pixels_own_position_reprojects_onto_its_centre():
    """X of the pixel-centre rays of a camera, through the same camera's vp without the identical-view flag: pu = x and pv = y up to
    the rounding of the 4 x 4 product.  A row of it is four products and three sums, each rounded once, of terms m_i X_i that carry the
    rounding of X and of vp to binary32: at most 9 u sum |m_i X_i| to first order; X itself comes from a ray made with the binary32
    ivp, another such product (9 u more of the same size).  The two divisions by clip.w pass on |row error| / w + |n| |w error| / w,
    the map to pixels multiplies by W / 2 (H / 2) and rounds four more times on values <= W:
    |pu - x| <= W / 2 * 18 u (A_x + |nx| A_w) / w + 4 u W, with A_r = sum |m_i X_i| of row r."""
    for w, h in ((37, 19), (96, 64)):
        cam = nh.camera(w, h, yaw_deg=12.0, origin=(0.3, -0.2, 0.5))
        X = nh.plane_guides(cam, w, h)[0]
        hit = X[..., 3] >= 0
        ok, pu, pv = nh.project(cam["vp"], X, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        m = np.abs(cam["vp"].astype(np.float64).reshape(-1))
        ax = np.abs(X.astype(np.float64))
        rows = [m[r] * ax[..., 0] + m[4 + r] * ax[..., 1] + m[8 + r] * ax[..., 2] + m[12 + r] for r in range(4)]
        mm = cam["vp"].astype(np.float64).reshape(-1)
        cw = np.abs(mm[3] * X[..., 0] + mm[7] * X[..., 1] + mm[11] * X[..., 2] + mm[15])
        tol_x = w / 2 * 18 * U * (rows[0] + rows[3]) / cw + 4 * U * w
        tol_y = h / 2 * 18 * U * (rows[1] + rows[3]) / cw + 4 * U * h
        ex, ey = np.abs(pu - xs)[hit], np.abs(pv - ys)[hit]
        print("%d x %d: |pu - x| max %.3g (bound min %.3g), |pv - y| max %.3g (bound min %.3g)" % (w, h, ex.max(), tol_x[hit].min(), ey.max(), tol_y[hit].min()))
        assert ok[hit].all()
        assert (ex <= tol_x[hit]).all() and (ey <= tol_y[hit]).all()
        # ... and the library's own projection: a first call's set, seen again through the same camera without the flag.  Every hit
        # lands within 1e-4 of its own texel, which weighs nearly 1 and passes the geometric test against itself; what else its four taps
        # reach has N = 1 or 0, and sum (wt * 1) and sum wt are the same additions in the same order: N_h = 1 exactly, N = 1 + n = 2
        guides = nh.plane_guides(cam, w, h)
        first = host.debug_denoise_history(HOST_ONLY, nh.samples(w, h, 1, 5, spoil=False), 1, *guides)
        iv, a, b = host.debug_denoise_history(HOST_ONLY, nh.samples(w, h, 1, 6, spoil=False), 1, *guides, prev=(first[1], first[2], guides[0]),
                                              prev_vp=cam["vp"], same_view=False)
        assert (first[1][..., 3][hit] == 1).all() and (a[..., 3][hit] == 2).all() and (a[..., 3][~hit] == 0).all()
        # the integrated colour is the mean of the pixel's own two samples up to what a neighbour's weight of at most the bound lets in
        c0, c1 = first[0][..., :3].astype(np.float64), nh.step(nh.samples(w, h, 1, 6, spoil=False), 1, *guides)[0][..., :3].astype(np.float64)
        leak = 2.0 * np.maximum(tol_x, tol_y)[hit][:, None] * 64.0 + 8 * U * 128.0      # (|c| <= 2 / amod <= 128)
        assert (np.abs(iv[..., :3][hit] - (c0 + c1)[hit] / 2) <= leak).all()


def test_a_sum_of_squares_that_overflowed_is_not_passed_on():
    """one finite sample whose |d|^2 is past FLT_MAX makes S = inf, which (1 - al) never shrinks: the texel is stored as it is and is no
    usable tap afterwards -- the pixel itself and the pixels that would tap it start over, and nothing else inherits the inf"""
    w, h = 16, 8
    guides = wall(w, h)
    first = host.debug_denoise_history(HOST_ONLY, nh.samples(w, h, 1, 300, spoil=False), 1, *guides)
    big = nh.samples(w, h, 1, 301, spoil=False)
    big[4, 8, :3] = 1e30
    second = host.debug_denoise_history(HOST_ONLY, big, 1, *guides, prev=(first[1], first[2], guides[0]), same_view=True)
    assert np.isinf(second[2][4, 8, 3]) and second[1][4, 8, 3] == 2 and np.isfinite(np.delete(second[2][..., 3].reshape(-1), 4 * w + 8)).all()
    prev = (second[1], second[2], guides[0])
    for same in (True, False):
        args = dict(prev=prev, same_view=same, prev_vp=None if same else np.eye(4, dtype=F))
        iv, a, b = both(HOST_ONLY, nh.samples(w, h, 1, 302, spoil=False), 1, guides, **args)
        assert np.isfinite(b[..., 3]).all() and np.isfinite(iv).all()
        if same:
            assert a[4, 8, 3] == 1 and (np.delete(a[..., 3].reshape(-1), 4 * w + 8) == 3).all()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------

BAD = [dict(enable=2), dict(enable=-1), dict(max_history=0), dict(max_history=65537), dict(min_history=0), dict(min_history=33), dict(max_history=3),
       dict(sigma_plane=0.0), dict(sigma_plane=-1.0), dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")), dict(reserved=(0, 0, 1, 0)),
       dict(reserved=(1, 0, 0, 0))]


def test_refusals_on_a_host_only_context(L):
    ctx = host.Context(HOST_ONLY)
    try:
        S = L.jpt_set_denoise_history
        for fields in BAD:
            assert S(ctx.h, C.byref(capi.DenoiseHistoryParams(**fields))) == E_INVALID, fields
            assert b"jpt_denoise_history_params" in L.jpt_last_error(ctx.h)
        assert S(ctx.h, None) == E_DEVICE and S(ctx.h, C.byref(capi.DenoiseHistoryParams(enable=1))) == E_DEVICE   # checks passed: no device
        assert b"host-only" in L.jpt_last_error(ctx.h)
        assert S(None, None) == E_INVALID
        assert L.jpt_denoise_history_reset(None) == E_INVALID and L.jpt_denoise_history_reset(ctx.h) == E_DEVICE
        out = np.zeros(4, F)
        assert L.jpt_read_denoise_history_f32(None, out.ctypes.data, None) == E_INVALID
        assert L.jpt_read_denoise_history_f32(ctx.h, out.ctypes.data, None) == E_DEVICE
        for call in (lambda: ctx.set_denoise_history(enable=1), ctx.denoise_history_reset, ctx.read_denoise_history):
            with pytest.raises(capi.JptError, match="host-only"):
                call()
        assert L.jpt_denoise(ctx.h) == E_DEVICE     # (as before: the history was never set)
    finally:
        ctx.close()


def test_the_debug_call_checks_its_arguments(L):
    w = h = 8
    guides = wall(w, h)
    acc = nh.samples(w, h, 1, 0)
    first = host.debug_denoise_history(HOST_ONLY, acc, 1, *guides)
    outs = [np.zeros((h, w, 4), F) for _ in range(3)]
    ins = [acc.ctypes.data] + [g.ctypes.data for g in guides]
    prev = [first[1].ctypes.data, first[2].ctypes.data, guides[0].ctypes.data]
    vp = np.eye(4, dtype=F).reshape(-1)

    def call(w_=w, h_=h, prm=None, hp=None, frames=1, arrays=ins, view=vp.ctypes.data, same=0, old=prev, o=None):
        o = [x.ctypes.data for x in outs] if o is None else o
        return L.jpt_debug_denoise_history(HOST_ONLY, w_, h_, prm, hp, arrays[0], frames, *arrays[1:], view, same, *old, *o)

    assert call() == 0 and call(old=[None] * 3, view=None) == 0 and call(same=1, view=None) == 0
    assert call(w_=0) == E_INVALID and call(h_=-1) == E_INVALID and call(w_=65537) == E_INVALID
    assert call(frames=0) == E_INVALID and call(same=2) == E_INVALID
    assert call(view=None) == E_INVALID                                      # a previous set in another view needs the view
    for k in range(3):
        assert call(old=prev[:k] + [None] + prev[k + 1:]) == E_INVALID, k    # a set is three planes
        assert call(o=[x.ctypes.data for x in outs[:k]] + [None] + [x.ctypes.data for x in outs[k + 1:]]) == E_INVALID, k
    for k in range(4):
        assert call(arrays=ins[:k] + [None] + ins[k + 1:]) == E_INVALID, k
    assert call(prm=C.byref(capi.DenoiseParams(normal_power_log2=9))) == E_INVALID
    for fields in BAD:
        assert call(hp=C.byref(capi.DenoiseHistoryParams(**fields))) == E_INVALID, fields
    assert call(hp=C.byref(capi.DenoiseHistoryParams())) == 0                # (enable is checked and otherwise ignored)
    with pytest.raises(capi.JptError, match=r"\(-1\)"):
        host.debug_denoise_history(HOST_ONLY, acc, 0, *guides)


# ---- 4. the header and the bindings ------------------------------------------------------------------------------------------------------

def test_the_header_and_the_bindings_carry_the_four_functions(L):
    header = open(os.path.join(ROOT, "include", "jpt.h")).read()
    for pattern in (r"int jpt_set_denoise_history\(jpt_ctx \*ctx, const jpt_denoise_history_params \*params\);",
                    r"int jpt_denoise_history_reset\(jpt_ctx \*ctx\);",
                    r"int jpt_read_denoise_history_f32\(jpt_ctx \*ctx, float \*integrated4, float \*length\);",
                    r"int jpt_debug_denoise_history\(int device_id, int32_t width, int32_t height, const jpt_denoise_params \*params,\s+"
                    r"const jpt_denoise_history_params \*hparams, const float \*sum4, uint32_t frame_count, const float \*position_t,",
                    r"typedef struct jpt_denoise_history_params \{\s+int32_t enable;[^}]*int32_t max_history;[^}]*int32_t min_history;[^}]*float   sigma_plane;"
                    r"[^}]*int32_t reserved\[4\];[^}]*\}"):
        assert re.search(pattern, header), pattern
    for name in NAMES:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert C.sizeof(capi.DenoiseHistoryParams) == 32 and C.sizeof(capi.DenoiseParams) == 16 and C.sizeof(capi.DenoiseVarianceParams) == 16
    d = capi.DenoiseHistoryParams()
    assert (d.enable, d.max_history, d.min_history, tuple(d.reserved)) == (0, 32, 4, (0, 0, 0, 0)) and d.sigma_plane == F(0.05)
    assert L.jpt_abi_version() == 6 and "#define JPT_ABI_VERSION 6" in header
    assert not any("denoise" in s for s in capi.SYMBOLS if s.startswith("jpt_multi"))
