"""TEMPORAL_REPROJECTION on the device -- temporal_kernel (jpt_kernels_post.hip) and the state around it in jpt_render.cpp and jpt_capi.cpp (the two
history images, hist_valid, hist_written, the image picked by frame_count % 2) -- at the edges tests/test_oracle_temporal.py pins
for the oracle on the CPU.  Every comparison is bit for bit.  Two yardsticks:

(a) the oracle: trace_frame -> screen_rgba8 -> np_restatement.temporal_reproject AND oracle.temporal_reproject over a model pair
    fb1 / fb2 that starts as zeros and is carried from call to call (Model); the two must agree with each other and with the device;
(b) a twin context in DENOISE_NONE that renders the same frame index: its read_ldr() and read_depth() are the screen and depth the
    pass reads (test_gpu_denoise.test_none_mode_shows_the_frame_itself), and np_restatement.temporal_reproject is applied to those.

After each call the screen (read_ldr), the history image just written (read_accum) and the depth image are compared; the image
NOT written cannot be read back, and is checked by the next call of the opposite parity, which reads it.

1. the kernel under hand-made RenderParameters: five sizes (one pixel, rows shorter than a wave, a second and a third x-block),
   eleven delta matrices and five frame_count sequences, and a chain whose pixels sit exactly ON the 0.1 threshold; what each case
   exercises is asserted on the restatement's own intermediates (section1_plan), on the CPU, before anything runs on the device;
2. the reference's own flow (host.PathTracingCamera) on every builder and upload route, both kernels, both accumulation modes, two
   scenes; the same calls queued; the depth output switched off;
3. an environment map with both kinds of MIS and a scene that moves between two calls, against the twin; the lens and the panorama,
   which the mode refuses (jpt_primary.cpp: it assumes one centre of projection and the pinhole): refused in the middle of a
   sequence, which then goes on as if nothing had been asked;
4. what restarts the history: jpt_accum_reset, a mode switch, a new size."""
import copy

import numpy as np
import pytest

from gdpathtracing_amd import capi, host, scenes, wire

import np_restatement as R
from test_gpu_camera import make_ctx
from test_gpu_tx_scene_changes import LENS, all_transforms, with_transform

pytestmark = pytest.mark.gpu

F = np.float32
BOUNCES = 2
KERNELS = [capi.KERNEL_WAVEFRONT, capi.KERNEL_REFERENCE_LAYOUT]
ACCUMS = [wire.ACCUM_REF_LDR8, wire.ACCUM_HDR_F32]
UPLOAD_NATIVE, UPLOAD_AS_GIVEN = "upload", "upload as given"


# ---- the yardsticks ----------------------------------------------------------------------------------------------------------------------------

_SCENES, _REFS, _TRACES = {}, {}, {}


def scene_of(name):
    """a copy of the named scene (a test may move its camera)"""
    if name not in _SCENES:
        _SCENES[name] = scenes.cornell_scene() if name == "cornell" else scenes.demo_scene(800)
    return copy.deepcopy(_SCENES[name])


def ref_of(oracle, name):
    if name not in _REFS:
        _REFS[name] = oracle.build_scene(scene_of(name))
    return _REFS[name]


def trace(oracle, name, cam, w, h, frame):
    """(screen rgba8, depth) of main.glsl for one frame: traced once, shared, never changed (the screen is handed out as a copy)"""
    key = (name, np.asarray(cam.transform, F).tobytes(), w, h, frame)
    if key not in _TRACES:
        rad, depth, _ = oracle.trace_frame(ref_of(oracle, name), scenes.camera_block(cam, w, h, frame_index=frame), w, h, BOUNCES)
        depth.setflags(write=False)
        _TRACES[key] = (oracle.screen_rgba8(rad), depth)
    screen, depth = _TRACES[key]
    return screen.copy(), depth


def view(cam, yaw_deg=0.0, offset=(0.0, 0.0, 0.0), pitch_deg=0.0, near=None):
    """`cam` (which looks down -z, unturned) turned about y, then about its own x, and moved; near: another near plane"""
    a = np.deg2rad(pitch_deg)
    rot_x = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    out = copy.deepcopy(cam)
    if near is not None:
        out.near = near
    out.transform = scenes.transform12(scenes.rot_y(yaw_deg) @ rot_x, np.asarray(cam.transform[9:12], np.float64) + np.asarray(offset, np.float64))
    return out


def params(delta, w, h, frame_count):
    """an 88-byte RenderParameters block written by hand"""
    p = np.zeros((), dtype=wire.TEMPORAL_PARAMS)
    p["deltaMatrix"] = np.asarray(delta, dtype=F).reshape(-1)
    p["width"], p["height"], p["frame_count"] = w, h, frame_count
    p["blendFactor"], p["nearPlane"], p["farPlane"] = 0.75, 0.01, 1000.0
    return p


class Model:
    """frameBuffer1 / frameBuffer2 of temporal_reprojection.glsl: zeros, then whatever the calls leave.  With an oracle the C
    restatement keeps a pair of its own, and after every call screen and both images must equal the numpy restatement's."""

    def __init__(self, w, h, oracle=None):
        self.fb = [np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)]
        self.oracle = oracle
        self.ofb = [np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)] if oracle is not None else None

    def step(self, p, screen, depth):
        """-> (screen after the pass, the history image written, the restatement's intermediates, whether the image the pass may
        read held anything)"""
        fc = int(p["frame_count"])
        read_nonzero = bool(self.fb[0 if fc % 2 == 0 else 1].any())
        detail = {}
        after, hist, which = R.temporal_reproject(p["deltaMatrix"], fc, screen, depth, self.fb[0], self.fb[1], detail)
        self.fb[which - 1] = hist
        if self.oracle is not None:
            o = np.ascontiguousarray(screen).copy()
            self.oracle.temporal_reproject(p, o, depth, self.ofb[0], self.ofb[1])
            assert np.array_equal(o, after), "the oracle and the numpy restatement disagree on the screen"
            assert np.array_equal(self.ofb[0], self.fb[0]) and np.array_equal(self.ofb[1], self.fb[1]), "... on the history images"
        return after, hist, detail, read_nonzero


def categories(detail, shape):
    """(pixels that took history, pixels rejected on depth, pixels that landed outside) of one call"""
    if not detail:   # frame_count == 0: nothing is reprojected
        return 0, 0, 0
    taken, inside = detail["taken"], detail["inside"]
    assert taken.shape == tuple(shape) and not (taken & ~inside).any()
    return int(taken.sum()), int((inside & ~taken).sum()), int((~inside).sum())


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    same = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else (a == b)
    return int((~same).reshape(a.shape[0] * a.shape[1], -1).any(axis=-1).sum()) if a.ndim >= 2 else int((~same).sum())


def assert_call(ctx, want_screen, want_hist, want_depth, what):
    got = (ctx.read_ldr(), ctx.read_accum(), ctx.read_depth())
    n = [differing(g, x) for g, x in zip(got, (want_screen, want_hist, want_depth))]
    print("%s: %d screen, %d history and %d depth pixels differ from the yardstick" % (what, n[0], n[1], n[2]))
    assert n == [0, 0, 0], "%s: screen differs at %d pixels, history at %d, depth at %d" % (what, n[0], n[1], n[2])
    return got


def uploaded_ctx(ref, w, h, kernel=capi.KERNEL_WAVEFRONT, accum=wire.ACCUM_REF_LDR8, as_given=False, mode=capi.DENOISE_TEMPORAL):
    ctx = host.Context(0)
    try:
        ctx.set_kernel(kernel)
        ctx.upload_reference_layout(ref.tri_geom, ref.tri_data, ref.materials, ref.bvh_nodes, ref.instances, ref.tlas_nodes, ref.textures,
                                    as_given=as_given)
        ctx.set_params(w, h, BOUNCES, accum)
        ctx.set_denoising_mode(mode)
    except Exception:
        ctx.close()
        raise
    return ctx


# ---- 1. the kernel under hand-made RenderParameters ----------------------------------------------------------------------------------------

SIZES = [(1, 1), (7, 5), (53, 37), (257, 3), (600, 2)]   # 257 and 600: a second and a third x-block of 256 threads, 1 and 88 of them alive
LARGER = SIZES[2:]
# The views a chain renders from, per size: (how far the scene's camera is moved along its axis first, view 1, view 2), a view being
# (yaw, pitch, offset) from there.  Moved INTO the box (its front is open, at z = 3; the scene's camera stands at z = 9.77, where
# four pixels of five see the sky at depth 1.0 and the two strips see nothing else), so that the depth image varies from pixel to
# pixel.  A step's delta keeps the bottom row 0 0 0 1 (scenes.temporal_delta), so cz is the previous clip-space z WITHOUT its
# divide: it leaves the depth image by about (the step along the view axis) / (twice the distance), plus sin(turn) times the
# pixel's tangent -- which is how a dolly or a turn pushes pixels over the 0.1 threshold.  View 1 was searched on the CPU for a
# step that has all three kinds of pixel at once (one pixel cannot: at 1 x 1 view 1 takes history and view 2 is rejected); the
# strips need a steep pitch for a row to leave the image.  section1_plan asserts what came of it.
DOLLY = (2.0, 0.0, (0.1, 0.05, -0.8))
SECTION1_VIEWS = {
    (1, 1): (-2.0, (0.0, 0.0, (0.1, 0.05, -0.3)), (0.0, 0.0, (0.1, 0.05, -1.5))),
    (7, 5): (-7.0, (-8.0, -20.0, (0.3, 0.05, -0.3)), DOLLY),
    (53, 37): (-7.0, (-8.0, -20.0, (0.3, 0.05, -0.3)), DOLLY),
    (257, 3): (-7.0, (0.0, -20.0, (0.0, 0.05, 0.0)), DOLLY),
    (600, 2): (-7.0, (0.05, -35.0, (0.1, 0.05, -0.3)), DOLLY),
}
# (frame_count, delta, view) per call; the frame index of the render is the call's number, from 1
CHAINS = {
    "2_3_4_5": [(2, "identity", 0), (3, "identity", 0), (4, "step", 1), (5, "fraction", 1)],
    "0_first_and_0_later": [(0, "random", 0), (3, "three_screens", 0), (0, "all_nan", 0), (2, "z_offset_a", 0), (3, "z_offset_b", 0)],
    "2_2_3_3": [(2, "identity", 0), (2, "step", 2), (3, "random", 2), (3, "zero_w", 2)],
    "7_then_2": [(7, "identity", 0), (2, "nan", 0), (3, "huge", 0), (4, "identity", 0)],
    "wraparound": [(0xFFFFFFFE, "identity", 0), (0xFFFFFFFF, "step", 2), (0xFFFFFFFE, "fraction", 2)],
    "at_the_threshold": [(2, "identity", 3), (3, "z_exact", 3), (4, "z_exact", 3)],
}
# View 3, for the last chain: |depth - cz| EQUAL to 0.1f.  Around the scene's depths (1 - 0.01 / distance: in [0.5, 1), a grid of 2^-24)
# no offset gets there: depth - cz is exact (Sterbenz) and a multiple of 2^-24, and 0.1f = 13421773 * 2^-27 is not.  With the near
# plane at 1 and the camera 1.05 in front of the right wall the depths 1.001 (1 - 1 / distance) around the view axis are below
# 0.225; there d - 0.1f is exact, and so is d - (d - 0.1f) = 0.1f: with the z offset -0.1f those pixels sit ON the threshold, which
# `<` rejects.
WALL_VIEW = dict(yaw_deg=-90.0, offset=(1.95, 0.5, -11.27), near=1.0)
KINDS = sorted({k for calls in CHAINS.values() for _, k, _ in calls} - {"all_nan"})   # (all_nan rides on frame_count 0: never read)
assert all(len(c) <= 8 for c in CHAINS.values())


def hand_delta(kind, w, h, vp_from=None, vp_to=None, offset=None, seed=0):
    """the 16 floats, column-major"""
    m = np.eye(4, dtype=np.float64)   # row-major here
    if kind == "step":                # a real camera step
        return scenes.temporal_delta(vp_from, vp_to)
    if kind == "random":              # anything at all, a projective row included
        return np.random.RandomState(seed).uniform(-1.0, 1.0, size=16).astype(F)
    if kind == "all_nan":
        return np.full(16, np.nan, F)
    if kind == "three_screens":       # every position lands outside
        m[0, 3] = 6.0
    elif kind == "fraction":          # 3/4 of a pixel to the left and up: column 0 has u * W = -0.25, row 0 has v * H = -0.25
        m[0, 3], m[1, 3] = -1.5 / w, 1.5 / h
    elif kind.startswith("z_offset"):
        m[2, 3] = float(offset)       # (a float32 value: the conversion below is exact)
    elif kind == "z_exact":
        m[2, 3] = -float(F(0.1))
    elif kind == "zero_w":            # division by zero: +-inf and NaN into the integer conversion
        m[3, :] = 0.0
    elif kind == "nan":               # cx is NaN everywhere: the pinned conversion makes texel column 0 of it
        m[0, 0] = np.nan
    elif kind == "huge":              # u * W far beyond int32: saturation, both signs
        m[0, 0] = 1e30
    else:
        assert kind == "identity", kind
    return m.T.reshape(-1).astype(F)


def threshold_scan(depth):
    """the identity with a z offset of +-(0.1f + k ulp), |k| <= 8 -> [(offset, the pixels the restatement lets take history)].  Every
    pixel lands on itself, so the test is |d - fl(d + offset)| < 0.1f: which side a pixel falls on depends on how d + offset rounds."""
    h, w = depth.shape
    base, out = F(0.1), []
    ulp = np.spacing(base)
    for sign in (1.0, -1.0):
        for k in range(-8, 9):
            off = F(sign) * F(base + F(k) * ulp)
            detail = {}
            R.temporal_reproject(hand_delta("z_offset", w, h, offset=off), 2, np.zeros((h, w, 4), np.uint8), depth,
                                 np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), detail)
            assert detail["inside"].all()
            out.append((off, detail["taken"]))
    return out


def pick_thresholds(depth_a, depth_b):
    """the two offsets of the threshold calls -> (offset a, offset b, fallback).  Kept: offsets for which the restatement accepts
    some pixels and rejects others of the same image, the most evenly split one of each sign where there is one.  Where fewer than
    two offsets split an image (fallback): the pair that flips the most pixels between them."""
    scan_a, scan_b = threshold_scan(depth_a), threshold_scan(depth_b)
    n = depth_a.size

    def split(scan):
        return sorted(((min(int(t.sum()), n - int(t.sum())), float(off)) for off, t in scan if 0 < int(t.sum()) < n), reverse=True)
    mixed_a, mixed_b = split(scan_a), split(scan_b)
    if mixed_a and mixed_b:
        a = next((off for _, off in mixed_a if off > 0), mixed_a[0][1])
        rest = [(s, off) for s, off in mixed_b if off != a]
        if rest:
            return F(a), F(next((off for _, off in rest if off < 0), rest[0][1])), False
    flips, a, b = max(((int((ta != tb).sum()), float(oa), float(ob)) for oa, ta in scan_a for ob, tb in scan_b), key=lambda t: t[0])
    assert flips > 0, "no pair of offsets around 0.1f flips a pixel"
    return F(a), F(b), True


_PLANS = {}


def section1_plan(oracle, size):
    """Every chain of one size on the CPU, with yardstick (a): per call the inputs (view, frame index, params) and what the device
    must show after it.  Asserts, on the restatement's intermediates, that the cases exercise what they are there for."""
    if size in _PLANS:
        return _PLANS[size]
    w, h = size
    into, view1, view2 = SECTION1_VIEWS[size]
    base = view(scene_of("cornell").camera, 0.0, (0.0, 0.0, into))
    cams = [base] + [view(base, yaw, off, pitch) for yaw, pitch, off in (view1, view2)] + [view(scene_of("cornell").camera, **WALL_VIEW)]
    vps = [scenes.view_projection(c, w, h) for c in cams]
    plan = {"chains": {}, "fallback": False, "totals": np.zeros(3, np.int64)}
    read_history = {k: False for k in KINDS}        # per delta: some call read a non-zero history image with it
    steps = np.zeros(3, np.int64)                   # the camera-step calls' categories, summed
    all_three = 0                                   # ... and how many of those calls had all three at once
    for name, calls in CHAINS.items():
        model = Model(w, h, oracle)
        out, last_view = [], 0
        for frame, (fc, kind, vi) in enumerate(calls, 1):
            screen, depth = trace(oracle, "cornell", cams[vi], w, h, frame)
            offset = None
            if kind == "z_offset_a":
                depth_b = trace(oracle, "cornell", cams[vi], w, h, frame + 1)[1]
                za, zb, plan["fallback"] = pick_thresholds(depth, depth_b)
                offset = za
            elif kind == "z_offset_b":
                offset = zb
            p = params(hand_delta(kind, w, h, vps[last_view], vps[vi], offset, seed=w * 1000 + h), w, h, fc)
            before = [f.copy() for f in model.fb]
            after, hist, detail, read_nonzero = model.step(p, screen, depth)
            cat = categories(detail, (h, w))
            if fc == 0:   # the history is not read: the image written is the frame itself, whatever the other images hold
                cur = screen[..., :3].astype(F) / F(255.0)
                assert not detail and np.array_equal(hist[..., :3], cur * (F(1.0) - F(0.75)) + cur * F(0.75))
            else:
                plan["totals"] += cat
                read_history[kind] = read_history[kind] or read_nonzero
            if fc == 2 and name == "2_2_3_3" and frame == 2:   # the same parity twice: the pass reads the OLDER image, still zeros
                assert not read_nonzero and before[1].any()
            if kind == "step":
                steps += cat
                all_three += int(min(cat) > 0)
            elif kind == "three_screens":
                assert cat == (0, 0, w * h)
            elif kind == "fraction":
                edge = ((detail["uw"] > -1) & (detail["uw"] < 0)) | ((detail["vh"] > -1) & (detail["vh"] < 0))
                both = (detail["uw"] > -1) & (detail["uw"] < 0) & (detail["vh"] > -1) & (detail["vh"] < 0)
                assert (edge & detail["taken"]).any() and (both & detail["taken"])[0, 0], "no pixel in (-1, 0) takes history"
                assert edge[:, 0].all() and edge[0, :].all() and (detail["px"][:, 0] == 0).all() and (detail["py"][0, :] == 0).all()
            elif kind.startswith("z_offset") and not plan["fallback"]:
                assert 0 < cat[0] < w * h and cat[2] == 0, "the threshold call does not split the image"
            elif kind == "z_exact":
                on = np.abs(depth[detail["py"], detail["px"]] - detail["cz"]) == F(0.1)
                assert on.any() and not (on & detail["taken"]).any() and cat[2] == 0, "no pixel sits on the threshold"
                plan["on_threshold"] = plan.get("on_threshold", 0) + int(on.sum())
            elif kind == "nan":
                assert (detail["px"] == 0).all() and cat[0] > 0    # NaN -> texel column 0, and its history is taken
            elif kind == "huge" and w > 1:   # (the one column of w == 1 has nx == 0: nothing to scale)
                assert (detail["px"] == -2 ** 31).any() and (detail["px"] == 2 ** 31 - 1).any() and cat[2] > 0
            elif kind == "zero_w":
                assert not np.isfinite(detail["uw"]).any() and not np.isfinite(detail["vh"]).any() and cat[0] == 0
            assert np.isfinite(hist).all()
            out.append({"frame": frame, "cam": cams[vi], "params": p, "kind": kind, "screen": after, "hist": hist, "depth": depth, "cat": cat})
            last_view = vi
        plan["chains"][name] = out
    if plan["fallback"]:   # (one offset is accepted and the other rejected at the pixels that flip)
        assert size in THRESHOLD_FALLBACK, "no offset splits the image at %r" % (size,)
    else:
        assert size not in THRESHOLD_FALLBACK
    missing = [k for k, seen in read_history.items() if not seen]
    assert not missing, "never applied to a non-zero history: %s" % missing
    assert steps[0] > 0 and steps[1] > 0, "the camera steps at %r: %s" % (size, steps)
    if size in LARGER:
        assert steps[2] > 0 and all_three > 0, "the camera steps at %r: %s, %d calls with all three" % (size, steps, all_three)
    plan["steps"] = steps
    _PLANS[size] = plan
    return plan


THRESHOLD_FALLBACK = [(1, 1)]


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_under_hand_made_parameters(oracle, hiplib, size, chain):
    """Cornell, uploaded from the oracle's arrays; params blocks written by hand (wire.TEMPORAL_PARAMS), copied verbatim by
    jpt_set_temporal_params.  The threshold calls use two offsets 0.1f +- k ulp for which the restatement accepts some pixels and
    rejects others of the same image; at 1 x 1 no offset can split the one pixel, and the pair that flips it is used instead
    (THRESHOLD_FALLBACK)."""
    w, h = size
    plan = section1_plan(oracle, size)   # (asserts the conditions on the inputs, on the CPU, before the device runs anything)
    print("size %d x %d, all chains: %d pixels took history, %d were rejected on depth, %d landed outside; camera steps: %s; on the threshold: %d"
          % (w, h, *plan["totals"], plan["steps"].tolist(), plan["on_threshold"]))
    ctx = uploaded_ctx(ref_of(oracle, "cornell"), w, h)
    try:
        for c in plan["chains"][chain]:
            ctx.set_camera(scenes.camera_block(c["cam"], w, h))
            ctx.set_temporal_params(c["params"])
            ctx.render(1, c["frame"])
            what = "%s, call %d (%s, frame_count %d): %s took / rejected / outside" % (chain, c["frame"], c["kind"], int(c["params"]["frame_count"]), c["cat"])
            _, got_hist, _ = assert_call(ctx, c["screen"], c["hist"], c["depth"], what)
            if c["kind"] in ("zero_w", "nan", "huge"):
                assert np.isfinite(got_hist[np.isfinite(c["hist"])]).all()
    finally:
        ctx.close()


# ---- 2. the reference's own flow -----------------------------------------------------------------------------------------------------------

FLOW_W, FLOW_H, FLOW_FRAMES = 96, 64, 8
FLOW_SCENES = ["cornell", "demo800"]


def flow_pose(base, frame):
    """frames 1 to 5: from in front of the box, a turn of 5 degrees and a translation per frame (the turn takes the pixels at the sides over
    the depth threshold, see SECTION1_VIEWS); frames 6 to 8 stand where frame 5 was"""
    k = min(frame, 5) - 1
    return view(base, 5.0 * k, (0.12 * k, 0.04 * k, -4.0 - 0.5 * k))


_FLOWS = {}


def flow_plan(oracle, name):
    """the eight frames of PathTracingCamera::render in TEMPORAL_REPROJECTION mode, with yardstick (a)"""
    if name in _FLOWS:
        return _FLOWS[name]
    w, h = FLOW_W, FLOW_H
    base = scene_of(name).camera
    model, t, out = Model(w, h, oracle), host.TemporalReprojection(w, h), []
    for frame in range(1, FLOW_FRAMES + 1):
        cam = flow_pose(base, frame)
        screen, depth = trace(oracle, name, cam, w, h, frame)
        tp = t.render(scenes.view_projection(cam, w, h))
        assert int(tp["frame_count"]) == frame + 1
        after, hist, detail, read_nonzero = model.step(tp, screen, depth)
        cat = categories(detail, (h, w))
        if 2 <= frame <= 5:   # the moving frames that have a frame before them
            assert min(cat) > 0 and read_nonzero, "%s, frame %d: %s took / rejected / outside" % (name, frame, cat)
        if frame > 5:         # standing: every pixel lands on itself
            assert cat[2] == 0 and cat[0] > 0
        out.append({"frame": frame, "cam": cam, "params": tp, "screen": after, "hist": hist, "depth": depth, "cat": cat, "unblended": screen})
    # history really is used: the last image differs from the no-history blend
    assert np.abs(out[-1]["hist"][..., :3] - out[-1]["unblended"][..., :3].astype(F) / F(255.0)).max() > 0
    _FLOWS[name] = out
    return out


class UploadedGroup:
    """what PathTracingCamera asks of a GeometryGroup3D, on the upload route"""

    def __init__(self, scene, ref, as_given):
        self.scene, self.ref, self.as_given = scene, ref, as_given

    def build(self, ctx):
        r = self.ref
        ctx.upload_reference_layout(r.tri_geom, r.tri_data, r.materials, r.bvh_nodes, r.instances, r.tlas_nodes, r.textures, as_given=self.as_given)


@pytest.mark.parametrize("accum", ACCUMS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH, UPLOAD_NATIVE, UPLOAD_AS_GIVEN])
@pytest.mark.parametrize("name", FLOW_SCENES)
def test_reference_flow(oracle, hiplib, name, builder, kernel, accum):
    """Eight frames of host.PathTracingCamera.render: the camera turns and moves for five frames and then stands.  Screen, history
    image and depth equal the oracle's after every frame, on every builder and upload route, both kernels and both accumulation
    modes (the mode does not read the accumulation mode: every case meets the same yardstick)."""
    plan = flow_plan(oracle, name)
    sc = scene_of(name)
    if builder in (UPLOAD_NATIVE, UPLOAD_AS_GIVEN):
        group = UploadedGroup(sc, ref_of(oracle, name), builder == UPLOAD_AS_GIVEN)
    else:
        group = host.GeometryGroup3D(sc, builder)
    cam = host.PathTracingCamera(group, 0, max_bounces=BOUNCES, accum_mode=accum)
    try:
        cam.ctx.set_kernel(kernel)
        cam.denoising_mode = cam.TEMPORAL_REPROJECTION
        cam.init(FLOW_W, FLOW_H)
        for c in plan:
            sc.camera.transform = c["cam"].transform.copy()
            got_screen = cam.render()
            assert cam.temporal_reprojection.params.tobytes() == c["params"].tobytes()
            got = assert_call(cam.ctx, c["screen"], c["hist"], c["depth"], "%s, frame %d: %s took / rejected / outside" % (name, c["frame"], c["cat"]))
            assert np.array_equal(got_screen, got[0])
    finally:
        cam.ctx.close()


def flow_ctx(name, builder, w=FLOW_W, h=FLOW_H):
    sc = scene_of(name)
    ctx = host.Context(0)
    try:
        ctx.build_scene(sc, builder)
        ctx.set_params(w, h, BOUNCES, wire.ACCUM_REF_LDR8)
        ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
    except Exception:
        ctx.close()
        raise
    return ctx


def run_flow(ctx, plan, asynchronous):
    for c in plan:
        ctx.set_camera(scenes.camera_block(c["cam"], FLOW_W, FLOW_H))
        ctx.set_temporal_params(c["params"])
        ctx.render(1, c["frame"], asynchronous=asynchronous)
    ctx.sync()
    return ctx.read_ldr(), ctx.read_accum(), ctx.read_depth()


@pytest.mark.parametrize("builder", [capi.BUILD_REFERENCE_EXACT, capi.BUILD_SAH])
@pytest.mark.parametrize("name", FLOW_SCENES)
def test_queued_renders_equal_the_blocking_run(oracle, hiplib, name, builder):
    """The same eight calls as render(1, k, asynchronous=True), jpt_set_temporal_params before each and no read-back in between:
    each pass must run behind its own render's last write and ahead of the next render's first, with the params block it was
    queued with.  Screen, history and depth at the end equal the blocking run's (and so the oracle's)."""
    plan = flow_plan(oracle, name)
    out = []
    for asynchronous in (False, True):
        ctx = flow_ctx(name, builder)
        try:
            out.append(run_flow(ctx, plan, asynchronous))
        finally:
            ctx.close()
    n = [differing(a, b) for a, b in zip(out[1], out[0])]
    print("queued against blocking: %d screen, %d history and %d depth pixels differ" % tuple(n))
    assert n == [0, 0, 0]
    last = plan[-1]
    assert [differing(a, b) for a, b in zip(out[0], (last["screen"], last["hist"], last["depth"]))] == [0, 0, 0]


@pytest.mark.parametrize("asynchronous", [False, True])
def test_depth_output_off_changes_nothing(oracle, hiplib, asynchronous):
    """jpt_set_outputs(depth off): the temporal pass is the depth image's one reader, so the render still produces it -- same screen,
    same history, and jpt_read_depth_f32 answers with the frame's depth, not JPT_E_STATE (do_render_batch: want_depth, depth_valid)."""
    plan = flow_plan(oracle, "cornell")
    ctx = flow_ctx("cornell", capi.BUILD_REFERENCE_EXACT)
    try:
        ctx.set_outputs(depth=False)
        got = run_flow(ctx, plan, asynchronous)
        last = plan[-1]
        assert [differing(a, b) for a, b in zip(got, (last["screen"], last["hist"], last["depth"]))] == [0, 0, 0]
        assert np.array_equal(ctx.read_depth(), last["depth"])   # the pin: valid, and this frame's
    finally:
        ctx.close()


# ---- 3. newer render families and a moving scene, against the twin ---------------------------------------------------------------------------

TWIN_W, TWIN_H, TWIN_CALLS = 48, 32, 4
BLOCK = 2   # cornell_scene's short block


def twin_pose(base, call):
    return view(base, 5.0 * (call - 1), (0.1 * (call - 1), 0.03 * (call - 1), -4.0 - 0.5 * (call - 1)))   # (like flow_pose)


def twin_pair(sc, lighting="sky", builder=capi.BUILD_SAH):
    """(the context under test, its twin in DENOISE_NONE): the same scene, lighting and builder"""
    ctx = make_ctx(sc, None, TWIN_W, TWIN_H, builder=builder, bounces=3, lighting=lighting)
    try:
        twin = make_ctx(sc, None, TWIN_W, TWIN_H, builder=builder, bounces=3, lighting=lighting)
    except Exception:
        ctx.close()
        raise
    ctx.set_denoising_mode(capi.DENOISE_TEMPORAL)
    twin.set_denoising_mode(capi.DENOISE_NONE)
    return ctx, twin


class TwinChain:
    """yardstick (b), call by call"""

    def __init__(self, ctx, twin, base):
        self.ctx, self.twin, self.base = ctx, twin, base
        self.model, self.t = Model(TWIN_W, TWIN_H), host.TemporalReprojection(TWIN_W, TWIN_H)
        self.cats, self.calls = [], 0

    def inputs(self, call):
        """the twin's screen and depth of this call's frame, as the scene stands"""
        self.twin.set_camera(scenes.camera_block(twin_pose(self.base, call), TWIN_W, TWIN_H))
        self.twin.render(1, call)
        return self.twin.read_ldr(), self.twin.read_depth()

    def call(self, what):
        self.calls += 1
        cam = twin_pose(self.base, self.calls)
        tp = self.t.render(scenes.view_projection(cam, TWIN_W, TWIN_H))
        screen, depth = self.inputs(self.calls)
        self.ctx.set_camera(scenes.camera_block(cam, TWIN_W, TWIN_H))
        self.ctx.set_temporal_params(tp)
        self.ctx.render(1, self.calls)
        after, hist, detail, _ = self.model.step(tp, screen, depth)
        self.cats.append(categories(detail, (TWIN_H, TWIN_W)))
        assert_call(self.ctx, after, hist, depth, "%s, call %d: %s took / rejected / outside" % (what, self.calls, self.cats[-1]))
        return tp, screen, depth, after, hist


def test_environment_map_with_both_kinds_of_mis(hiplib):
    """test_gpu_camera.make_ctx's sun_map() with environment and light sampling on MIS: renders the oracle does not trace"""
    sc = scene_of("cornell")
    ctx, twin = twin_pair(sc, "map_mis_emitters")
    sky = make_ctx(sc, None, TWIN_W, TWIN_H, bounces=3)
    try:
        chain = TwinChain(ctx, twin, sc.camera)
        for _ in range(TWIN_CALLS):
            _, screen, _, _, _ = chain.call("map + MIS")
        assert sum(c[0] for c in chain.cats[1:]) > 0, "no call took history"
        # and the map is what lit these frames: under the gradient sky the same frame is another image
        sky.set_denoising_mode(capi.DENOISE_NONE)
        sky.set_camera(scenes.camera_block(twin_pose(sc.camera, TWIN_CALLS), TWIN_W, TWIN_H))
        sky.render(1, TWIN_CALLS)
        assert differing(sky.read_ldr(), screen) > 0
    finally:
        for c in (ctx, twin, sky):
            c.close()


REFUSED = {
    "lens": (lambda c: c.set_lens(*LENS), lambda c: c.set_lens(0.0, 1.0), "one centre of projection"),
    "equirect": (lambda c: c.set_camera_model(capi.CAMERA_EQUIRECT), lambda c: c.set_camera_model(capi.CAMERA_PINHOLE), "assumes the pinhole"),
}


@pytest.mark.parametrize("family", list(REFUSED))
def test_lens_and_panorama_are_refused_and_leave_the_history_alone(hiplib, family):
    """The thin lens and CAMERA_EQUIRECT have no single centre of projection to reproject through: the mode refuses them
    (resolve_primary; test_gpu_lens, test_gpu_camera and test_gpu_primary_rays pin the refusals).  Here the refusal comes between
    calls 2 and 3 of a sequence, blocking and queued: nothing was rendered, no pass ran, and calls 3 and 4 go on from the history
    calls 1 and 2 left -- checked against the twin, which never saw the lens or the model."""
    switch_on, switch_off, why = REFUSED[family]
    sc = scene_of("cornell")
    ctx, twin = twin_pair(sc)
    try:
        chain = TwinChain(ctx, twin, sc.camera)
        chain.call(family)
        chain.call(family)
        hist = ctx.read_accum()
        switch_on(ctx)
        for asynchronous in (False, True):
            with pytest.raises(capi.JptError, match=why):
                ctx.render(1, 3, asynchronous=asynchronous)
        assert np.array_equal(ctx.read_accum(), hist)
        switch_off(ctx)
        chain.call(family)
        chain.call(family)
        assert sum(c[0] for c in chain.cats[2:]) > 0, "calls 3 and 4 took no history"
    finally:
        ctx.close()
        twin.close()


def test_scene_moves_between_two_calls(hiplib):
    """jpt_scene_refit_tlas moves Cornell's short block between calls 2 and 3 (BUILD_SAH_WATERTIGHT; the twin gets the same refit).
    Calls 3 and 4 show the moved block over the history of the unmoved one, and the move altered both the screen and the history:
    they differ from what the pass makes of the same frame of the unmoved scene."""
    sc = scene_of("cornell")
    t = np.asarray(sc.instances[BLOCK].transform, F).copy()
    t[9:12] += np.array([-0.8, 0.6, 0.5], F)
    moved = all_transforms(with_transform(sc, BLOCK, t))
    ctx, twin = twin_pair(sc, builder=capi.BUILD_SAH_WATERTIGHT)
    try:
        chain = TwinChain(ctx, twin, sc.camera)
        chain.call("unmoved")
        chain.call("unmoved")
        unmoved_screen, unmoved_depth = chain.inputs(3)          # frame 3 as it would have been
        unmoved = copy.deepcopy(chain.model)
        ctx.refit_tlas(moved)
        twin.refit_tlas(moved)
        tp, screen, depth, after, hist = chain.call("moved")
        want_screen, want_hist, _, _ = unmoved.step(tp, unmoved_screen, unmoved_depth)
        n = differing(screen, unmoved_screen), differing(after, want_screen), differing(hist, want_hist)
        print("the move changed %d pixels of the frame, %d of the screen after the pass and %d of the history" % n)
        assert min(n) > 0
        chain.call("moved")
        assert sum(c[0] for c in chain.cats[2:]) > 0
    finally:
        ctx.close()
        twin.close()


# ---- 4. state --------------------------------------------------------------------------------------------------------------------------------

S = 32
NO_PASS = "no temporal pass has run since the last reset"


def state_ctx(w=S, h=S):
    sc = scene_of("cornell")
    ctx = flow_ctx("cornell", capi.BUILD_SAH, w, h)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    return ctx


def state_call(ctx, frame_count, frame, w=S, h=S):
    """the identity delta: every pixel takes whatever the image of that parity holds at its own place"""
    ctx.set_temporal_params(params(hand_delta("identity", w, h), w, h, frame_count))
    ctx.render(1, frame)
    return ctx.read_ldr(), ctx.read_accum()


def first_call_of_a_fresh_context(frame_count, frame, w=S, h=S):
    ctx = state_ctx(w, h)
    try:
        return state_call(ctx, frame_count, frame, w, h)
    finally:
        ctx.close()


RESTARTS = {
    "accum_reset": (lambda c: c.accum_reset(), (S, S)),
    "mode_switch": (lambda c: (c.set_denoising_mode(capi.DENOISE_PROGRESSIVE), c.set_denoising_mode(capi.DENOISE_TEMPORAL)), (S, S)),
    "smaller_size": (lambda c: c.set_params(24, 20, BOUNCES, wire.ACCUM_REF_LDR8), (24, 20)),
    "larger_size": (lambda c: c.set_params(40, 48, BOUNCES, wire.ACCUM_REF_LDR8), (40, 48)),
    "same_pixel_count": (lambda c: c.set_params(16, 64, BOUNCES, wire.ACCUM_REF_LDR8), (16, 64)),   # d_hist1.n stays what it was
}


@pytest.mark.parametrize("frame_count", [2, 3])
@pytest.mark.parametrize("how", list(RESTARTS))
def test_what_restarts_the_history(hiplib, how, frame_count):
    """After two calls both history images hold a frame.  jpt_accum_reset, a switch of mode away and back, and jpt_set_params to
    another size each make a new TemporalReprojection of the context: jpt_read_accum_f32 is refused until a pass has run, and the
    next call -- of either parity -- equals the first call of a fresh context, because the history is zeros again."""
    restart, (w, h) = RESTARTS[how]
    ctx = state_ctx()
    try:
        state_call(ctx, 2, 1)
        state_call(ctx, 3, 2)
        if (w, h) == (S, S):   # what the call would have shown over the history that was there
            went_on = state_ctx()
            try:
                state_call(went_on, 2, 1)
                state_call(went_on, 3, 2)
                stale = state_call(went_on, frame_count, 3)
            finally:
                went_on.close()
        restart(ctx)
        with pytest.raises(capi.JptError, match=NO_PASS):
            ctx.read_accum()
        if (w, h) != (S, S):
            ctx.set_camera(scenes.camera_block(scene_of("cornell").camera, w, h))
        got = state_call(ctx, frame_count, 3, w, h)
        want = first_call_of_a_fresh_context(frame_count, 3, w, h)
        n = differing(got[0], want[0]), differing(got[1], want[1])
        print("%s: %d screen and %d history pixels differ from a fresh context's first call" % (how, n[0], n[1]))
        assert n == (0, 0)
        assert 0 < want[1][..., :3].max() <= 0.25   # zeros for history: the image written is a quarter of the frame
        if (w, h) == (S, S):
            assert differing(stale[1], want[1]) > 0
    finally:
        ctx.close()


def test_params_of_another_size_are_still_refused_after_a_valid_call(hiplib):
    ctx = state_ctx()
    try:
        state_call(ctx, 2, 1)
        _, hist = state_call(ctx, 3, 2)
        for w, h in ((16, S), (S, 16), (S + 1, S), (0, 0)):
            ctx.set_temporal_params(params(hand_delta("identity", S, S), w, h, 4))
            for asynchronous in (False, True):
                with pytest.raises(capi.JptError, match="width/height"):
                    ctx.render(1, 3, asynchronous=asynchronous)
        assert np.array_equal(ctx.read_accum(), hist)   # nothing ran
        went_on = state_ctx()
        try:
            state_call(went_on, 2, 1)
            state_call(went_on, 3, 2)
            want = state_call(went_on, 4, 3)
        finally:
            went_on.close()
        got = state_call(ctx, 4, 3)
        assert differing(got[0], want[0]) == 0 and differing(got[1], want[1]) == 0
    finally:
        ctx.close()
