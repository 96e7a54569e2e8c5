# What jpt_scene_rebuild_tlas costs and buys, through the C ABI in one process, on grids of 256, 4096 and 32 761 instances of one mesh
# (scenes.instanced_scene without its two planes) whose transforms are permuted by seeded shuffles.  After four untimed rounds and
# 100 ms of the workload's own queued renders (the clocks, as bench.py preheats), the median of `reps` runs (default 15), min .. max, of
#   host       the wall time the host spends inside jpt_scene_rebuild_tlas, jpt_scene_refit_tlas and jpt_scene_update_tlas;
#   step       a queued "call, 1920 x 1080 render" step, per step of a run of six, for each of the three calls;
#   counters   inst_visits / tlas_expand of one counted render after each call, against a fresh JPT_BUILD_SAH commit of the shuffled scene.
# With JPT_LIB naming a library without jpt_scene_rebuild_tlas (the parent's) the rebuild rows are left out: the refit-only step on
# that library is the figure the feature must leave where it was.  Arguments: the instance counts' grid sides (default 16 64 181);
# `kernels` first: only fifteen rebuilds per size and nothing timed, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
args = sys.argv[1:]
kernels_only = bool(args) and args[0] == "kernels"
sides = [int(a) for a in args[1 if kernels_only else 0:]] or [16, 64, 181]
reps = 15
have_rebuild = hasattr(capi.lib(), "jpt_scene_rebuild_tlas")
W, H, FRAMES, BOUNCES, STEPS = 1920, 1080, 2, 3, 6


def stats(v):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def preheat(ctx):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 100.0:
        for _ in range(4):
            ctx.render(FRAMES, 1, asynchronous=True)
        ctx.sync()


def grid(side):
    sc = scenes.instanced_scene(n_side=side, n_unique=1, tris_per_mesh=64)
    sc.instances = sc.instances[2:]
    return sc


def context(sc):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(W, H, BOUNCES, capi.ACCUM_REF_LDR8)
    ctx.set_camera(scenes.camera_block(sc.camera, W, H))
    return ctx


def counters(ctx):
    ctx.accum_reset()
    ctx.render(FRAMES, 1, counted=True)
    st = ctx.stats()
    return int(st["inst_visits"]), int(st["tlas_expand"])


for side in sides:
    sc = grid(side)
    n = len(sc.instances)
    base = np.stack([np.asarray(i.transform, np.float32) for i in sc.instances])
    shuffles = [base[np.random.RandomState(2024 + k).permutation(n)] for k in range(2)]
    ctx = context(sc)
    calls = {"refit": lambda t: ctx.refit_tlas(t), "update": lambda t: (ctx.refit_tlas(t), ctx.update_tlas())}
    if have_rebuild:
        calls["rebuild"] = lambda t: ctx.rebuild_tlas(t)
    if kernels_only:
        for k in range(reps):
            ctx.rebuild_tlas(shuffles[k % 2])
            ctx.sync()
        ctx.close()
        continue
    print("## %d instances (%s)" % (n, os.environ.get("JPT_LIB", "this library")))
    rows = {}
    for name, call in calls.items():
        for k in range(4):
            call(shuffles[k % 2]); ctx.render(FRAMES, 1, asynchronous=True); ctx.sync()
        host_ms, step_ms = [], []
        preheat(ctx)
        for k in range(reps):
            if name == "update":   # the host's time in jpt_scene_update_tlas alone, behind a refit that made the TLAS dirty
                ctx.refit_tlas(shuffles[k % 2]); ctx.sync()
                t0 = time.perf_counter(); ctx.update_tlas()
            else:
                t0 = time.perf_counter(); call(shuffles[k % 2])
            host_ms.append((time.perf_counter() - t0) * 1e3)
            ctx.sync()
        preheat(ctx)
        for k in range(reps):
            t0 = time.perf_counter()
            for s in range(STEPS):
                call(shuffles[(k + s) % 2])
                ctx.accum_reset()
                ctx.render(FRAMES, 1, asynchronous=True)
            ctx.sync()
            step_ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
        call(shuffles[0]); ctx.sync()
        rows[name] = (stats(host_ms), stats(step_ms), counters(ctx))
    ctx.close()
    import copy
    moved = copy.deepcopy(sc)
    for i, inst in enumerate(moved.instances):
        inst.transform = shuffles[0][i]
    fresh = context(moved)
    want = counters(fresh)
    fresh.close()
    print("| call | host time in the call | queued call + %d x %d render, per step | inst_visits | tlas_expand | vs fresh SAH commit |" % (W, H))
    print("|---|---|---|---|---|---|")
    for name, (h, s, c) in rows.items():
        print("| %s | %s | %s | %d | %d | %.2fx / %.2fx |" % (name, h, s, c[0], c[1], c[0] / want[0], c[1] / want[1]))
    print("| fresh commit | | | %d | %d | |" % want)
