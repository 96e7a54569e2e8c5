# What jpt_set_bake_directional costs: the demo scene's atlas (one grid cell per (instance, surface), rasterised on the device as
# tools/bake_rate.py does) at 1024 x 1024 and 2048 x 2048, 16 frames per render, 4 bounces, JPT_ACCUM_REF_LDR8, through the C ABI in one
# process.  After four untimed rounds and 100 ms of the workload's own queued renders (the clocks, as bench.py preheats), the median of
# `reps` runs (default 15), min .. max, of
#   queued render   wall time per render of a queue of 8 renders and a sync, the switch off and on;
#   blocking render jpt_stats.last_render_ms of a blocking render, the switch off and on;
#   finish          wall time of jpt_bake_finish and of jpt_bake_finish_directional, each with a sync.
# With JPT_LIB naming a library without the call (the parent's) only the switch-off rows are timed: that is the baseline.
#   python tools/bake_directional_rate.py [reps] [sizes, e.g. 1024,2048]
# The kernels' own times: run the same under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bake_directional_rate.py trace`
# (15 queued renders per size with the switch on, behind the warm-up), then
#   python tools/bake_directional_rate.py kernels DIR
# prints the median, min .. max of bake_moments and wf2_accumulate over those launches, per size (the two grow with the texel count).
import csv, glob, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def stats(v):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    per = {}
    for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = "bake_moments" if "bake_moments" in name else ("wf2_accumulate" if "wf2_accumulate" in name else None)
            if key:
                grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
                per.setdefault((key, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print("| kernel | grid (threads) | launches | last 15 launches: median (min .. max) |")
    print("|---|---|---|---|")
    for (key, grid), v in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("| %s | %s | %d | %s |" % (key, grid, len(v), stats(v[-15:])))
    sys.exit(0)

from gdpathtracing_amd import capi, host, scenes
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 15
sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1024, 2048]
frames = 16
L = capi.lib()
have = hasattr(L, "jpt_set_bake_directional")
sc = scenes.demo_scene()
cells = [(inst, s) for inst in sc.instances for s in sc.meshes[inst.mesh].surfaces]
side = int(np.ceil(np.sqrt(len(cells))))


def preheat(ctx):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 100.0:
        for _ in range(4):
            ctx.render(frames, 1, asynchronous=True)
        ctx.sync()


def queued(ctx):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for k in range(8):
            ctx.render(frames, 1 + k * frames, asynchronous=True)
        ctx.sync()
        out.append((time.perf_counter() - t0) / 8 * 1e3)
    return out


def blocking(ctx):
    out = []
    for k in range(reps):
        ctx.render(frames, 1 + k * frames)
        out.append(ctx.stats()["last_render_ms"])
    return out


def timed(ctx, call):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


for w in sizes:
    h = w
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    ctx.bake_begin(w, h)
    for k, (inst, s) in enumerate(cells):
        uv2 = ((np.clip(s.uvs, 0.0, 1.0) * 0.9 + np.array([k % side, k // side])) / side).astype(np.float32)
        ctx.bake_add_surface(s, uv2, inst.transform)
    valid = (ctx.read_bake_texels()[1][..., :3] != 0).any(axis=-1)
    print("## %d x %d texels, %.1f %% valid, %d frames per render (%s)" % (w, h, 100.0 * valid.mean(), frames, os.environ.get("JPT_LIB", "this library")))
    if trace:
        ctx.set_bake_directional(True)
        for _ in range(4):
            ctx.render(frames, 1)
        preheat(ctx)
        for k in range(15):
            ctx.render(frames, 1 + k * frames, asynchronous=True)
        ctx.sync()
        ctx.close()
        continue
    rows = []
    for on in ((False, True) if have else (False,)):
        if have:
            ctx.set_bake_directional(on)
        for _ in range(4):
            ctx.render(frames, 1); ctx.bake_finish()
            if on:
                ctx.bake_finish_directional()
        ctx.sync()
        preheat(ctx)
        q = queued(ctx)
        preheat(ctx)
        b = blocking(ctx)
        preheat(ctx)
        f0 = timed(ctx, ctx.bake_finish)
        f1 = timed(ctx, ctx.bake_finish_directional) if on else None
        rows.append(("on" if on else "off", q, b, f0, f1))
    print("| switch | queued render | blocking render | jpt_bake_finish | jpt_bake_finish_directional |")
    print("|---|---|---|---|---|")
    for name, q, b, f0, f1 in rows:
        print("| %s | %s | %s | %s | %s |" % (name, stats(q), stats(b), stats(f0), stats(f1) if f1 else "-"))
    if len(rows) == 2:
        print("the switch costs a queued render %.3f ms, a blocking render %.3f ms (medians)" % (
            float(np.median(rows[1][1]) - np.median(rows[0][1])), float(np.median(rows[1][2]) - np.median(rows[0][2]))))
    ctx.close()
