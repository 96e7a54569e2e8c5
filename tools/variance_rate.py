# What jpt_set_variance and jpt_noise_estimate cost, at 1920 x 1080, 16 frames per render, 4 bounces, JPT_ACCUM_REF_LDR8, through the C
# ABI in one process, on two workloads: the benchmark's C3 scene through its camera (a pinhole: the switch also takes its sky cull
# away) and the demo scene's bake atlas (one grid cell per (instance, surface), rasterised on the device as tools/bake_rate.py does; a
# bake render has no cull to lose).  After four untimed rounds and 100 ms of the workload's own queued renders (the clocks, as bench.py
# preheats), the median of `reps` runs (default 15), min .. max, of
#   queued render   wall time per render of a queue of 8 renders and a sync, the switch off and on;
#   one check       wall time of jpt_noise_estimate + jpt_read_noise (32 bytes) behind a sync;
#   read_accum      wall time of jpt_read_accum_f32 of the same image behind a sync: the route the check replaces.
# With JPT_LIB naming a library without the calls (the parent's) only the switch-off row and read_accum are timed: that is the
# yardstick for "off costs nothing".  With JPT_SKY_CULL=0 in the environment the switch-off row is a render without its sky cull: the
# difference to the plain switch-off row is what the lost cull costs, the rest of the switch's cost is the moment kernel's.
#   python tools/variance_rate.py [reps] [WxH]
# The kernels' own times: run the same under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/variance_rate.py
# trace [camera|bake]` (15 queued renders with the switch on and 15 checks, each check behind a jpt_meter, behind the warm-up; one
# workload per trace keeps the two workloads' launches apart), then
#   python tools/variance_rate.py kernels DIR
# prints the median, min .. max of variance_moments, wf2_accumulate, noise_estimate_kernel, noise_resolve_kernel and jpt_meter's two
# kernels over those launches, per grid size.
import csv, glob, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

KERNELS = ("variance_moments", "wf2_accumulate", "noise_estimate_kernel", "noise_resolve_kernel", "meter_histogram_kernel", "meter_resolve_kernel")


def stats(v):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    per = {}
    for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if key:
                grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
                per.setdefault((key, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print("| kernel | grid (threads) | launches | last 15 launches: median (min .. max) |")
    print("|---|---|---|---|")
    for (key, grid), v in sorted(per.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        print("| %s | %s | %d | %s |" % (key, grid, len(v), stats(v[-15:])))
    sys.exit(0)

from gdpathtracing_amd import capi, host, scenes
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 15
w, h = [int(s) for s in sys.argv[2].split("x")] if len(sys.argv) > 2 and not trace else (1920, 1080)
frames = 16
L = capi.lib()
have = hasattr(L, "jpt_set_variance")
sc = scenes.demo_scene(51200)       # bench.py's C3
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


def timed(ctx, call):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def check(ctx):
    ctx.noise_estimate()
    ctx.read_noise(histogram=False)


for workload in ("C3 camera", "bake atlas"):
    if trace and len(sys.argv) > 2 and sys.argv[2] not in workload:      # (trace camera | trace bake: one workload per trace)
        continue
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    if workload == "bake atlas":
        ctx.bake_begin(w, h)
        for k, (inst, s) in enumerate(cells):
            uv2 = ((np.clip(s.uvs, 0.0, 1.0) * 0.9 + np.array([k % side, k // side])) / side).astype(np.float32)
            ctx.bake_add_surface(s, uv2, inst.transform)
    print("## %s, %d x %d, %d frames per render (%s%s)" % (workload, w, h, frames, os.environ.get("JPT_LIB", "this library"),
                                                          ", JPT_SKY_CULL=0" if os.environ.get("JPT_SKY_CULL") == "0" else ""))
    if trace:
        ctx.set_variance(True)
        for _ in range(4):
            ctx.render(frames, 1)
        preheat(ctx)
        for k in range(15):
            ctx.render(frames, 1 + k * frames, asynchronous=True)
        ctx.sync()
        for k in range(15):
            ctx.meter()
            check(ctx)
        ctx.close()
        continue
    rows = []
    for on in ((False, True) if have else (False,)):
        if have:
            ctx.set_variance(on)
        for _ in range(4):
            ctx.render(frames, 1)
        ctx.sync()
        preheat(ctx)
        q = queued(ctx)
        preheat(ctx)
        c = timed(ctx, lambda: check(ctx)) if on else None
        preheat(ctx)
        r = timed(ctx, ctx.read_accum)
        rows.append(("on" if on else "off", q, c, r))
    print("| switch | queued render | jpt_noise_estimate + jpt_read_noise | jpt_read_accum_f32 |")
    print("|---|---|---|---|")
    for name, q, c, r in rows:
        print("| %s | %s | %s | %s |" % (name, stats(q), stats(c) if c else "-", stats(r)))
    if len(rows) == 2:
        print("the switch costs a queued render %.3f ms (medians)" % float(np.median(rows[1][1]) - np.median(rows[0][1])))
    ctx.close()
