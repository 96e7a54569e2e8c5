# What the history costs jpt_denoise, at 1920 x 1080 with the default five passes on the benchmark's C3 scene (4 bounces,
# JPT_ACCUM_REF_LDR8, 4 frames accumulated with jpt_set_variance on), through the C ABI in one process.  After ten untimed calls and
# 100 ms of queued calls (the clocks, as bench.py preheats), the median of `reps` runs (default 15), min .. max, of the device time of
# one jpt_denoise -- guide pass, stage and filter passes -- timed as a queue of 20 calls and a sync: unguided, variance-guided, and with
# the history on under a standing camera.  A history call consumes its frames, so every call of a queue is preceded by
# jpt_set_progressive_frame_count(frame_count + 1), a host-side assignment that re-positions the accumulation where it is.
# With JPT_LIB naming a library without the calls (the parent's) only the first two rows are timed: the yardstick of the same session.
#   python tools/denoise_temporal_rate.py [reps] [WxH]
# The kernels' own times: run the same under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
# tools/denoise_temporal_rate.py trace` -- three phases of 25 + 15 history calls each: a standing camera (every pixel carries history: no
# block stages), a jpt_denoise_history_reset before every call (every block with a hit stages) and a camera that pans to and fro by
# four pixels -- then
#   python tools/denoise_temporal_rate.py kernels DIR
# prints the median, min .. max of the last 15 launches of each phase of history_kernel and atrous_var_pre_kernel, and the bytes the
# stage has to move per pixel against the measured copy bandwidth.
import csv, glob, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

PHASES = ("standing", "reset before every call", "pan")
WARM, TIMED = 25, 15
COPY_TBS = 6.29                      # float4 copy, measured (MI355X)
BYTES_PER_PIXEL = 64 + 48 + 64       # sum, albedo, position, normal read; one previous texel's three planes; four planes written


def stats(v):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    per = {"history_kernel": [], "atrous_var_pre_kernel": []}
    rows = []
    for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for key in per:
            if key in r["Kernel_Name"]:
                per[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    w, h = [int(s) for s in sys.argv[3].split("x")] if len(sys.argv) > 3 else (1920, 1080)
    floor_ms = w * h * BYTES_PER_PIXEL / (COPY_TBS * 1e12) * 1e3
    print("| kernel | phase | launches | last %d launches: median (min .. max) |" % TIMED)
    print("|---|---|---|---|")
    for key, v in per.items():
        for k, phase in enumerate(PHASES):
            part = v[k * (WARM + TIMED):(k + 1) * (WARM + TIMED)]
            if len(part) == WARM + TIMED:
                print("| %s | %s | %d | %s |" % (key, phase, len(v), stats(part[-TIMED:])))
    print("history_kernel has to move %d B per pixel: %.3f ms at the %.2f TB/s of a float4 copy, %d x %d" % (BYTES_PER_PIXEL, floor_ms, COPY_TBS, w, h))
    sys.exit(0)

from gdpathtracing_amd import capi, host, scenes
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 15
w, h = [int(s) for s in sys.argv[2].split("x")] if len(sys.argv) > 2 and not trace else (1920, 1080)
queue, frames = 20, 4
L = capi.lib()
have = hasattr(L, "jpt_set_denoise_history")
sc = scenes.demo_scene(51200)       # bench.py's C3
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
cams = [scenes.camera_block(sc.camera, w, h)]
t = np.asarray(sc.camera.transform, np.float64)
pan = scenes.CameraDesc(scenes.transform12(scenes.rot_y(4 * sc.camera.fov_deg / h) @ t[:9].reshape(3, 3), t[9:]), sc.camera.fov_deg, sc.camera.near, sc.camera.far)
cams.append(scenes.camera_block(pan, w, h))
ctx.set_camera(cams[0])
ctx.set_variance(True)
ctx.render(frames, 1)
ctx.sync()
history = False


def call(k=0, reset=False, moving=False):
    if history:
        L.jpt_set_progressive_frame_count(ctx.h, frames + 1)   # (the accumulation stays what it is: the call's frames count as new ones)
        if reset:
            ctx.denoise_history_reset()
        if moving:
            ctx.set_camera(cams[k & 1])
    ctx.denoise()


def preheat():
    for _ in range(10):
        call()
    ctx.sync()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 100.0:
        for _ in range(queue):
            call()
        ctx.sync()


def queued():
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(queue):
            call()
        ctx.sync()
        out.append((time.perf_counter() - t0) / queue * 1e3)
    return out


print("## jpt_denoise, %d x %d, five passes, C3 (%s)" % (w, h, os.environ.get("JPT_LIB", "this library")))
if trace:
    assert have, "the library has no history"
    ctx.set_denoise_history(enable=1)
    history = True
    for phase in range(3):
        ctx.set_camera(cams[0])
        for k in range(WARM + TIMED):
            call(k, reset=phase == 1, moving=phase == 2)
        ctx.sync()
    ctx.close()
    sys.exit(0)
rows = []
for name in ("unguided", "variance-guided") + (("history", "history", "variance-guided", "unguided") if have else ("variance-guided", "unguided")):
    history = name == "history"
    if have:
        ctx.set_denoise_history(enable=int(history))
    ctx.set_denoise_variance(enable=int(name == "variance-guided"))
    preheat()
    rows.append((name, queued()))
print("| jpt_denoise | one call, device time |")
print("|---|---|")
for name, q in rows:
    print("| %s | %s |" % (name, stats(q)))
med = {name: float(np.median(sum((q for n, q in rows if n == name), []))) for name in set(n for n, _ in rows)}
if have:
    print("with history one jpt_denoise takes %.3f ms (medians of both runs): %.2f times the variance-guided call, %.2f times the unguided one"
          % (med["history"], med["history"] / med["variance-guided"], med["history"] / med["unguided"]))
ctx.close()
