# What the variance guidance costs jpt_denoise, at 1920 x 1080 with the default five passes on the benchmark's C3 scene (4 bounces,
# JPT_ACCUM_REF_LDR8, 4 frames accumulated with jpt_set_variance on), through the C ABI in one process.  After ten untimed calls and
# 100 ms of queued calls (the clocks, as bench.py preheats), the median of `reps` runs (default 15), min .. max, of the device time of
# one jpt_denoise -- guide pass and filter passes -- timed as a queue of 20 calls and a sync, the guidance off and on, in that order and
# then once more the other way round (the second pair shows what the order does).
# With JPT_LIB naming a library without the calls (the parent's) only the guidance-off row is timed: that is the yardstick for "off
# costs nothing".
#   python tools/denoise_var_rate.py [reps] [WxH]
# The kernels' own times: run the same under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
# tools/denoise_var_rate.py trace` (15 calls with the guidance off, then 15 with it on, behind the warm-up), then
#   python tools/denoise_var_rate.py kernels DIR
# prints the median, min .. max of guide_kernel, atrous_kernel and atrous_var_kernel over those launches, per instantiation.
import csv, glob, os, re, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

KERNELS = ("guide_kernel", "atrous_var_kernel", "atrous_kernel")


def stats(v):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    per = {}
    for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if key:
                inst = re.search(r"<[^>]*>", r["Kernel_Name"])
                per.setdefault(key + (inst.group(0) if inst else ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print("| kernel | launches | last 15 launches: median (min .. max) |")
    print("|---|---|---|")
    for key, v in sorted(per.items()):
        print("| %s | %d | %s |" % (key, len(v), stats(v[-15:])))
    sys.exit(0)

from gdpathtracing_amd import capi, host, scenes
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 15
w, h = [int(s) for s in sys.argv[2].split("x")] if len(sys.argv) > 2 and not trace else (1920, 1080)
queue = 20
have = hasattr(capi.lib(), "jpt_set_denoise_variance")
sc = scenes.demo_scene(51200)       # bench.py's C3
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
ctx.set_variance(True)
ctx.render(4, 1)
ctx.sync()


def preheat():
    for _ in range(10):
        ctx.denoise()
    ctx.sync()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 100.0:
        for _ in range(queue):
            ctx.denoise()
        ctx.sync()


def queued():
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(queue):
            ctx.denoise()
        ctx.sync()
        out.append((time.perf_counter() - t0) / queue * 1e3)
    return out


print("## jpt_denoise, %d x %d, five passes, C3 (%s)" % (w, h, os.environ.get("JPT_LIB", "this library")))
if trace:
    for on in ((False, True) if have else (False,)):
        if have:
            ctx.set_denoise_variance(enable=int(on))
        preheat()
        for _ in range(15):
            ctx.denoise()
        ctx.sync()
    ctx.close()
    sys.exit(0)
rows = []
for on in ((False, True, True, False) if have else (False, False)):
    if have:
        ctx.set_denoise_variance(enable=int(on))
    preheat()
    rows.append(("on" if on else "off", queued()))
print("| guidance | one jpt_denoise, device time |")
print("|---|---|")
for name, q in rows:
    print("| %s | %s |" % (name, stats(q)))
if have:
    off, on = float(np.median(rows[0][1] + rows[3][1])), float(np.median(rows[1][1] + rows[2][1]))
    print("the guidance costs one jpt_denoise %.3f ms (medians of both runs): %.2f times the unguided call" % (on - off, on / off))
ctx.close()
