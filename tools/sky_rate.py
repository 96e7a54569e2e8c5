# What jpt_set_sky costs and what it replaces, through the C ABI in one process: maps of 2048 x 1024 and 4096 x 2048, samples 1, 4 and 8,
# Godot's default sky with no sun and with one (radius 0.05, the default 30 degree halo).  After 100 ms of queued jpt_set_sky calls at
# the largest shape (the clocks, as bench.py preheats), the median of `reps` runs (default 15), min .. max, of
#   kernel     the kernel's time by HIP events on the context's stream (torch.cuda.Event around 10 back-to-back calls at the map's own
#              size in BRDF mode, which only queue the kernel; divided by 10), texels/s and subsamples/s;
#   set_sky    the wall time of jpt_set_sky + jpt_sync in BRDF mode (the call itself returns once the kernel is queued: `call` is that
#              time alone) and with JPT_ENV_SAMPLING_MIS on (the tables are rebuilt and the call waits for their total);
#   old route  the wall time of jpt_set_environment of a same-size float32 array, in both modes, and of a vectorised numpy evaluation of
#              the same formula on the host (tests/np_sky.py, samples 1 only: it is the cheapest the host can do) -- together the
#              route the call replaces.
# With JPT_LIB naming a library without jpt_set_sky (the parent's) only jpt_set_environment is timed.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from gdpathtracing_amd import capi, host
import np_sky as ns
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
L = capi.lib()
have_sky = hasattr(L, "jpt_set_sky")
SIZES = ((2048, 1024), (4096, 2048))
SAMPLES = (1, 4, 8)
SUN = [dict(direction=(0.3, 0.8, 0.52), angular_radius=0.05, color=(1.0, 0.95, 0.9), energy=8.0)]
K = 10


def stats(v, unit="ms"):
    return "%.3f %s (%.3f .. %.3f)" % (float(np.median(v)), unit, min(v), max(v))


def wall(fn):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


ctx = host.Context(0)
lib = os.environ.get("JPT_LIB", "this library")
if have_sky:
    stream = torch.cuda.ExternalStream(ctx.get_stream())
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 100.0:
        for _ in range(4):
            ctx.set_sky(None, 4096, 2048, 8)
        ctx.sync()
    print("| map | samples | suns | kernel | Gtexels/s | Gsubsamples/s | jpt_set_sky call | + jpt_sync | with MIS on |")
    print("|---|---|---|---|---|---|---|---|---|")
    for w, h in SIZES:
        for n_suns in (0, 1):
            p = ns.lib_params(ns.params(suns=SUN[:n_suns]))
            for n in SAMPLES:
                ctx.set_environment_sampling(capi.ENV_SAMPLING_BRDF)
                ctx.set_sky(p, w, h, n)
                ctx.sync()
                kernel = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(K):
                        ctx.set_sky(p, w, h, n)
                    e1.record(stream)
                    e1.synchronize()
                    kernel.append(e0.elapsed_time(e1) / K)
                call, synced = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    ctx.set_sky(p, w, h, n)
                    t1 = time.perf_counter()
                    ctx.sync()
                    t2 = time.perf_counter()
                    call.append((t1 - t0) * 1e3); synced.append((t2 - t0) * 1e3)
                ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
                mis = wall(lambda: ctx.set_sky(p, w, h, n))
                k = float(np.median(kernel)) * 1e-3
                print("| %d x %d | %d | %d | %s | %.1f | %.1f | %s | %s | %s |" % (w, h, n, n_suns, stats([x * 1e3 for x in kernel], "us"), w * h / k / 1e9,
                                                                            w * h * n * n / k / 1e9, stats(call), stats(synced), stats(mis)))
print("| map | jpt_set_environment (%s) | with MIS on | numpy evaluation of the formula, samples 1 |" % lib)
print("|---|---|---|---|")
for w, h in SIZES:
    t0 = time.perf_counter()
    rgb = ns.sky_map(ns.params(suns=SUN), w, h, 1)
    host_eval = (time.perf_counter() - t0) * 1e3
    ctx.set_environment_sampling(capi.ENV_SAMPLING_BRDF)
    ctx.set_environment(rgb)
    brdf = wall(lambda: ctx.set_environment(rgb))
    ctx.set_environment_sampling(capi.ENV_SAMPLING_MIS)
    mis = wall(lambda: ctx.set_environment(rgb))
    print("| %d x %d | %s | %s | %.0f ms |" % (w, h, stats(brdf), stats(mis), host_eval))
ctx.close()
