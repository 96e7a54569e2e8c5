# What jpt_denoise costs: the device time of one call (guide pass + filter passes) at 1920x1080 and 3840x2160 on the C3 scene (demo
# scene, 4 bounces), beside one blocking 8-spp render and one blocking 1-spp frame of the same context, measured in one process with
# the clocks raised first (tools/clock_ramp.py: a lone 100 us launch on an idle device measures the clock ramp, so the calls are
# timed as a queue of `steps` behind a warm-up).  Per kernel: run this under `rocprofv3 --kernel-trace --stats -- python
# tools/denoise_rate.py 20`, in a run of its own, and read guide_kernel / atrous_kernel from the kernel statistics.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
sizes = [(1920, 1080), (3840, 2160)] if len(sys.argv) <= 2 else [tuple(int(v) for v in sys.argv[2].split("x"))]
sc = scenes.demo_scene()
print("| size | passes | jpt_denoise us | per pixel ns | blocking 8-spp render ms | blocking 1-spp frame ms |")
print("|---|---|---|---|---|---|")
for w, h in sizes:
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    for _ in range(4):
        ctx.render(8, 1)
    ms8, ms1 = [], []
    for _ in range(5):
        ctx.accum_reset(); ctx.render(8, 1); ms8.append(ctx.stats()["last_render_ms"])
        ctx.accum_reset(); ctx.render(1, 1); ms1.append(ctx.stats()["last_render_ms"])
    for passes in (5, 1):
        ctx.set_denoise_params(passes=passes)
        for _ in range(10):
            ctx.denoise()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.denoise()
        ctx.sync()
        us = (time.perf_counter() - t0) / steps * 1e6
        print("| %dx%d | %d | %.1f | %.3f | %.3f | %.3f |" % (w, h, passes, us, us * 1e3 / (w * h), float(np.median(ms8)), float(np.median(ms1))))
    ctx.close()
