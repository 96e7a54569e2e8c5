# What jpt_display costs: the device time of one call at 1920x1080 and 3840x2160 on the C3 scene (demo scene, 4 bounces, HDR
# accumulation) without bloom (one launch) and with five levels (ten launches), with the costliest tone map and transfer (REINHARD,
# sRGB), beside one jpt_denoise with its default parameters in the same process -- the yardstick: five a-trous passes move several
# times the bytes.  Measured as denoise_rate.py measures: the clocks raised by renders first, the calls timed as a queue of `steps`
# behind a warm-up.  Per kernel: run this under `rocprofv3 --kernel-trace --stats -- python tools/display_rate.py 40`, in a run of its
# own, and read the display_* kernels from the kernel trace (the sizes differ by their grids).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
sizes = [(1920, 1080), (3840, 2160)] if len(sys.argv) <= 2 else [tuple(int(v) for v in sys.argv[2].split("x"))]
sc = scenes.demo_scene()
def queue_us(call, sync):
    for _ in range(10):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    sync()
    return (time.perf_counter() - t0) / steps * 1e6
print("| size | call | us | per pixel ns | blocking 1-spp frame ms |")
print("|---|---|---|---|---|")
for w, h in sizes:
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    for _ in range(4):
        ctx.render(8, 1)
    ms1 = []
    for _ in range(5):
        ctx.accum_reset(); ctx.render(1, 1); ms1.append(ctx.stats()["last_render_ms"])
    rows = [("jpt_denoise, defaults", queue_us(ctx.denoise, ctx.sync))]
    ctx.set_display_params()
    rows.append(("jpt_display, defaults", queue_us(ctx.display, ctx.sync)))
    for levels in (0, 5):
        ctx.set_display_params(bloom_levels=levels, exposure=2.0, tonemap=capi.TONEMAP_REINHARD, transfer=capi.TRANSFER_SRGB)
        rows.append(("jpt_display, REINHARD + sRGB, %d levels" % levels, queue_us(ctx.display, ctx.sync)))
    for what, us in rows:
        print("| %dx%d | %s | %.1f | %.3f | %.3f |" % (w, h, what, us, us * 1e3 / (w * h), float(np.median(ms1))))
    ctx.close()
