# What jpt_set_camera_model costs: renders of the benchmark's C3 scene and camera (demo scene, 1920x1080, 8 frames per render, 4
# bounces) through the C ABI, in one process: with the pinhole; with PROJECTIVE and the same perspective matrix (the same directions
# from the near plane: the figure isolates the lost sky cull and the second unprojection); and with PROJECTIVE and an orthographic
# matrix that frames what the perspective one frames at the box's middle, 9.7694 units down the axis.  Blocking renders with kernel
# timing on (the render's time and its primary launch's share, last_primary_ms), then queued renders (ms per render with the pipeline
# full).  Preheated as bench.py preheats; the median and the spread of `runs` runs.  Per kernel: `rocprofv3 --kernel-trace --stats --
# python tools/camera_rate.py 20`, in a run of its own.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
w, h, spp = 1920, 1080, 8
sc = scenes.demo_scene()
perspective = scenes.camera_block(sc.camera, w, h)
size = 2.0 * 9.7694 * np.tan(np.deg2rad(sc.camera.fov_deg) / 2.0)   # the perspective frame's height where the camera's axis meets z = 0
orthogonal = scenes.camera_block_orthogonal(sc.camera, size, w, h)
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_REF_LDR8)
ctx.set_camera(perspective)
for _ in range(8):   # (the clocks)
    ctx.render(spp, 1)
print("| camera | blocking ms (median, min-max) | primary launch ms | queued ms per render (median, min-max) |")
print("|---|---|---|---|")
for name, model, cam in (("pinhole", capi.CAMERA_PINHOLE, perspective), ("PROJECTIVE, perspective matrix", capi.CAMERA_PROJECTIVE, perspective),
                         ("PROJECTIVE, orthographic matrix", capi.CAMERA_PROJECTIVE, orthogonal)):
    ctx.set_camera_model(model)
    ctx.set_camera(cam)
    ctx.set_kernel_timing(True)
    blocking, primary = [], []
    for k in range(3 + 2 * runs):
        ctx.accum_reset(); ctx.render(spp, 1 + k * spp)
        if k >= 3:
            st = ctx.stats(); blocking.append(st["last_render_ms"]); primary.append(st["last_primary_ms"])
    ctx.set_kernel_timing(False)
    queued = []
    for _ in range(runs):
        for k in range(8):
            ctx.render(spp, 1 + k * spp, asynchronous=True)
        ctx.sync()
        t0 = time.perf_counter()
        for k in range(steps):
            ctx.render(spp, 1 + k * spp, asynchronous=True)
        ctx.sync()
        queued.append((time.perf_counter() - t0) / steps * 1e3)
    print("| %s | %.3f (%.3f-%.3f) | %.3f | %.3f (%.3f-%.3f) |" % (name, np.median(blocking), min(blocking), max(blocking), np.median(primary),
                                                                 np.median(queued), min(queued), max(queued)))
ctx.close()
