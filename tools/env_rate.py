# What an environment map costs (jpt_set_environment): C3 (demo scene, 1920x1080, 8 spp, 4 bounces) queued and blocking, and the
# close-up camera queued (bench.py's value_closeup), each with main.glsl's gradient, a 2048x1024 map and a 4096x2048 map (128 MiB
# of float4 texels: past the L2, gathered by incoherent bounce rays, four 16-byte loads per miss).  Ray segments per second
# (the library's own ray count of a blocking render / ms per render), and ms per render.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
w, h, spp, bounces = 1920, 1080, 8, 4
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40

def sky(hh, ww):
    v, u = np.mgrid[0:hh, 0:ww].astype(np.float32)
    rgb = np.stack([0.4 + 0.6 * u / ww, 0.3 + 1.2 * (1.0 - v / hh), 0.6 + 0.3 * np.sin(20.0 * u / ww)], axis=-1)
    rgb[hh // 6:hh // 6 + hh // 100 + 1, ww // 3:ww // 3 + ww // 200 + 1] = 40.0
    return rgb.astype(np.float32)

maps = [("gradient", None), ("2048x1024", sky(1024, 2048)), ("4096x2048", sky(2048, 4096))]
closeup = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 4.2)), fov_deg=75.0)
print("| camera | sky | blocking ms | queued ms | queued Mrays/s |")
print("|---|---|---|---|---|")
for cam_name in ("demo", "closeup"):
    sc = scenes.demo_scene()
    if cam_name == "closeup":
        sc.camera = closeup
    for name, rgb in maps:
        ctx = host.Context(0)
        ctx.build_scene(sc, capi.BUILD_SAH)
        ctx.set_params(w, h, bounces, capi.ACCUM_REF_LDR8)
        ctx.set_camera(scenes.camera_block(sc.camera, w, h))
        if rgb is not None:
            ctx.set_environment(rgb)
            ctx.set_environment_params(None, 1.0)
        for _ in range(3):
            ctx.render(spp, 1)
        blocking = []
        for _ in range(5):
            ctx.accum_reset()
            ctx.render(spp, 1)
            blocking.append(ctx.stats()["last_render_ms"])
        rays = ctx.stats()["rays"]
        for _ in range(10):
            ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
        ctx.sync()
        queued = (time.perf_counter() - t0) / steps * 1e3
        ctx.close()
        print("| %s | %s | %.3f | %.3f | %.0f |" % (cam_name, name, float(np.median(blocking)), queued, rays / queued / 1e3))
