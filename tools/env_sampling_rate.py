# What importance sampling of the map costs and what it saves (jpt_set_environment_sampling): C3 (demo scene, 1920x1080, 8 spp,
# 4 bounces) and the close-up camera (bench.py's value_closeup) under a 2048x1024 map with a small sun, per sampling mode: ms per
# render blocking and queued (REF_LDR8, as bench.py), and the RMSE of the HDR mean image against a long MIS run when both modes get
# the same time (as many 8-spp renders as fit in `budget` BRDF renders' time).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
w, h, spp, bounces = 1920, 1080, 8, 4
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
budget = int(sys.argv[2]) if len(sys.argv) > 2 else 16      # equal-time budget, in BRDF renders
ref_renders = int(sys.argv[3]) if len(sys.argv) > 3 else 256  # the long MIS run: renders of spp frames


def sun_sky(hh, ww):
    v, u = np.mgrid[0:hh, 0:ww].astype(np.float32)
    rgb = np.stack([0.10 + 0.05 * u / ww, 0.12 + 0.10 * (1.0 - v / hh), 0.20 + 0.05 * np.sin(20.0 * u / ww)], axis=-1)
    rgb[hh // 3:hh // 3 + 6, ww // 3:ww // 3 + 6] = 2000.0     # a sun of 6 x 6 texels, 30 degrees above the horizon
    return rgb.astype(np.float32)


a = np.radians(-120.0)   # world -> map: the sun stands over the camera's shoulder and shines into the open side of the box
ROT = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], np.float32)
rgb = sun_sky(1024, 2048)
closeup = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 4.2)), fov_deg=75.0)


def context(sc, accum, mode):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, bounces, accum)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    ctx.set_environment(rgb)
    ctx.set_environment_params(ROT, 1.0)
    ctx.set_environment_sampling(mode)
    return ctx


def mean_image(ctx, renders, first=1):
    ctx.accum_reset()
    for k in range(renders):
        ctx.render(spp, first + k * spp, asynchronous=True)
    return ctx.read_accum()[..., :3].astype(np.float64) / (renders * spp)


print("| camera | sampling | blocking ms | queued ms | renders in equal time | RMSE vs long MIS run | mean (long run) |")
print("|---|---|---|---|---|---|---|")
for cam_name in ("C3", "closeup"):
    sc = scenes.demo_scene()
    if cam_name == "closeup":
        sc.camera = closeup
    ref_ctx = context(sc, capi.ACCUM_HDR_F32, capi.ENV_SAMPLING_MIS)
    ref = mean_image(ref_ctx, ref_renders, first=1_000_001)
    ref_ctx.close()
    rows, queued = [], {}
    for name, mode in (("BRDF", capi.ENV_SAMPLING_BRDF), ("MIS", capi.ENV_SAMPLING_MIS)):
        ctx = context(sc, capi.ACCUM_REF_LDR8, mode)
        for _ in range(3):
            ctx.render(spp, 1)
        blocking = []
        for _ in range(5):
            ctx.accum_reset()
            ctx.render(spp, 1)
            blocking.append(ctx.stats()["last_render_ms"])
        for _ in range(10):
            ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
        ctx.sync()
        queued[name] = (time.perf_counter() - t0) / steps * 1e3
        ctx.close()
        rows.append((name, mode, float(np.median(blocking))))
    for name, mode, blocking in rows:
        n = max(1, int(budget * queued["BRDF"] / queued[name]))
        ctx = context(sc, capi.ACCUM_HDR_F32, mode)
        img = mean_image(ctx, n)
        ctx.close()
        rmse = float(np.sqrt(np.nanmean((img - ref) ** 2)))
        print("| %s | %s | %.3f | %.3f | %d | %.4f | %.4f (%.4f) |" % (cam_name, name, blocking, queued[name], n, rmse, float(np.nanmean(img)),
                                                                  float(np.nanmean(ref))))
