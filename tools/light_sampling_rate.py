# What importance sampling of the emissive triangles costs and what it saves (jpt_set_light_sampling): C3 (demo scene, 1920x1080,
# 8 spp, 4 bounces; its light quad and its 51 200-triangle emissive blob) under the default sky, per sampling mode: ms per render
# blocking and queued (REF_LDR8, as bench.py), and the RMSE of the HDR mean image against a long light-sampling run when both modes
# get the same time (as many 8-spp renders as fit in `budget` BRDF renders' time).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
w, h, spp, bounces = 1920, 1080, 8, 4
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
budget = int(sys.argv[2]) if len(sys.argv) > 2 else 16      # equal-time budget, in BRDF renders
ref_renders = int(sys.argv[3]) if len(sys.argv) > 3 else 256  # the long light-sampling run: renders of spp frames


def context(sc, accum, mode):
    ctx = host.Context(0)
    ctx.build_scene(sc, capi.BUILD_SAH)
    ctx.set_params(w, h, bounces, accum)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    ctx.set_light_sampling(mode)
    return ctx


def mean_image(ctx, renders, first=1):
    ctx.accum_reset()
    for k in range(renders):
        ctx.render(spp, first + k * spp, asynchronous=True)
    return ctx.read_accum()[..., :3].astype(np.float64) / (renders * spp)


print("| sampling | blocking ms | queued ms | renders in equal time | RMSE vs long light-sampling run | mean (long run) |")
print("|---|---|---|---|---|---|")
sc = scenes.demo_scene()
ref_ctx = context(sc, capi.ACCUM_HDR_F32, capi.LIGHT_SAMPLING_MIS)
ref = mean_image(ref_ctx, ref_renders, first=1_000_001)
ref_ctx.close()
rows, queued = [], {}
for name, mode in (("BRDF", capi.LIGHT_SAMPLING_BRDF), ("MIS", capi.LIGHT_SAMPLING_MIS)):
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
    print("| %s | %.3f | %.3f | %d | %.4f | %.4f (%.4f) |" % (name, blocking, queued[name], n, rmse, float(np.nanmean(img)),
                                                          float(np.nanmean(ref))))
