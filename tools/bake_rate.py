# What a lightmap bake costs beside a picture: the demo scene at 1024 x 1024, 8 frames per render, 4 bounces, through the C ABI in one
# process -- a pinhole render from the scene's camera, and a bake render of an atlas that gives every (instance, surface) of the scene
# one cell of a square grid, rasterised on the device (jpt_bake_begin + jpt_bake_add_surface, timed on the host).  Blocking renders
# with kernel timing on: the render's time and its primary launch's share (last_primary_ms: the two 16-byte texel loads per refill
# are in there); then queued renders, ms per render with the pipeline full.  The two renders trace other paths (a bake has no sky
# cull and every valid texel's first ray starts on a surface), so this is the price of a bake, not a comparison of kernels.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
w = h = 1024
spp = 8
sc = scenes.demo_scene()
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
for _ in range(8):   # (the clocks)
    ctx.render(spp, 1)
cells = [(inst, s) for inst in sc.instances for s in sc.meshes[inst.mesh].surfaces]
side = int(np.ceil(np.sqrt(len(cells))))


def rasterise():
    ctx.bake_begin(w, h)
    for k, (inst, s) in enumerate(cells):
        uv2 = ((np.clip(s.uvs, 0.0, 1.0) * 0.9 + np.array([k % side, k // side])) / side).astype(np.float32)
        ctx.bake_add_surface(s, uv2, inst.transform)


rasterise()
t0 = time.perf_counter()
rasterise()
raster_ms = (time.perf_counter() - t0) * 1e3
valid = (ctx.read_bake_texels()[1][..., :3] != 0).any(axis=-1)
images = ctx.read_bake_texels()
print("atlas: %d surfaces, %d triangles, %.1f %% of %d x %d texels valid, rasterised in %.2f ms (host time, %d calls)" % (
    len(cells), sum(len(s.indices) // 3 for _, s in cells), 100.0 * valid.mean(), w, h, raster_ms, len(cells) + 1))
print("| render | blocking ms (median, min-max) | primary launch ms (median, min-max) | queued ms per render (median, min-max) |")
print("|---|---|---|---|")
for name, bake in (("pinhole", False), ("bake", True)):
    ctx.set_bake_texels(*(images if bake else (None, None)))
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
    print("| %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) |" % (name, np.median(blocking), min(blocking), max(blocking), np.median(primary),
                                                                            min(primary), max(primary), np.median(queued), min(queued), max(queued)))
ctx.close()
