# What a ray query costs beside the guide pass that does the same walk: jpt_query_rays_device on the 1920x1080 pixel-centre rays of
# the C3 scene (demo scene; 2 073 600 rays, the guide pass's own) and on 2 000 000 random rays (the incoherent case), closest and any,
# beside jpt_denoise with one filter pass (guide_kernel + one atrous_kernel), in one process with the clocks raised first
# (tools/clock_ramp.py); every call is timed as a queue of `steps` behind a warm-up.
#   python tools/query_rate.py [steps]
# Per kernel (guide_kernel against query_kernel, without the filter pass and the launch gaps): run it under
#   rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/query_rate.py 50
# in a run of its own, then
#   python tools/query_rate.py --trace DIR
# which prints count / median / mean duration per kernel name and grid size (the two ray sets differ in size, so in grid).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

if len(sys.argv) > 2 and sys.argv[1] == "--trace":
    import csv, glob
    from collections import defaultdict
    by = defaultdict(list)
    for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if "guide_kernel" in name or "query_" in name or "atrous" in name:
                by[(name[-70:], r.get("Grid_Size_X", r.get("Grid_Size", "?")))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (name, grid), v in sorted(by.items()):
        v = sorted(v)[len(v) // 5:]          # (the first fifth: warm-up)
        print("%-70s grid %9s  n %4d  median %8.1f us  mean %8.1f us" % (name, grid, len(v), v[len(v) // 2] / 1e3, sum(v) / len(v) / 1e3))
    sys.exit(0)

import torch
from gdpathtracing_amd import capi, host, scenes, wire
F = np.float32
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
W, H = 1920, 1080
sc = scenes.demo_scene()
cam = scenes.camera_block(sc.camera, W, H)


def centre_rays():   # raster_direction(cam, W, H, x + 0.5, y + 0.5) from the camera position, float32 as the kernels
    ys, xs = np.mgrid[0:H, 0:W]
    nx = (xs.reshape(-1).astype(F) + F(0.5)) / F(W) * F(2.0) - F(1.0)
    ny = -((ys.reshape(-1).astype(F) + F(0.5)) / F(H) * F(2.0) - F(1.0))
    m = cam["ivp"].astype(F).reshape(-1)
    ww = m[3] * nx + m[7] * ny + m[11] + m[15]
    world = np.stack([(m[k] * nx + m[4 + k] * ny + m[8 + k] + m[12 + k]) / ww for k in range(3)], axis=-1)
    pos = np.asarray(cam["position"], F).reshape(-1)[:3]
    d = world - pos[None, :]
    d = d * (F(1.0) / np.sqrt((d * d).sum(axis=1, dtype=F)))[:, None]
    return np.broadcast_to(pos, d.shape), d.astype(F)


def random_rays(n):
    rng = np.random.default_rng(1)
    d = rng.normal(size=(n, 3))
    return rng.uniform(-3.0, 3.0, (n, 3)).astype(F), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(W, H, 4, capi.ACCUM_REF_LDR8)
ctx.set_camera(cam)
for _ in range(4):
    ctx.render(8, 1)       # raises the clocks; jpt_denoise needs an accumulation
ctx.set_denoise_params(passes=1)


def timed(call):
    for _ in range(10):
        call()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    ctx.sync()
    return (time.perf_counter() - t0) / steps * 1e6


print("| what | rays | us per call | Mrays/s |")
print("|---|---|---|---|")
us = timed(ctx.denoise)
print("| jpt_denoise, 1 pass (guide_kernel + one atrous_kernel) | %d | %.1f | %.0f |" % (W * H, us, W * H / us))
for what, (o, d) in (("pixel-centre rays", centre_rays()), ("random rays", random_rays(2_000_000))):
    n = len(d)
    rays = torch.from_numpy(host.make_rays(o, d).view(np.uint8)).cuda()
    hits = torch.zeros(n * wire.RAY_HIT.itemsize, dtype=torch.uint8, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us = timed(lambda: ctx.query_rays_device(rays, hits=hits))
    print("| jpt_query_rays_device closest, %s | %d | %.1f | %.0f |" % (what, n, us, n / us))
    us = timed(lambda: ctx.query_rays_device(rays, occluded=occ, mode=capi.QUERY_ANY))
    print("| jpt_query_rays_device any, %s | %d | %.1f | %.0f |" % (what, n, us, n / us))
    hit = (hits.cpu().numpy().view(wire.RAY_HIT)["flags"] & capi.HIT_VALID) != 0
    print("|   (%.1f %% of them hit) | | | |" % (100.0 * hit.mean()))
ctx.close()
