# What capturing light probes costs: the demo scene, 4 096 probes of 16 x 8 cells on a 16 x 16 x 16 lattice through the scene's box
# (64 to a row: a 1024 x 512 image), 4 bounces, through the C ABI in one process.
#   probes    one 16-frame probe render plus jpt_probe_project and the read-back of 144 B per probe, blocking: wall time per capture
#             (a host clock around calls that end in a read-back), and the render's own time from kernel timing;
#   one by one   the route it replaces: a 16 x 8 JPT_CAMERA_EQUIRECT render of 16 frames per probe with the accumulation read back
#             (the projection on the CPU not counted), for the first `per_probe` probes, scaled to 4 096.
# With the argument `project` it only runs jpt_probe_project `reps` times after one render, for a kernel trace taken in a run of its own;
# with `onebyone` only the second route, which needs no call newer than jpt_set_camera_model (a library of an earlier commit: JPT_LIB).
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
mode = sys.argv[1] if len(sys.argv) > 1 else "wall"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
per_probe = int(sys.argv[3]) if len(sys.argv) > 3 else 8
tw, th, per_row, frames = 16, 8, 64, 16
sc = scenes.demo_scene()
lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
for inst in sc.instances:
    t = np.asarray(inst.transform, np.float32).reshape(4, 3)
    for s in sc.meshes[inst.mesh].surfaces:
        v = np.asarray(s.vertices) @ t[:3] + t[3]
        lo, hi = np.minimum(lo, v.min(axis=0)), np.maximum(hi, v.max(axis=0))
g = (np.arange(16) + 0.5) / 16.0
pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo
pos = pos.astype(np.float32)
n = len(pos)
w, h = host.probe_image_size(n, tw, th, per_row)
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
if mode != "onebyone":
    ctx.set_probes(pos, tw, th, per_row)
for _ in range(4 if mode != "onebyone" else 0):   # (the clocks, the code objects)
    ctx.accum_reset(); ctx.render(frames, 1); ctx.probe_project(); ctx.read_probe_sh()
if mode == "project":
    for _ in range(reps):
        ctx.probe_project()
    ctx.sync()
    ctx.close()
    sys.exit(0)
wall, render = [], []
ctx.set_kernel_timing(mode != "onebyone")
for k in range(reps if mode != "onebyone" else 0):
    ctx.accum_reset()
    t0 = time.perf_counter()
    ctx.render(frames, 1 + k * frames)
    ctx.probe_project(capi.PROBE_IRRADIANCE)
    sh = ctx.read_probe_sh()
    wall.append((time.perf_counter() - t0) * 1e3)
    render.append(ctx.stats()["last_render_ms"])
ctx.set_kernel_timing(False)
if mode != "onebyone":
  print("%d probes of %d x %d, image %d x %d, %d frames: capture %.2f ms wall (median of %d, %.2f-%.2f), of which the render %.2f ms (%.2f-%.2f); %d B read back" % (
      n, tw, th, w, h, frames, np.median(wall), reps, min(wall), max(wall), np.median(render), min(render), max(render), sh.nbytes))
  ctx.set_probes(None)
ctx.set_params(tw, th, 4, capi.ACCUM_HDR_F32)
ctx.set_camera_model(capi.CAMERA_EQUIRECT)
cams = [scenes.camera_block(scenes.CameraDesc(scenes.transform12(None, tuple(float(x) for x in p)), fov_deg=70.0), tw, th) for p in pos[:per_probe]]
for cam in cams:   # (warm)
    ctx.set_camera(cam); ctx.accum_reset(); ctx.render(frames, 1); ctx.read_accum()
one = []
for k in range(reps):
    t0 = time.perf_counter()
    for cam in cams:
        ctx.set_camera(cam); ctx.accum_reset(); ctx.render(frames, 1); ctx.read_accum()
    one.append((time.perf_counter() - t0) * 1e3 / per_probe)
print("one by one: %.3f ms per probe (median of %d runs of %d probes, %.3f-%.3f): %.0f ms for %d probes" % (
    np.median(one), reps, per_probe, min(one), max(one), np.median(one) * n, n) + (
    ", %.0f times the capture" % (np.median(one) * n / np.median(wall)) if wall else ""))
ctx.close()
