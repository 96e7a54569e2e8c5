# What reflection probes cost: the demo scene, 64 probes with faces of 128 x 128 on a 4 x 4 x 4 lattice through the scene's box (8 to a
# row: a 6144 x 1024 image), 4 bounces, 7 levels of 64 samples, through the C ABI in one process.  After the clocks are raised (four
# untimed rounds, as bench.py warms up), the median of `reps` runs (default 15) of
#   chain, prefilter   the kernel time of jpt_reflection_prefilter's two steps under jpt_set_kernel_timing (jpt_get_reflection_timing),
#                      and the gathers per second of the second: every kept sample of every texel of levels 1 .. 6 of every probe;
#   capture            the wall time of one 16-frame cube render plus jpt_reflection_prefilter and the read-back of the last level,
#                      blocking (a host clock around calls that end in a read-back).
# With the argument `prefilter` it only runs jpt_reflection_prefilter `reps` times after one render, for a kernel trace or a counter
# run taken in a run of its own.
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
mode = sys.argv[1] if len(sys.argv) > 1 else "wall"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
S, per_row, frames, n_levels, K = 128, 8, 16, 7, 64
sc = scenes.demo_scene()
lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
for inst in sc.instances:
    t = np.asarray(inst.transform, np.float32).reshape(4, 3)
    for s in sc.meshes[inst.mesh].surfaces:
        v = np.asarray(s.vertices) @ t[:3] + t[3]
        lo, hi = np.minimum(lo, v.min(axis=0)), np.maximum(hi, v.max(axis=0))
g = (np.arange(4) + 0.5) / 4.0
pos = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo).astype(np.float32)
n = len(pos)
w, h = host.reflection_image_size(n, S, per_row)
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
ctx.set_reflection_probes(pos, S, per_row)
ctx.set_reflection_params(n_levels=n_levels, samples=K)
for _ in range(4):   # (the clocks, the code objects)
    ctx.accum_reset(); ctx.render(frames, 1); ctx.reflection_prefilter(); ctx.read_reflection(n_levels - 1)
if mode == "prefilter":
    for _ in range(reps):
        ctx.reflection_prefilter()
    ctx.sync()
    ctx.close()
    sys.exit(0)
gathers = n * sum(6 * (S >> l) ** 2 * len(host.debug_reflection_samples(S, n_levels, K, l)[1]) for l in range(1, n_levels))
wall, chain, pre = [], [], []
ctx.set_kernel_timing(True)
for k in range(reps):
    ctx.accum_reset()
    t0 = time.perf_counter()
    ctx.render(frames, 1 + k * frames)
    ctx.reflection_prefilter()
    top = ctx.read_reflection(n_levels - 1)
    wall.append((time.perf_counter() - t0) * 1e3)
    a, b = ctx.reflection_timing()
    chain.append(a); pre.append(b)
ctx.set_kernel_timing(False)
print("%d probes of %d x %d faces, image %d x %d, %d levels of %d samples: source chain %.3f ms (median of %d, %.3f-%.3f), prefilter %.3f ms (%.3f-%.3f): "
      "%.3g gathers, %.3g gathers/s" % (n, S, S, w, h, n_levels, K, np.median(chain), reps, min(chain), max(chain), np.median(pre), min(pre), max(pre),
                                        gathers, gathers / (np.median(pre) * 1e-3)))
print("capture: %d frames plus the prefilter and the read-back of level %d (%d B): %.2f ms wall (median of %d, %.2f-%.2f)" % (
    frames, n_levels - 1, top.nbytes, np.median(wall), reps, min(wall), max(wall)))
ctx.close()
