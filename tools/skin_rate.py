# An animation loop on the demo scene (51 200-triangle blob, two instances) with a synthetic rig (tests/np_skin.py ring_rig: 64 bones along
# the torus, four influences per vertex, two blend shapes): every step poses the blob and renders once (1920x1080x1, 30 steps).  Routes:
#   pose      jpt_scene_pose_mesh: palette and weights to the device, the skin kernel, the refit
#   update    jpt_scene_update_mesh with vertices computed OUTSIDE the timed loop: the floor of the host route
#   cpuskin   jpt_scene_update_mesh with the CPU skin (np_skin) inside the loop
# Two figures per route, the median of `reps` repetitions with min .. max:
#   queued    ms per step of the loop "call, render" with nothing synchronised: the rate an application sees.  The device bounds it (one
#             pipeline drain and one render per step), and the host's time in the call then includes the wait for a free staging slot.
#   idle      host ms in the call alone, the device idle before it (a sync before each call, outside the timing): the host's own cost.
# `update` and `cpuskin` need no new call: run them on an older library with JPT_LIB=... and routes = update,cpuskin.
# bone_shift > 0 moves the rig's bone indices up by that much (the palette grows by as many unused bones): 256 puts the same rig on the
# kernel's global-memory palette path.  The kernel's own time: run the pose route under `rocprofv3 --kernel-trace --stats`.
# usage: skin_rate.py [reps] [routes] [bone_shift]
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import np_skin
from gdpathtracing_amd import capi, host, scenes
w, h, spp, steps, BLOB, N_BONES = 1920, 1080, 1, 30, 2, 64
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
routes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["pose", "update", "cpuskin"]
shift = int(sys.argv[3]) if len(sys.argv) > 3 else 0

sc = scenes.demo_scene()
surf = sc.meshes[BLOB].surfaces[0]
rig = np_skin.ring_rig(surf, N_BONES, wide_weights=False)
rig.bones = (rig.bones + shift).astype(np.int32)
poses = [(np_skin.random_palette(np.random.RandomState(k), N_BONES + shift, 0.1), np.float32([0.5 + 0.5 * np.sin(0.3 * k), 0.3 * np.cos(0.2 * k)]))
         for k in range(steps)]

def loop(mode, idle):
    ctx = host.Context(0); ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT); ctx.set_params(w, h, 4, 0)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    if mode == "pose": ctx.set_mesh_rig(BLOB, sc.meshes[BLOB], [host.SurfaceRig(rig.bones, rig.weights, rig.position_deltas, rig.normal_deltas)], 4, 2)
    frames = [np_skin.skin_mesh(sc.meshes[BLOB], [rig], 4, *p) for p in poses] if mode == "update" else None
    for k in range(3): ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
    ctx.sync()
    t_call = 0.0
    t0 = time.perf_counter()
    for k in range(steps):
        if idle: ctx.sync()
        ta = time.perf_counter()
        if mode == "pose": ctx.pose_mesh(BLOB, *poses[k])
        elif mode == "update": ctx.update_mesh(BLOB, frames[k])
        else: ctx.update_mesh(BLOB, np_skin.skin_mesh(sc.meshes[BLOB], [rig], 4, *poses[k]))
        t_call += time.perf_counter() - ta
        ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
    ctx.sync()
    dt = time.perf_counter() - t0
    ctx.close()
    return dt / steps * 1e3, t_call / steps * 1e3

def stat(v):
    return "%.3f (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())

print("%d vertices, %d bones + %d unused, 2 shapes, %dx%dx%d, %d steps, %d repetitions; library %s" %
      (len(surf.vertices), N_BONES, shift, w, h, spp, steps, reps, os.environ.get("JPT_LIB", "(the tree's)")))
for mode in routes:
    queued = np.array([loop(mode, False) for _ in range(reps)])
    idle = np.array([loop(mode, True) for _ in range(reps)])
    print("%-8s queued: %s ms per step, %s ms of it in the call;  idle device: %s ms in the call" %
          (mode, stat(queued[:, 0]), stat(queued[:, 1]), stat(idle[:, 1])))
