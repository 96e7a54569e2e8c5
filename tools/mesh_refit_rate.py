# An animation loop on the demo scene (51 200-triangle blob, two instances): every step deforms the blob and renders once.
# A full re-commit per step (jpt_scene_begin / add_mesh x 3 / commit, JPT_BUILD_SAH_WATERTIGHT) against jpt_scene_update_mesh
# per step; then one step of each on unique_scene (1 M triangles).  Reports ms per step and the host time of the calls.
import copy, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
w, h, spp = 1920, 1080, int(sys.argv[1]) if len(sys.argv) > 1 else 1
steps = 30

def deformed(mesh, k):
    m = copy.deepcopy(mesh)
    s = m.surfaces[0]
    v = s.vertices.astype(np.float64)
    v[:, 1] += 0.05 * np.sin(3.0 * v[:, 0] + 0.3 * k)
    s.vertices = v.astype(np.float32)
    return m

def loop(sc, blob, mode, n_steps):
    frames = [deformed(sc.meshes[blob], k) for k in range(n_steps)]
    ctx = host.Context(0); ctx.build_scene(sc, capi.BUILD_SAH_WATERTIGHT); ctx.set_params(w, h, 4, 0)
    ctx.set_camera(scenes.camera_block(sc.camera, w, h))
    for k in range(3): ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
    ctx.sync()
    t_call = 0.0
    t0 = time.perf_counter()
    for k in range(n_steps):
        ta = time.perf_counter()
        if mode == "commit":
            s2 = copy.copy(sc); s2.meshes = list(sc.meshes); s2.meshes[blob] = frames[k]
            ctx.build_scene(s2, capi.BUILD_SAH_WATERTIGHT)
        elif mode == "update":
            ctx.update_mesh(blob, frames[k])
        t_call += time.perf_counter() - ta
        ctx.accum_reset(); ctx.render(spp, 1, asynchronous=True)
    ctx.sync()
    dt = time.perf_counter() - t0
    ctx.close()
    return dt / n_steps * 1e3, t_call / n_steps * 1e3

for name, sc, n_steps in (("demo", scenes.demo_scene(), steps), ("unique", scenes.unique_scene(), 3)):
    for mode in ("commit", "update", "static"):
        ms, call = loop(sc, 2, mode, n_steps)
        print("%-6s %-6s %d triangles in the mesh, 1920x1080x%d: %.3f ms per step, of which %.3f ms in the call" %
              (name, mode, sc.meshes[2].n_tris, spp, ms, call))
