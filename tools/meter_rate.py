# What jpt_meter costs: the device time of one call at 1920x1080 (or WxH) on the C3 scene (demo scene, 4 bounces, HDR accumulation)
# and on the flat worst case (0.18 everywhere, written into the accumulation through jpt_device_accum: every lane of every wave names
# one bin), beside jpt_display without bloom, which reads the same 16 B per pixel and also writes 20 B.  Each call is timed with a
# pair of HIP events on the context's stream; the clocks are raised by renders and 20 untimed calls first; the figure is the median
# of `calls` (default 50).  With JPT_LIB naming a library without jpt_meter (the parent's), only jpt_display is timed.
import ctypes as C, os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gdpathtracing_amd import capi, host, scenes
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
w, h = (1920, 1080) if len(sys.argv) <= 2 else tuple(int(v) for v in sys.argv[2].split("x"))
L = capi.lib()
hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))   # the runtime the library loaded
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
def ok(rc):
    assert rc == 0, "HIP error %d" % rc
sc = scenes.demo_scene()
ctx = host.Context(0)
ctx.build_scene(sc, capi.BUILD_SAH)
ctx.set_params(w, h, 4, capi.ACCUM_HDR_F32)
ctx.set_camera(scenes.camera_block(sc.camera, w, h))
stream = C.c_void_p()
ok(L.jpt_get_stream(ctx.h, C.byref(stream)))
ev = [C.c_void_p() for _ in range(2 * calls)]
for e in ev:
    ok(hip.hipEventCreate(C.byref(e)))
def device_us(call):
    for _ in range(20):
        call()
    ctx.sync()
    for k in range(calls):
        ok(hip.hipEventRecord(ev[2 * k], stream))
        call()
        ok(hip.hipEventRecord(ev[2 * k + 1], stream))
    ctx.sync()
    ms = C.c_float()
    out = []
    for k in range(calls):
        ok(hip.hipEventElapsedTime(C.byref(ms), ev[2 * k], ev[2 * k + 1]))
        out.append(ms.value * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))
for _ in range(4):
    ctx.render(8, 1)
have_meter = hasattr(L, "jpt_meter")
rows = []
ctx.set_display_params(bloom_levels=0)
rows.append(("jpt_display, no bloom, C3 render", device_us(ctx.display)))
if have_meter:
    rows.append(("jpt_meter, average, C3 render", device_us(ctx.meter)))
    ctx.set_meter_params(mode=capi.METER_CENTER_WEIGHTED)
    rows.append(("jpt_meter, center-weighted, C3 render", device_us(ctx.meter)))
    ctx.set_meter_params()
    print("C3 render:", ctx.read_meter(histogram=False)[0])
    rows.append(("jpt_display, no bloom, C3 render (again)", device_us(ctx.display)))
# the flat worst case: the accumulation of 32 frames of 0.18
n = C.c_size_t()
L.jpt_device_accum.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
ptr = L.jpt_device_accum(ctx.h, C.byref(n))
flat = np.full((h, w, 4), 0.18 * 32, np.float32)
assert n.value == flat.nbytes, (n.value, flat.nbytes)
ctx.sync()
ok(hip.hipMemcpy(ptr, flat.ctypes.data, flat.nbytes, 1))
rows.append(("jpt_display, no bloom, flat image", device_us(ctx.display)))
if have_meter:
    rows.append(("jpt_meter, average, flat image", device_us(ctx.meter)))
    res, hist = ctx.read_meter()
    print("flat image:", res, "non-empty bins", int(np.count_nonzero(hist)))
print("| %dx%d | median us | min | max |" % (w, h))
print("|---|---|---|---|")
for what, (med, lo, hi) in rows:
    print("| %s | %.1f | %.1f | %.1f |" % (what, med, lo, hi))
ctx.close()
