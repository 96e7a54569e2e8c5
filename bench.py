#!/usr/bin/env python3
"""bench.py -- headline metric of BASELINE.json: Mrays/s at 1920x1080, 8 spp, 4 bounces.

One "step" = one full render of the workload (accumulation reset, `spp` frames of the path-tracing
kernels + accumulation, and -- for N > 1 -- the RCCL gather of every rank's finished float4 rows to rank 0
and their assembly).  The K timed steps are queued with jpt_render_async and bracketed by barrier +
torch.cuda.synchronize() on both sides; the library overlaps the launches of consecutive queued renders, so
ms_per_step is the queued rate (the device time of one render on its own is reported as roofline.render_ms).
Scene, camera and RNG streams are synthetic and deterministic (gdpathtracing_amd/scenes.py); the scene is
resident in HBM before the timed region starts.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W     (the driver's form)
  python bench.py --gpus N ...                    starts that torch.distributed.run itself, as a child process
  python bench.py --gpus N --launcher multi ...   ONE process, one context per device (jpt_multi_*, peer-to-peer pushes)

Rank 0 prints ONE JSON line.  `value` = ray segments actually traced by all ranks / max-over-ranks time.
At N = 1 the line also carries
  parity        the image of the timed region's last step against the CPU oracle's render of the same workload (the
                oracle walks the REFERENCE tree, the GPU the native one): relative L2 on the accumulation buffer, number of
                differing pixels, tolerance 1e-4 -- the process exits with status 3 when the tolerance is exceeded;
  cpu_baseline  that oracle render's rate on the host cores;
  roofline      the dominant kernel (wf2_trace) alone: algorithmic bytes of the work it did / its launch duration, both
                from serial launches, beside the HBM traffic of the committed rocprofv3 counter passes;
  value_closeup the same scene with the camera at the box opening (every pixel sees geometry).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# The number of hardware queues per stream priority level (GPU_MAX_HW_QUEUES, read at the process's first HIP call) is the
# caller's to export and is not set here: the library measures whether six of its streams run side by side and keeps four renders
# in flight if not (the line reports both under "config").
# dmabuf IPC: RCCL between processes (and CUDA-tensor sharing) needs it on this pool's driver -- `hipIpcGetMemHandle: invalid argument`
# without it.  Set here, at the top of the file, so that the ranks the DRIVER starts with `python -m torch.distributed.run ... bench.py`
# get it too, not only the ones self_launch() starts (never over a value the caller exported).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PARITY_TOLERANCE = 1e-4  # BASELINE.json north_star: relative L2 on the accumulated buffer

# bytes one event of the traversal kernels touches in the flattened layout
WIDE_BYTES = dict(blas_expand=64, tri_tests=48, tlas_expand=64, inst_visits=64)    # two-child 64-byte records (reference-exact trees)
WIDE4_BYTES = dict(blas_expand=64, tri_tests=48, tlas_expand=64, inst_visits=64)   # native builder: four-child records, 64-byte quantised form
RAY_IN, HIT_OUT = 32, 20   # a queued ray read, a hit record written
# the same events priced in the reference layout
REF_BYTES = dict(blas_expand=96, tri_tests=48, tlas_expand=64, inst_visits=224, shaded_hits=320)

COUNTER_KEYS = ("rays", "blas_expand", "tri_tests", "tlas_expand", "inst_visits", "shaded_hits", "sky_culled")


def rel_l2(a, b):
    a = a[..., :3].astype(np.float64)
    b = b[..., :3].astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


DUMP_BUDGET_BYTES = 64_000_000   # --dump-outputs: all files together
DUMP_SEED = 20240601


def dump_outputs(out_dir, images):
    """--dump-outputs DIR: the images the timed path's last step left for its caller, {name: (H, W, ...) array}, written as
    DIR/<name>.npy in float32 (float64 arrays stay float64).  When they do not fit in DUMP_BUDGET_BYTES together, every image is
    cut to the same fixed, seeded sample of pixels -- (n, channels) arrays in increasing pixel order -- and the flat pixel indices
    (y * W + x) are written as DIR/pixel_index.npy (float64, exact).  Returns what the result line reports about it."""
    os.makedirs(out_dir, exist_ok=True)
    arrs = {k: np.asarray(v, dtype=np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in images.items()}
    h, w = next(iter(arrs.values())).shape[:2]
    n_pixels = h * w
    full = sum(a.nbytes for a in arrs.values())
    sampled = None
    if full > DUMP_BUDGET_BYTES:
        per_pixel = full // n_pixels + 8   # (+ its index)
        k = min(n_pixels, (DUMP_BUDGET_BYTES - 4096) // per_pixel)   # (room for the .npy headers)
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n_pixels, size=k, replace=False))
        arrs = {name: a.reshape(n_pixels, -1)[idx] for name, a in arrs.items()}
        arrs["pixel_index"] = idx.astype(np.float64)
        sampled = int(k)
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
    return {"dir": out_dir, "files": sorted(name + ".npy" for name in arrs), "bytes": int(sum(a.nbytes for a in arrs.values())),
            "image": [h, w], "sampled_pixels": sampled, "sample_seed": DUMP_SEED if sampled is not None else None}


def self_launch(n):
    """python -m torch.distributed.run --nnodes=1 --nproc-per-node n ... bench.py <the same arguments>, as a child process.
    --standalone: the launcher's own rendezvous picks its port (a port probed here and closed again could be taken in between)"""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(n),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL between processes needs it on this driver
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            line = ln
        else:
            sys.stderr.write(ln + "\n")
    if line is not None:
        print(line)
        sys.stdout.flush()
    elif p.returncode == 0:
        sys.stderr.write("bench.py: the launched ranks printed no JSON line\n")
        return 1
    return p.returncode


def main_multi(args):
    """--launcher multi: the same workload from ONE process through jpt_multi_* (include/jpt.h): a context per device, every
    render fanned out, each peer pushing its float4 rows to device 0 on a copy stream of its own, assembly on device 0.  One
    JSON line in the same format; `value` = ray segments of all ranks / wall time of K queued steps."""
    import torch
    from gdpathtracing_amd import capi, host, scenes
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    n = args.gpus
    have = torch.cuda.device_count()
    devices = [r % have for r in range(n)]     # fewer GPUs than ranks: a rehearsal, ranks share devices (copies are device-local)
    if args.scene == "demo":
        sc = scenes.demo_scene(args.tris)
    elif args.scene == "cornell":
        sc = scenes.cornell_scene()
    elif args.scene == "unique":
        sc = scenes.unique_scene(args.tris if args.tris != 51200 else 1_000_000)
    else:
        sc = scenes.instanced_scene()
    accum_mode = capi.ACCUM_REF_LDR8 if args.accum == "ldr8" else capi.ACCUM_HDR_F32
    builder = {"sah": capi.BUILD_SAH, "exact": capi.BUILD_REFERENCE_EXACT, "watertight": capi.BUILD_SAH_WATERTIGHT}[args.builder]
    m = host.MultiContext(devices)
    t0 = time.time()
    m.build_scene(sc, builder)
    build_s = time.time() - t0
    for r in range(n):
        m.ctx(r).set_outputs(depth=args.depth)
    m.set_gather(args.gather == "ldr")

    def sync_all():
        m.sync()
        for d in sorted(set(devices)):
            torch.cuda.synchronize(d)

    def leg(w, h, spp, bounces, steps, warmup, dump=None):
        cam = scenes.camera_block(sc.camera, w, h)
        m.set_params(w, h, bounces, accum_mode)
        m.set_camera(cam)
        rays = 0
        for r in range(n):                       # exact event counts, rank by rank (deterministic)
            c = m.ctx(r)
            c.accum_reset()
            c.render(spp, 1, counted=True)
            rays += c.stats()["rays"]

        def step():
            m.accum_reset()
            m.render(spp, 1)

        step()
        sync_all()
        for _ in range(warmup):
            step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync_all()
        elapsed = time.perf_counter() - t0
        plan = m.gather_plan()
        got = m.read_ldr() if args.gather == "ldr" else m.read_accum()
        dumped = dump_outputs(dump, {"accum": m.read_accum(), "ldr": m.read_ldr()}) if dump else None   # (the assembled images)
        solo = host.Context(devices[0])
        solo.build_scene(sc, builder)
        solo.set_params(w, h, bounces, accum_mode)
        solo.set_camera(cam)
        solo.render(spp, 1)
        same = bool(np.array_equal(got, solo.read_ldr() if args.gather == "ldr" else solo.read_accum()))
        solo.close()
        return dict(rays_per_step=rays, steps=steps, ms_per_step=round(elapsed / steps * 1e3, 4), value=round(rays * steps / elapsed / 1e6, 3),
                    verified_bit_identical_to_one_context=same, gather_plan=plan, dump_outputs=dumped)

    c3 = leg(args.width, args.height, args.spp, args.bounces, args.steps, args.warmup, dump=args.dump_outputs)
    dumped = c3.pop("dump_outputs")
    c5 = leg(3840, 2160, 16, 6, max(5, args.steps // 5), 2)
    c5.pop("dump_outputs")
    c5["workload"] = "C5: the same scene at 3840x2160, 16 spp, 6 bounces"
    out = {
        "metric": "Mrays/sec at 1920x1080, 8 spp, 4 bounces", "value": c3["value"], "unit": "Mrays/s", "n_gpus": n, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": c3["ms_per_step"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic", "launcher": "multi",
        "config": {"workload": "C3: S-demo (open Cornell cube + light + 2 instances of a %d-tri procedural mesh), %dx%d, %d spp, %d bounces, accum=%s, builder=%s"
                               % (args.tris, args.width, args.height, args.spp, args.bounces, args.accum, args.builder),
                   "unique_tris": sc.n_unique_tris, "instances": len(sc.instances), "rays_per_step": c3["rays_per_step"],
                   "parallelism": "screen strips x%d, ONE process (jpt_multi): each peer pushes its %s rows to device 0 on its own copy stream, "
                                  "assembly on device 0" % (n, "rgba8 display" if args.gather == "ldr" else "float4 accumulation"),
                   "scene_build_s": round(build_s, 4)},
        "verified_bit_identical_to_one_context": c3["verified_bit_identical_to_one_context"],
        "value_c5": c5["value"], "ms_per_step_c5": c5["ms_per_step"],
        "multi_gpu": {"ranks_seen": n, "devices": devices, "distinct_devices": len(set(devices)), "backend": "hipMemcpyPeerAsync (one process)",
                      "gather_plan": c3["gather_plan"], "c5": c5,
                      "note": "ranks share a device when the box has fewer GPUs than ranks: a rehearsal of the protocol, not a link rate"
                              if len(set(devices)) < n else "one device per rank"},
    }
    if dumped is not None:
        out["dump_outputs"] = dumped
    print(json.dumps(out))
    m.close()
    ok = c3["verified_bit_identical_to_one_context"] and c5["verified_bit_identical_to_one_context"]
    if not ok:
        sys.stderr.write("bench.py: the assembled image differs from one context's\n")
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)   # (six renders are in flight: the timed region includes the queue's fill and drain, ~1 % of 100 steps)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--tris", type=int, default=51200)
    ap.add_argument("--scene", default="demo", choices=["demo", "cornell", "inst", "unique"])
    ap.add_argument("--builder", default="sah", choices=["sah", "exact", "watertight"])
    ap.add_argument("--route", default="commit", choices=["commit", "upload", "upload-given"],
                    help="scene ingest: commit = jpt_scene_begin/.../commit with --builder (route ii); upload = the reference-layout "
                         "arrays GeometryGroup3D::build emits, handed to jpt_scene_upload_reference_layout (route i, the addon's "
                         "drop-in route: walked on the native tree, reported as `dropin` by the default run); upload-given = the "
                         "same arrays walked node for node (audit)")
    ap.add_argument("--no-dropin", action="store_true", help="skip the third timed region (route i on the same workload)")
    ap.add_argument("--accum", default="ldr8", choices=["ldr8", "hdr"])
    ap.add_argument("--kernel", default="wavefront", choices=["wavefront", "ref"])
    ap.add_argument("--camera", default="demo", choices=["demo", "closeup"],
                    help="demo = demo.tscn's camera (the box covers ~1/6 of the frame); closeup = camera at the box opening "
                         "(every pixel sees geometry; reported as value_closeup by the default run)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the oracle legs (cpu_baseline and parity)")
    ap.add_argument("--no-closeup", action="store_true", help="skip the second timed region (value_closeup)")
    ap.add_argument("--verify", action="store_true",
                    help="after the timed region, rank 0 re-renders the whole image alone and checks the assembled one bit for bit")
    ap.add_argument("--gather", choices=["ldr", "accum"], default="accum",
                    help="N > 1: what crosses the links each render -- the float4 accumulation rows (16 B/pixel: the exchange "
                         "BASELINE.json's north_star names, the default) or only the rgba8 display rows (4 B/pixel, what the "
                         "reference reads back)")
    ap.add_argument("--launcher", choices=["torchrun", "multi"], default="torchrun",
                    help="N > 1: torchrun = one process per GPU under torch.distributed (RCCL gather; started as a child process "
                         "when WORLD_SIZE is not set) -- the driver's mode; multi = ONE process, one context per device through "
                         "jpt_multi_* (what the addon's C++ host uses): every peer pushes its rows to device 0 on its own copy stream")
    ap.add_argument("--project-ranks", type=int, default=8,
                    help="N = 1 only: time every rank's share of C3 and of C5 under jpt_set_partition(r, n) for n = 2, 4, .. up to this "
                         "on the ONE device, add the modelled link time of the gather (piece bytes / 153 GB/s per xGMI link, every peer "
                         "on its own link) and the measured assembly, and report it as `projected_scaling` (measured: false) -- what "
                         "the line can say about 2/4/8 GPUs without a multi-GPU node; 0 or 1: skip")
    ap.add_argument("--preheat-ms", type=float, default=100.0,
                    help="before the W warm-up steps: keep the device busy with the workload's own renders for this long (untimed, like the "
                         "set-up).  The device drops its clocks within a fraction of a second of idling and takes tens of milliseconds of load "
                         "to raise them again: a queue of 20 renders (16 ms) started from idle reads 8-15 %% below the steady rate whatever the "
                         "library does (profiles/r06/r06l_driver_form.txt); 0: none")
    ap.add_argument("--depth", action="store_true", help="also produce the r32f depth image every render (only the temporal mode reads it)")
    ap.add_argument("--cpu-sample", default="auto")
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "profiles", "current_pmc.json"),
                    help="per-launch HBM bytes of each kernel from the committed rocprofv3 --pmc passes (tools/pmc.sh)")
    ap.add_argument("--sq-json", default=os.path.join(ROOT, "profiles", "current_sq.json"),
                    help="per-launch SQ counters of each kernel from the committed rocprofv3 --pmc passes (tools/diag.sh)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed -- the images a caller of the timed path reads back -- as "
                         "DIR/<name>.npy (float32; a fixed, seeded pixel sample when larger than 64 MB in all), for output-by-output "
                         "comparison of two builds: the inputs depend on the arguments alone")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # `python bench.py --gpus N` on its own (no torch.distributed.run around it, WORLD_SIZE unset): start the per-GPU
    # processes ourselves.  A CHILD process (never exec: nothing in this process may have touched the GPU, and nothing has --
    # torch is not imported yet), its one JSON line relayed, its exit status ours.  VERDICT r03 weak 3b.
    if args.gpus > 1 and args.launcher == "torchrun" and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    if args.gpus > 1 and args.launcher == "multi" and "WORLD_SIZE" not in os.environ:
        sys.exit(main_multi(args))

    import torch
    from gdpathtracing_amd import capi, host, partition, scenes

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" in os.environ and args.launcher == "multi":
        raise SystemExit("bench.py: --launcher multi is ONE process over all devices; it cannot run under torch.distributed.run (WORLD_SIZE is set)")
    if world != args.gpus:
        # a run asked for N GPUs must not report an n_gpus = 1 line with status 0: the launcher's world size and
        # --gpus have to agree (the driver passes both)
        raise SystemExit("bench.py: --gpus %d but the launcher's WORLD_SIZE is %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # JPT_BENCH_BACKEND=gloo is a functional rehearsal of the N > 1 flow on a box with fewer GPUs than ranks
    # (ranks share devices, the gather is staged through host memory); real runs use RCCL ("nccl").
    backend = os.environ.get("JPT_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dist = None
    # JPT_BENCH_FORCE_DIST=1: the N > 1 flow -- process group, gather, assembly, per-rank phase times, the C5 leg -- with a world of ONE
    # rank: what a box with one GPU can rehearse of the driver's 8-GPU launch with the real backend (RCCL loaded beside the library's
    # six slot streams; tests/test_gpu_full.py).  Needs MASTER_ADDR / MASTER_PORT like any rank.
    use_dist = world > 1 or os.environ.get("JPT_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import datetime
        import threading
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # a rendezvous or a first collective that hangs must be a RECORD, not the driver's 1 800 s limit: two minutes for the process
        # group, and a watchdog around everything up to the first completed gather that says what hung and exits non-zero
        limit = datetime.timedelta(seconds=120)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank), timeout=limit)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=limit)

        def _hung():
            sys.stderr.write("bench.py: rank %d of %d: no gather completed within 240 s of the process group coming up (backend %s, "
                             "HSA_ENABLE_IPC_MODE_LEGACY=%s, GPU_MAX_HW_QUEUES=%s, device %d): a peer-to-peer set-up that hangs -- "
                             "check dmabuf IPC and that every rank reached its first dist.gather\n"
                             % (rank, world, backend, os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), os.environ.get("GPU_MAX_HW_QUEUES"), local_rank))
            sys.stderr.flush()
            os._exit(5)

        watchdog = threading.Timer(240.0, _hung)
        watchdog.daemon = True
        watchdog.start()

    if args.scene == "demo":
        sc = scenes.demo_scene(args.tris)
    elif args.scene == "cornell":
        sc = scenes.cornell_scene()
    elif args.scene == "unique":
        sc = scenes.unique_scene(args.tris if args.tris != 51200 else 1_000_000)   # --tris 4000000 leaves the Infinity Cache too
    else:
        sc = scenes.instanced_scene()
    closeup_camera = scenes.CameraDesc(scenes.transform12(None, (0.0, 0.0, 4.2)), fov_deg=75.0)
    if args.camera == "closeup":
        sc.camera = closeup_camera
    W, H, spp, bounces = args.width, args.height, args.spp, args.bounces
    cam = scenes.camera_block(sc.camera, W, H)
    accum_mode = capi.ACCUM_REF_LDR8 if args.accum == "ldr8" else capi.ACCUM_HDR_F32
    builder = {"sah": capi.BUILD_SAH, "exact": capi.BUILD_REFERENCE_EXACT, "watertight": capi.BUILD_SAH_WATERTIGHT}[args.builder]

    def reference_layout_arrays():
        """what GeometryGroup3D::build leaves in its vectors (geometry_group3d.cpp:305-365, get_*_buffer :40-68): made by
        the library's reference-exact builder on a host-only context (byte-identical to the reference's; tests)"""
        from gdpathtracing_amd import wire
        hc = host.Context(-1)
        hc.build_scene(sc, capi.BUILD_REFERENCE_EXACT)
        arrs = [hc.reference_buffer(w, d) for w, d in (
            (capi.BUF_TRI_GEOMETRY, wire.TRI_GEOMETRY), (capi.BUF_TRI_DATA, wire.TRI_DATA), (capi.BUF_MATERIALS, wire.MATERIAL),
            (capi.BUF_BVH_NODES, wire.BVH_NODE), (capi.BUF_INSTANCES, wire.BLAS_INSTANCE), (capi.BUF_TLAS_NODES, wire.TLAS_NODE))]
        hc.close()
        return arrs

    ctx = host.Context(local_rank)
    if args.route == "commit":
        t0 = time.time()
        ctx.build_scene(sc, builder)
        build_s = time.time() - t0
    else:
        arrs = reference_layout_arrays()
        t0 = time.time()
        ctx.upload_reference_layout(*arrs, textures=sc.textures, as_given=args.route == "upload-given")
        build_s = time.time() - t0
    ctx.set_partition(rank, world)
    # the r32f depth image (main.glsl:435) has one reader, TemporalReprojection; the benchmarked mode is progressive rendering,
    # where nothing ever reads it: not produced (jpt_set_outputs; --depth keeps it)
    ctx.set_outputs(depth=args.depth)
    ctx.set_params(W, H, bounces, accum_mode)
    ctx.set_camera(cam)
    ctx.set_kernel({"wavefront": capi.KERNEL_WAVEFRONT, "ref": capi.KERNEL_REFERENCE_LAYOUT}[args.kernel])
    # One explicit (non-null) stream carries the renders, the timing events and the collective: the context's own,
    # made torch's current stream.  (Not a stream from torch's pool: the pool is 32 streams created at once, the HIP
    # runtime deals streams to its hardware queues round-robin in creation order, and the library's slot streams,
    # created next, would land on the very queue the pool stream sits on -- one frame per render 0.40 instead of 0.31 ms.)
    stream = torch.cuda.ExternalStream(ctx.get_stream(), device=torch.device("cuda", local_rank))
    torch.cuda.set_stream(stream)
    ctx.set_kernel_timing(False)   # per-launch HIP events serialise the launches: they are collected after the timed region

    # gather plumbing (N > 1): the local piece (rgba8 display rows, or float4 sums) viewed as a torch tensor, no copy;
    # made again whenever jpt_set_params changes the framebuffers (the C5 leg)
    gp = {"piece": None, "gathered": None}

    def setup_gather():
        if not use_dist:
            return
        ptr, nbytes = ctx.device_ldr() if args.gather == "ldr" else ctx.device_accum()
        typestr, tdtype = ("<i4", torch.int32) if args.gather == "ldr" else ("<f4", torch.float32)

        class _View:
            __cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": typestr, "data": (ptr, False), "version": 2}

        gp["piece"] = torch.as_tensor(_View(), device=torch.device("cuda", local_rank))
        gp["gathered"] = torch.empty((world, nbytes // 4), dtype=tdtype, device=gp["piece"].device) if rank == 0 else None

    setup_gather()

    def gather():
        """the one exchange of a render: every rank's piece to rank 0"""
        piece, gathered = gp["piece"], gp["gathered"]
        if backend == "nccl":
            # direct point-to-point gather: every peer sends its piece over its own xGMI link
            partition.gather_to_rank0(piece, dist, rank, world, gathered)
        else:
            stream.synchronize()
            g = partition.gather_to_rank0(piece.cpu(), dist, rank, world)
            if rank == 0:
                gathered.copy_(g)

    def assemble():
        if rank == 0:
            if args.gather == "ldr":
                ctx.assemble_ldr_from_ranks(gp["gathered"].data_ptr(), world)
            else:
                ctx.assemble_from_ranks(gp["gathered"].data_ptr(), world)

    cur = {"spp": spp}

    def step():
        ctx.accum_reset()
        ctx.render(cur["spp"], 1, asynchronous=True)
        if use_dist:
            gather()
            assemble()

    def phase_split(n=3):
        """per-rank device time of a step's three phases -- render, gather, assemble -- from events on the context's
        stream (which orders all three), one step at a time (nothing else in flight); [world, 3] ms on every rank"""
        acc = np.zeros(3)
        for _ in range(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            barrier()
            ctx.accum_reset()
            ev[0].record(stream)
            ctx.render(cur["spp"], 1, asynchronous=True)
            ev[1].record(stream)
            gather()
            ev[2].record(stream)
            assemble()
            ev[3].record(stream)
            barrier()
            acc += [ev[k].elapsed_time(ev[k + 1]) for k in range(3)]
        mine = torch.tensor(acc / n, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        return [[round(float(x), 4) for x in t.tolist()] for t in every]

    def counted(n_bounces, w=None, h=None, n_spp=None):
        """exact event counts of one step (deterministic), outside the timed region; summed over the ranks"""
        ctx.set_params(w or W, h or H, n_bounces, accum_mode)
        ctx.accum_reset()
        ctx.render(n_spp or spp, 1, counted=True)
        st = ctx.stats()
        t = torch.tensor([st[k] for k in COUNTER_KEYS], dtype=torch.int64, device="cuda" if backend == "nccl" else "cpu")
        if use_dist:
            dist.all_reduce(t)
        return dict(zip(COUNTER_KEYS, (int(x) for x in t.tolist())))

    primary = counted(0) if args.kernel == "wavefront" else None   # the bounce-0 launch alone
    total = counted(bounces)                                        # (leaves the context at the workload's bounce count)
    rays = total["rays"]

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n_steps):
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        barrier()
        elapsed = time.perf_counter() - t0
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        if use_dist:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # Set-up, like the allocations above: the library creates its pipeline slots (a stream and a workspace each) at
    # the first queued render -- ~25 ms once per context, which is not a property of a step (--warmup 0 is honoured
    # as "no warm-up steps", not as "time the resource creation").
    step()
    barrier()
    if use_dist:
        watchdog.cancel()   # the first gather (and the barrier behind it) completed on every rank
    # ... and so are the device's clocks: everything up to here was blocking renders with host work in between, and the device clocks
    # down when it idles.  The workload's own renders, queued, for --preheat-ms (reported in config.preheat_ms); then the W warm-up steps.
    def preheat():
        n, t_heat = 0, time.perf_counter()
        while args.preheat_ms > 0:
            for _ in range(10):
                step()
            barrier()
            n += 10
            # (every rank must leave the loop after the same batch -- the steps hold collectives: the ranks agree on the largest elapsed time)
            t = torch.tensor([(time.perf_counter() - t_heat) * 1e3], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            if use_dist:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if float(t.item()) >= args.preheat_ms or n >= 2000:
                break
        return n

    preheat_steps = preheat()
    for _ in range(args.warmup):
        step()
    barrier()
    # Timed region.  Steps are queued back to back and the closing barrier waits for all of them: the library runs
    # the path kernels of consecutive asynchronous renders on its pipeline slots' streams (four workspaces), so one
    # render's launch tails overlap the next renders' kernels; the accumulation kernels run in call order, chained
    # through the context's stream.  (A queue of K renders takes K x rate + the latency of the last one, ~3 ms: small
    # K reads lower.)
    elapsed = timed(args.steps)
    renders_in_flight = ctx.renders_in_flight()   # 6 where six of the library's streams run side by side, else 4
    gpu_image = ctx.read_accum() if (world == 1 and rank == 0) else None   # the image the timed region left behind (parity)
    dumped = None
    if args.dump_outputs and rank == 0:
        # the last timed step's images as a caller reads them back; under torch.distributed the assembled one (the gathered kind)
        if not use_dist:
            images = {"accum": gpu_image, "ldr": ctx.read_ldr()}
            if args.depth:
                images["depth"] = ctx.read_depth()
        elif args.gather == "ldr":
            images = {"ldr": ctx.read_ldr()}
        else:
            images = {"accum": ctx.read_accum()}
        dumped = dump_outputs(args.dump_outputs, images)
    verified = None
    if (args.verify or use_dist) and rank == 0:   # N > 1: always -- the assembled image of the last timed step against one context's
        got = ctx.read_ldr() if (use_dist and args.gather == "ldr") else ctx.read_accum()
        solo = host.Context(local_rank)
        solo.build_scene(sc, builder)
        solo.set_params(W, H, bounces, accum_mode)
        solo.set_camera(cam)
        solo.render(spp, 1)
        verified = bool(np.array_equal(got, solo.read_ldr() if (use_dist and args.gather == "ldr") else solo.read_accum()))
        solo.close()

    # Launch durations of the traversal kernels, measured live with HIP events on the stream they are launched on: the
    # library brackets every traversal launch when kernel timing is on, which also makes it run the launches one after
    # another (in the timed region above launches of different renders overlap, so a per-launch duration is not defined
    # there).  Three untimed renders, after the timed region.
    ctx.set_kernel_timing(True)
    trace_ms, primary_ms, render_ms = [], [], []
    for _ in range(3):
        ctx.accum_reset()
        ctx.render(spp, 1)
        st = ctx.stats()
        trace_ms.append(st["last_trace_ms"])
        primary_ms.append(st["last_primary_ms"])
        render_ms.append(st["last_render_ms"])   # device time of ONE render on its own (no overlap with a neighbour)
    ctx.set_kernel_timing(False)
    # One render at a time as the library runs it when nothing is queued behind it (no per-launch events: frame groups and
    # chained segments by the library's rule) -- what the addon's blocking render() per Godot frame gets
    blocking_ms = []
    for k in range(7):
        ctx.accum_reset()
        ctx.render(spp, 1)
        if k >= 2: blocking_ms.append(ctx.stats()["last_render_ms"])   # (the first ones create the frame groups' streams)
    if args.kernel == "wavefront":
        dom, n_dom = "wf2_trace", max(bounces, 1)
        dom_ms = (float(np.mean(trace_ms)) - float(np.mean(primary_ms))) / n_dom    # average duration of ONE wf2_trace launch
    else:
        dom, n_dom = "ref_frame_kernel", spp
        dom_ms = float(np.mean(trace_ms)) / n_dom

    # N > 1: what the ranks spend where, and a second timed region at C5's size -- the configuration BASELINE.json tiles
    # over 8 GPUs (3840x2160, 16 spp, 6 bounces: 8 ms of work on one GPU, against C3's 1 ms and eleven dependent launches)
    multi = None
    if use_dist:
        multi = {"ranks_seen": dist.get_world_size(), "backend": backend}
        # what every rank ran with (VERDICT r05 task 2d): the two variables a multi-process run depends on, and the renders the
        # library kept in flight there
        mine = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.get_device_name(local_rank),
                "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                "renders_in_flight": renders_in_flight}
        every = [None] * world
        dist.all_gather_object(every, mine)
        multi["ranks"] = every
        try:
            multi["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:
            multi["rccl_version"] = None
        setup_gather()                      # (counted() re-made the framebuffers)
        multi["c3_phase_ms_per_rank"] = phase_split()
        W5, H5, SPP5, B5 = 3840, 2160, 16, 6
        total5 = counted(B5, W5, H5, SPP5)
        ctx.set_camera(scenes.camera_block(sc.camera, W5, H5))
        setup_gather()
        cur["spp"] = SPP5
        step()
        barrier()
        for _ in range(2):
            step()
        barrier()
        steps5 = max(8, (2 * args.steps) // 5)
        elapsed5 = timed(steps5)
        got5 = (ctx.read_ldr() if args.gather == "ldr" else ctx.read_accum()) if rank == 0 else None
        multi["c5_phase_ms_per_rank"] = phase_split(2)
        multi["c5"] = dict(workload="C5: the same scene at %dx%d, %d spp, %d bounces" % (W5, H5, SPP5, B5), rays_per_step=total5["rays"], steps=steps5,
                           ms_per_step=round(elapsed5 / steps5 * 1e3, 4), value=round(total5["rays"] * steps5 / elapsed5 / 1e6, 3))
        if rank == 0:
            solo = host.Context(local_rank)
            solo.build_scene(sc, builder)
            solo.set_params(W5, H5, B5, accum_mode)
            solo.set_camera(scenes.camera_block(sc.camera, W5, H5))
            solo.render(SPP5, 1)
            multi["c5"]["verified_bit_identical_to_one_context"] = bool(np.array_equal(got5, solo.read_ldr() if args.gather == "ldr" else solo.read_accum()))
            solo.close()
        cur["spp"] = spp
        ctx.set_params(W, H, bounces, accum_mode)
        ctx.set_camera(cam)
        setup_gather()

    # ---- what 2 / 4 / 8 GPUs would do, projected from ONE: each rank's share timed here, the link modelled (VERDICT r04 task 2) ----
    projected = None
    if world == 1 and not use_dist and args.project_ranks > 1 and args.kernel == "wavefront":
        XGMI_LINK_GBS = 153.0     # ~153 GB/s per xGMI link, one link per peer pair
        LINK_LATENCY_MS = 0.01    # one peer copy's fixed cost (order of magnitude of a hipMemcpyPeerAsync on an idle link)

        def project_config(w, h, n_spp, n_bounces, n_steps, whole_ms, whole_rays):
            pcam = scenes.camera_block(sc.camera, w, h)
            res = {}
            n = 2
            while n <= args.project_ranks:
                per_rank, rays_rank = [], []
                for r in range(n):
                    ctx.set_partition(r, n)
                    ctx.set_params(w, h, n_bounces, accum_mode)
                    ctx.set_camera(pcam)
                    ctx.accum_reset()
                    ctx.render(n_spp, 1)
                    rays_rank.append(ctx.stats()["rays"])
                    for _ in range(3):
                        ctx.accum_reset()
                        ctx.render(n_spp, 1, asynchronous=True)
                    barrier()
                    t0 = time.perf_counter()
                    for _ in range(n_steps):
                        ctx.accum_reset()
                        ctx.render(n_spp, 1, asynchronous=True)
                    barrier()
                    per_rank.append((time.perf_counter() - t0) / n_steps * 1e3)
                # rank 0's assembly of the gathered float4 rows, measured (the other ranks' pieces: whatever the buffer holds)
                ctx.set_partition(0, n)
                ctx.set_params(w, h, n_bounces, accum_mode)
                ctx.set_camera(pcam)
                ctx.accum_reset()
                ctx.render(n_spp, 1)
                piece_rows = partition.max_local_rows(h, n)
                gathered = torch.zeros((n, piece_rows * w * 4), dtype=torch.float32, device="cuda")
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ctx.assemble_from_ranks(gathered.data_ptr(), n)
                barrier()
                ev[0].record(stream)
                for _ in range(5):
                    ctx.assemble_from_ranks(gathered.data_ptr(), n)
                ev[1].record(stream)
                barrier()
                assemble_ms = ev[0].elapsed_time(ev[1]) / 5
                del gathered
                piece_bytes = piece_rows * w * 16
                gather_ms = piece_bytes / (XGMI_LINK_GBS * 1e9) * 1e3 + LINK_LATENCY_MS    # n - 1 peers, each on its own link, side by side
                serial = max(per_rank) + gather_ms + assemble_ms
                overlapped = max(max(per_rank), gather_ms + assemble_ms)   # gather + assembly of render k behind render k + 1 (queued steps)
                res[str(n)] = dict(rank_ms=[round(x, 4) for x in per_rank], rank_ms_max=round(max(per_rank), 4), rank_ms_mean=round(float(np.mean(per_rank)), 4),
                                   rays_per_rank=rays_rank, rays_sum_equals_whole=bool(sum(rays_rank) == whole_rays),
                                   piece_bytes=int(piece_bytes), gather_ms_modelled=round(gather_ms, 4), assemble_ms_measured=round(assemble_ms, 4),
                                   step_ms_serial=round(serial, 4), step_ms_overlapped=round(overlapped, 4),
                                   speedup_serial=round(whole_ms / serial, 3), speedup_overlapped=round(whole_ms / overlapped, 3),
                                   mrays_overlapped=round(whole_rays / overlapped / 1e3, 1))
                n *= 2
            return res

        c3_ms = elapsed / args.steps * 1e3
        projected = {"measured": False,
                     "method": "every rank's share (jpt_set_partition(r, n): 8-row strips dealt round-robin) rendered on THIS device, queued like the headline; "
                               "gather = piece bytes / %.0f GB/s (one xGMI link per peer, all peers at once) + %.0f us; assembly measured on this device; "
                               "speedup = one GPU's ms_per_step / (slowest rank + gather + assembly [serial], or their maximum [overlapped: queued steps])"
                               % (XGMI_LINK_GBS, LINK_LATENCY_MS * 1e3),
                     "c3": dict(one_gpu_ms=round(c3_ms, 4), ranks=project_config(W, H, spp, bounces, args.steps, c3_ms, rays))}   # (as many queued steps as the headline: a shorter queue reads higher per step)
        # C5 (3840x2160, 16 spp, 6 bounces): one GPU's own rate first
        W5, H5, SPP5, B5 = 3840, 2160, 16, 6
        ctx.set_partition(0, 1)
        ctx.set_params(W5, H5, B5, accum_mode)
        ctx.set_camera(scenes.camera_block(sc.camera, W5, H5))
        ctx.accum_reset()
        ctx.render(SPP5, 1)
        rays5 = ctx.stats()["rays"]
        for _ in range(2):
            ctx.accum_reset()
            ctx.render(SPP5, 1, asynchronous=True)
        barrier()
        steps5 = max(8, (2 * args.steps) // 5)   # (40 by default: six renders are in flight, a queue of ten reads 15 % higher per step)
        t0 = time.perf_counter()
        for _ in range(steps5):
            ctx.accum_reset()
            ctx.render(SPP5, 1, asynchronous=True)
        barrier()
        c5_ms = (time.perf_counter() - t0) / steps5 * 1e3
        projected["c5"] = dict(one_gpu_ms=round(c5_ms, 4), rays_per_step=rays5, one_gpu_mrays=round(rays5 / c5_ms / 1e3, 1),
                               ranks=project_config(W5, H5, SPP5, B5, steps5, c5_ms, rays5))
        ctx.set_partition(0, 1)
        ctx.set_params(W, H, bounces, accum_mode)
        ctx.set_camera(cam)
        ctx.accum_reset()

    # the close-up camera on the same context: every pixel sees geometry, so rays/s here is the traversal rate proper
    closeup = None
    if world == 1 and not use_dist and args.camera == "demo" and args.scene == "demo" and not args.no_closeup:
        ctx.set_camera(scenes.camera_block(closeup_camera, W, H))
        ctx.accum_reset()
        ctx.render(spp, 1)
        c_rays = ctx.stats()["rays"]
        c_steps = max(10, args.steps)   # (as many as the headline: the timed region includes the pipeline's fill and drain)
        preheat()
        for _ in range(2):
            step()
        barrier()
        c_elapsed = timed(c_steps)
        closeup = dict(value=round(c_rays * c_steps / c_elapsed / 1e6, 3), ms_per_step=round(c_elapsed / c_steps * 1e3, 4),
                       rays_per_step=c_rays, steps=c_steps)
        ctx.set_camera(cam)

    # the drop-in route on the same workload: the reference-layout arrays of the same scene handed to
    # jpt_scene_upload_reference_layout (what the addon does when GeometryGroup3D::build() stays), on a second context
    dropin = None
    if world == 1 and not use_dist and args.route == "commit" and args.kernel == "wavefront" and not args.no_dropin and gpu_image is not None:
        arrs = reference_layout_arrays()
        dctx = host.Context(local_rank)
        t0 = time.perf_counter()
        dctx.upload_reference_layout(*arrs, textures=sc.textures)
        upload_s = time.perf_counter() - t0
        kind = dctx.tree_kind()
        dctx.set_outputs(depth=args.depth)
        dctx.set_params(W, H, bounces, accum_mode)
        dctx.set_camera(cam)
        main_ctx, ctx = ctx, dctx      # step() / timed() drive `ctx`
        try:
            torch.cuda.set_stream(torch.cuda.ExternalStream(dctx.get_stream(), device=torch.device("cuda", local_rank)))
            dctx.accum_reset()
            dctx.render(spp, 1)
            d_rays = dctx.stats()["rays"]
            step()
            barrier()
            preheat()                      # (the upload above was host work: the device has idled and clocked down)
            for _ in range(2):
                step()
            barrier()
            d_steps = args.steps           # (as many as the headline: a shorter queue reads a few per cent higher per step)
            d_elapsed = timed(d_steps)
            d_image = dctx.read_accum()
        finally:
            ctx = main_ctx
            torch.cuda.set_stream(stream)
        dropin = dict(value=round(d_rays * d_steps / d_elapsed / 1e6, 3), ms_per_step=round(d_elapsed / d_steps * 1e3, 4), steps=d_steps,
                      tree={capi.TREE_AS_GIVEN: "as given", capi.TREE_NATIVE_REACH: "native + reach records"}.get(kind, str(kind)),
                      upload_s=round(upload_s, 4), note=dctx.upload_note() or None, renders_in_flight=dctx.renders_in_flight(),
                      differing_pixels_vs_commit_route=int((d_image != gpu_image).any(axis=-1).sum()),
                      what="jpt_scene_upload_reference_layout of the reference-layout arrays (route i), same workload, queued renders")
        dctx.close()

    status = 0
    if rank == 0:
        n_pixels = W * H
        ms_per_step = elapsed / args.steps * 1e3
        mrays = rays * args.steps / elapsed / 1e6
        # ---- roofline of the dominant kernel alone, from the work it DID: the events of the bounce launches are the
        # counted render's totals minus those of a bounce-0-only render; sky-culled primaries fetch nothing and are in
        # neither (they belong to the bounce-0 launch anyway)
        table = WIDE4_BYTES if (args.builder != "exact" and args.kernel == "wavefront" and args.route != "upload-given") else WIDE_BYTES
        if args.kernel == "wavefront":
            ev = {k: total[k] - primary[k] for k in table}
            dom_rays = total["rays"] - primary["rays"]
        else:
            ev, dom_rays = {k: total[k] for k in table}, total["rays"]
        alg = (sum(ev[k] * v for k, v in table.items()) + dom_rays * (RAY_IN + HIT_OUT)) / world / n_dom     # per launch, this rank
        achieved = alg / (dom_ms * 1e-3) / 1e9
        alg_ref = sum(total[k] * v for k, v in REF_BYTES.items()) + n_pixels * spp * 48
        # HBM traffic of that kernel: PMC counters cannot be read from inside the process, so the per-launch figure comes
        # from the committed rocprofv3 passes of this same command (profiles/)
        traffic = traffic_src = valu = stale = None
        from tools.csrc_sha import csrc_sha
        kernels_sha = csrc_sha()
        default_run = (W, H, spp, bounces, args.tris, args.scene, args.builder, world, args.camera, args.kernel, args.route) == \
                      (1920, 1080, 8, 4, 51200, "demo", "sah", 1, "demo", "wavefront", "commit")
        # the other profiled workloads (tools/workload_profiles.sh): same size and settings, another scene / camera; their
        # counter passes are in profiles/current_{pmc,sq}_<workload>.json
        workload_key = None
        if (W, H, spp, bounces, args.builder, world, args.kernel, args.route) == (1920, 1080, 8, 4, "sah", 1, "wavefront", "commit"):
            workload_key = {("demo", "demo", 51200): "c3", ("demo", "closeup", 51200): "closeup", ("inst", "demo", 51200): "c4",
                            ("unique", "demo", 51200): "unique", ("unique", "demo", 4000000): "unique4m"}.get((args.scene, args.camera, args.tris))
        if workload_key not in (None, "c3"):
            default_run = True
            if args.pmc_json == os.path.join(ROOT, "profiles", "current_pmc.json"):
                args.pmc_json = os.path.join(ROOT, "profiles", "current_pmc_%s.json" % workload_key)
            if args.sq_json == os.path.join(ROOT, "profiles", "current_sq.json"):
                args.sq_json = os.path.join(ROOT, "profiles", "current_sq_%s.json" % workload_key)
        if default_run and os.path.exists(args.pmc_json):
            try:
                pj = json.load(open(args.pmc_json))
                if pj.get("_meta", {}).get("csrc_sha") != kernels_sha:
                    raise LookupError("profiled on other kernels")
                traffic = int(pj[dom]["hbm_bytes_per_launch"])
                traffic_src = os.path.relpath(args.pmc_json, ROOT) + ": read bytes [%s] + WRITE_SIZE KiB per launch of %s, separate --pmc passes" % (
                    pj[dom].get("fetch_method", "2 * FETCH_SIZE"), dom)
            except LookupError:
                traffic, stale = None, "profiles/current_pmc.json was collected on other kernel sources than the ones running (csrc hash %s): re-run tools/round_profiles.sh" % kernels_sha
            except Exception:
                traffic = None
        if default_run and os.path.exists(args.sq_json):
            try:
                sj = json.load(open(args.sq_json))
                if sj.get("_meta", {}).get("csrc_sha") != kernels_sha:
                    raise LookupError("profiled on other kernels")
                valu = sj.get(dom)
            except LookupError:
                valu, stale = None, "profiles/current_sq.json / current_pmc.json were collected on other kernel sources than the ones running (csrc hash %s): re-run tools/round_profiles.sh" % kernels_sha
            except Exception:
                valu = None
        hbm_frac = round(traffic / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if traffic else None
        valu_issue_frac = (valu or {}).get("valu_issue_frac")
        # How full is the chip's VALU issue capacity at the QUEUED rate?  Every kernel of a render, its serial launch time x its share of
        # the issue capacity (both from the committed passes) x its launches per render, over the measured time per queued render: the
        # launches of the renders in flight fill each other's idle issue slots, and at ~1 the queued rate IS the instruction stream's
        # roofline -- only fewer or cheaper instructions go faster (LAB_NOTEBOOK.md Part I section 5).
        queued_issue = None
        try:
            if valu is not None and traffic is not None and args.kernel == "wavefront":
                per_render = {"wf2_primary": 1, "wf2_trace": max(bounces, 0), "wf2_shade": bounces + 1, "wf2_finish": 1, "wf2_accumulate": 1}
                busy_us = sum(n * pj[k]["time"]["avg_us"] * (sj[k].get("valu_issue_frac") or 0.0) for k, n in per_render.items() if k in pj and k in sj)
                queued_issue = {"ratio": round(busy_us / (ms_per_step * 1e3), 4), "issue_us_per_render": round(busy_us, 1),
                                "note": "sum over a render's kernels of serial launch time x valu_issue_frac x launches, / ms_per_step; ~1 (within the "
                                        "instruction-pricing model's few per cent) = the queued rate is the instruction stream's VALU-issue roofline"}
        except Exception:
            queued_issue = None
        # what binds the dominant kernel: the largest of the utilisations this line can state (null when they are not known)
        # ... one of: "hbm" (counter traffic / duration >= 0.6 of the 8 TB/s peak: 6.3 TB/s is what the chip sustains), "valu_issue"
        # (>= 0.6 of the issue capacity), else "dependent_fetch_latency" -- neither the memory system nor the ALUs are busy, the
        # waves sit in s_waitcnt on the next record of their rays' chains (wait_frac says for what share of their cycles)
        binding = None
        if valu_issue_frac is not None and hbm_frac is not None:
            if hbm_frac >= 0.6 and hbm_frac >= valu_issue_frac:
                binding = "hbm"
            elif valu_issue_frac >= 0.6:
                binding = "valu_issue"
            else:
                binding = "dependent_fetch_latency"
        # ---- the line's roofline: the resource that BINDS the dominant kernel (VERDICT r05 task 3).  The tree is cache-resident, so
        # bytes asked for / duration against the HBM peak is not a bound (the same arithmetic exceeds 1 on the close-up); what the
        # counters show is VALU issue.  bound = "valu_issue": achieved = wave-level VALU instructions x the ISA's priced cycles per
        # instruction / launch duration (G issue-cycles/s over the chip's 1024 SIMDs), peak = 1024 SIMDs x the measured clock, frac =
        # their ratio (valu_issue_frac of the committed SQ passes); lane_frac = frac x the share of the 64 lanes those instructions
        # have enabled = the share of the chip's lane throughput the launch uses.  The HBM pair stays, under `hbm`: counter traffic
        # (what reaches the fabric) and the cache-served request rate (today's algorithmic bytes / duration).  Without current
        # counter passes (sources changed since: profiles_stale) nothing can be said about the binding and frac is null.
        v = valu or {}
        lane_util = v.get("lane_utilisation")
        hbm_block = {
            "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "achieved": round(traffic / (dom_ms * 1e-3) / 1e9, 2) if traffic else None, "frac": hbm_frac,
            "traffic": traffic, "traffic_source": traffic_src,
            "algorithmic_bytes": int(alg),
            "cache_served_achieved": round(achieved, 2), "cache_served_frac": round(achieved / HBM_PEAK_GBS, 5),
            "note": "achieved / frac = bytes that reach the fabric per launch (rocprofv3 PMC passes) / launch duration / 8 TB/s; cache_served_* = "
                    "bytes the kernel ASKS for (records, triangles, instances, rays in, hits out: exact event counts of the bounce launches x "
                    "record sizes) / duration -- requests the L2s and the Infinity Cache serve (the scene is 6 MB), NOT a bound: it may exceed 1",
            "compulsory_framebuffer_bytes_per_render": int(n_pixels * (16 + 4 + 4)),
            "ref_layout_algorithmic_bytes_per_render": int(alg_ref),
        }
        if valu_issue_frac is not None and binding in ("valu_issue", "dependent_fetch_latency"):
            peak_issue = 1024.0 * float(v.get("clock_ghz") or 2.4)                     # G issue-cycles/s: 256 CUs x 4 SIMDs x clock
            head = {"bound": "valu_issue", "achieved": round(valu_issue_frac * peak_issue, 1), "peak": round(peak_issue, 1),
                    "unit": "G VALU issue-cycles/s", "frac": valu_issue_frac,
                    "lane_frac": round(valu_issue_frac * lane_util, 4) if lane_util is not None else None}
        elif binding == "hbm":
            head = {"bound": "hbm", "achieved": hbm_block["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm_frac, "lane_frac": None}
        else:
            head = {"bound": None, "achieved": None, "peak": None, "unit": None, "frac": None, "lane_frac": None}
        roofline = dict(head)
        roofline.update({
            "kernel": "%s (%d launches per render, serial launches)" % (dom, n_dom),
            "kernel_ms": round(dom_ms, 4),
            "traffic": traffic,
            "binding": binding,
            "hbm": hbm_block,
            "wait_frac": v.get("wait_frac"), "l2_hit": v.get("l2_hit"),
            # from the committed SQ-counter passes of this command (profiles/current_sq.json, stamped with the hash of the kernel
            # sources they ran on; null + `profiles_stale` when the sources have changed since)
            "valu_issue_frac": valu_issue_frac,
            "lane_utilisation": lane_util,
            "queued_valu_issue": queued_issue,
            "valu": valu,
            "profiles_stale": stale,
            "kernels_sha": kernels_sha,
            "note": "frac = share of the chip's VALU issue capacity the dominant kernel's launches use (wave-level VALU instructions x the "
                    "cycles the ISA prices them at / (1024 SIMDs x launch cycles)); lane_frac = frac x enabled lanes / 64.  binding = "
                    "\"valu_issue\" at frac >= 0.6, else \"dependent_fetch_latency\" (the waves sit in s_waitcnt on the next record of "
                    "their rays' chains: wait_frac); \"hbm\" only when counter traffic / duration reaches 0.6 of the 8 TB/s peak.",
            "primary_kernel_ms": round(float(np.mean(primary_ms)), 4),
            "render_ms": round(float(np.mean(render_ms)), 4),
            "render_ms_note": "one render alone, launches serialised (kernel timing on); ms_per_step is the pipelined rate",
            "blocking_render_ms": round(float(np.mean(blocking_ms)), 4),
        })
        for name, f in (("roofline.frac", roofline["frac"]), ("roofline.hbm.frac", hbm_frac), ("roofline.lane_frac", roofline["lane_frac"])):
            if f is not None and not (0.0 <= f <= 1.0):
                sys.stderr.write("bench.py: %s = %r is not a fraction of a peak\n" % (name, f))
                status = 4
        sky = total.get("sky_culled", 0)
        traced = rays - sky
        out = {
            "metric": "Mrays/sec at 1920x1080, 8 spp, 4 bounces",
            "value": round(mrays, 3),
            "unit": "Mrays/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": ("C3: S-demo (open Cornell cube + light + 2 instances of a %d-tri procedural mesh), %dx%d, %d spp, "
                             "%d bounces, accum=%s, builder=%s, kernel=%s" % (args.tris, W, H, spp, bounces, args.accum, args.builder if args.route == "commit" else args.route, args.kernel)
                             if (args.scene == "demo" and args.camera == "demo") else "%s (camera %s) %dx%d %d spp %d bounces" % (sc.name, args.camera, W, H, spp, bounces))
                            + " -- `value` counts %.2f M ray segments per step (every ray_trace() call the reference makes), %.2f M of them sky-culled "
                              "primaries that NO kernel walks; `value_traced` counts the %.2f M a kernel does walk" % (rays / 1e6, sky / 1e6, traced / 1e6),
                "unique_tris": sc.n_unique_tris, "instances": len(sc.instances),
                "rays_per_step": rays, "nominal_rays_per_step": n_pixels * spp * (bounces + 1),
                "parallelism": "screen strips x%d" % world + ("" if world == 1 else ", gather of %s rows to rank 0" % ("rgba8 display" if args.gather == "ldr" else "float4 accumulation")),
                "scene_build_s": round(build_s, 4),
                "renders_in_flight": renders_in_flight, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                "preheat_ms": args.preheat_ms, "preheat_steps": preheat_steps,
                "preheat_note": "untimed renders of this workload before the W warm-up steps of every timed leg: the device clocks down within 50 ms of idling and "
                                "needs ~12 ms of load to come back (tools/clock_ramp.py, profiles/r06/r06n); from idle a 20-step queue reads 5-15 % slower "
                                "(profiles/r06/r06l, r06m); --preheat-ms 0 switches it off",
                "outputs": "float4 accumulation + rgba8 display" + (" + r32f depth" if args.depth else " (depth image off: only temporal reprojection reads it)"),
            },
            "roofline": roofline,
            "counters": total,
        }
        # (`rays` counts every ray_trace() invocation the reference would make; sky_culled of them are primaries
        # whose pixel lies outside the screen rectangles of the TLAS root's boxes: decided on the host, no kernel walks them)
        out["traced_rays_per_step"] = traced
        out["value_traced"] = round(traced * args.steps / elapsed / 1e6, 3)
        out["value_blocking"] = round(rays / (float(np.mean(blocking_ms)) * 1e-3) / 1e6, 3) if np.mean(blocking_ms) > 0 else None
        out["value_notes"] = ("value = rays_per_step / ms_per_step (queued renders, config.renders_in_flight of them in flight); value_traced counts only the rays a "
                              "kernel walks (rays - sky_culled); value_blocking = rays_per_step / roofline.blocking_render_ms (the device "
                              "time of one render with nothing queued behind it, as the library runs it; roofline.render_ms is the same "
                              "render with its launches serialised for per-kernel timing)")
        if projected is not None:
            out["projected_scaling"] = projected
        if closeup is not None:
            out["value_closeup"] = closeup["value"]
            out["closeup"] = closeup
        if dropin is not None:
            out["value_dropin"] = dropin["value"]
            out["dropin"] = dropin
        if multi is not None:
            out["value_c5"] = multi["c5"]["value"]
            out["ms_per_step_c5"] = multi["c5"]["ms_per_step"]
            out["multi_gpu"] = multi
            out["multi_gpu"]["phase_columns"] = ["render_ms", "gather_ms", "assemble_ms"]
            out["multi_gpu"]["note"] = ("phase times: one step at a time, HIP events on each rank's context stream (render = path kernels + accumulation "
                                        "of the rank's strips; gather = the rank's rows to rank 0; assemble = rank 0's scatter of the gathered rows); "
                                        "the timed regions queue steps back to back, so ms_per_step is below their sum")
        if verified is not None:
            out["verified_bit_identical_to_one_context"] = verified
        if dumped is not None:
            out["dump_outputs"] = dumped
        if world == 1 and not args.no_cpu_baseline:
            from oracle import binding as ob
            t0 = time.perf_counter()
            ref = ob.build_scene(sc)   # the reference's BVH / TLAS builder restated (src/bvh/bvh.cpp), one thread
            cpu_build_s = time.perf_counter() - t0
            # probe the host's rate on a small image, then size the sample for ~5-20 s of wall time
            # (the whole workload if the host is fast enough)
            pw, ph = 240, 135
            t0 = time.perf_counter()
            _, _, _, pc, used = ob.render(ref, scenes.camera_block(sc.camera, pw, ph), pw, ph, bounces, spp, 1, accum_mode)
            probe_rate = pc["rays"] / max(time.perf_counter() - t0, 1e-6)
            if args.cpu_sample != "auto":
                sw, sh = (int(x) for x in args.cpu_sample.split("x"))
            else:
                scale = min(1.0, (probe_rate * 15.0 / max(rays, 1)) ** 0.5)
                sw, sh = max(16, int(W * scale) // 16 * 16), max(9, int(H * scale) // 9 * 9)
                if scale >= 1.0:
                    sw, sh = W, H
            scam = scenes.camera_block(sc.camera, sw, sh)
            t0 = time.perf_counter()
            want, _, _, cnt, used = ob.render(ref, scam, sw, sh, bounces, spp, 1, accum_mode)
            dt = time.perf_counter() - t0
            out["cpu_baseline"] = {
                "value": round(cnt["rays"] / dt / 1e6, 3), "unit": "Mrays/s", "cores": used, "kind": "port",
                "bvh_build_s": round(cpu_build_s, 4), "bvh_build_cores": 1,
                "sample": "same scene/camera/seeds at %dx%d, %d spp, %d bounces (%.1f s, %d rays); oracle = C restatement "
                          "of main.glsl over the reference-layout BVH, pthreads" % (sw, sh, spp, bounces, dt, cnt["rays"]),
            }
            # parity: the oracle's image of that sample against the GPU's -- the timed region's own last image when the
            # sample is the whole workload, else one more render of the sample size on the same context
            if (sw, sh) == (W, H):
                got, what = gpu_image, "the image the timed region left behind"
            else:
                ctx.set_params(sw, sh, bounces, accum_mode)
                ctx.set_camera(scam)
                ctx.accum_reset()
                ctx.render(spp, 1)
                got, what = ctx.read_accum(), "a render of the CPU sample's size after the timed region"
                rays_gpu = ctx.stats()["rays"]
                if rays_gpu != cnt["rays"]:
                    what += " (ray segments: GPU %d, oracle %d)" % (rays_gpu, cnt["rays"])
            err = rel_l2(got, want)
            out["parity"] = {
                "rel_l2": err, "differing_pixels": int((got != want).any(axis=-1).sum()), "pixels": int(sw * sh),
                "tolerance": PARITY_TOLERANCE, "ok": bool(err <= PARITY_TOLERANCE),
                "against": "oracle/ (CPU restatement walking the reference-exact tree; parity unpinned: DESIGN.md section 2), %dx%d, %d spp, "
                           "%d bounces; GPU side: %s" % (sw, sh, spp, bounces, what),
            }
            if not err <= PARITY_TOLERANCE:
                status = 3
        print(json.dumps(out))
    ctx.close()
    if use_dist:
        dist.destroy_process_group()
    if status:
        sys.stderr.write("bench.py: parity above tolerance\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
