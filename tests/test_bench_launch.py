"""bench.py's own launcher: `python bench.py --gpus N` without torch.distributed.run around it starts
the per-GPU processes itself -- as a CHILD process, relaying the one JSON line and the exit status.  Here (no GPU) the ranks
can only fail with bench.py's "needs a GPU" message: what is checked is that they were started, two of them, and that their
failure is ours.  The GPU box runs the real thing (tests/test_gpu_full.py::test_bench_self_launch_two_ranks_on_one_gpu)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_world_size_starts_torchrun_as_a_child():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present: the launch is exercised for real by the gpu-marked test")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode != 0
    assert "needs torch.distributed.run" not in p.stderr            # round 3's refusal is gone
    assert p.stderr.count("bench.py needs a GPU") >= 2, p.stderr[-2000:]   # both ranks ran bench.py's main
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: images that fit are written whole in float32; larger ones are cut to one seeded pixel sample, the same
    for every image and from run to run, with its flat indices, and everything written stays within 64 MB."""
    code = r'''
import sys, json, numpy as np
sys.path.insert(0, %r)
import bench
d = sys.argv[1]
rng = np.random.default_rng(5)
small = {"accum": rng.random((9, 16, 4), dtype=np.float32), "ldr": rng.integers(0, 256, (9, 16, 4)).astype(np.uint8)}
print(json.dumps(bench.dump_outputs(d + "/small", small)))
big = {"accum": rng.random((1080, 1920, 4), dtype=np.float32), "ldr": rng.integers(0, 256, (1080, 1920, 4)).astype(np.uint8)}
np.save(d + "/big_accum_src.npy", big["accum"]); np.save(d + "/big_ldr_src.npy", big["ldr"])
print(json.dumps(bench.dump_outputs(d + "/big", big)))
print(json.dumps(bench.dump_outputs(d + "/big2", big)))
''' % ROOT
    p = subprocess.run([sys.executable, "-c", code, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    import numpy as np
    small, big, big2 = (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))
    assert small["sampled_pixels"] is None and small["files"] == ["accum.npy", "ldr.npy"]
    a = np.load(tmp_path / "small" / "accum.npy")
    ldr = np.load(tmp_path / "small" / "ldr.npy")
    assert a.dtype == np.float32 and a.shape == (9, 16, 4) and ldr.dtype == np.float32 and ldr.shape == (9, 16, 4)
    assert big["sampled_pixels"] and big["files"] == ["accum.npy", "ldr.npy", "pixel_index.npy"]
    total = sum(os.path.getsize(tmp_path / "big" / f) for f in big["files"])
    assert big["bytes"] <= 64_000_000 and total <= 64_000_000
    idx = np.load(tmp_path / "big" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < 1080 * 1920
    k = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "big" / "accum.npy"), np.load(tmp_path / "big_accum_src.npy").reshape(-1, 4)[k])
    assert np.array_equal(np.load(tmp_path / "big" / "ldr.npy"), np.load(tmp_path / "big_ldr_src.npy").reshape(-1, 4)[k].astype(np.float32))
    for f in big["files"]:
        assert np.array_equal(np.load(tmp_path / "big" / f), np.load(tmp_path / "big2" / f))
