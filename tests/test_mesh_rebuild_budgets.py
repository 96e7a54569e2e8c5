"""Budgets of the kernels of jpt_scene_rebuild_mesh (CPU: hipcc cross-compiles to ISA without a GPU), from the kernel metadata alone:
the order kernels and the three kernels of a sort pass exist, none uses scratch, and the LDS of each is what its arrays add up to.  The
VGPR counts are printed (DESIGN.md section 4 states them)."""
import os
import shutil
import subprocess

import pytest

from test_tlas_rebuild_budgets import metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_mesh_rebuild.hip")
WAVES = 4   # kMeshSortWaves: a block of 256 threads
KERNELS = {
    "_ZN3jpt22mesh_order_init_kernelE": 0,
    "_ZN3jpt25mesh_centre_bounds_kernelE": WAVES * 6 * 4,                 # the waves' bounds
    "_ZN3jpt17mesh_codes_kernelE": 0,
    "_ZN3jpt21mesh_sort_hist_kernelE": 256 * 4,                           # the digits' counts
    "_ZN3jpt21mesh_sort_scan_kernelE": 16 * 4,                            # the sixteen waves' totals
    "_ZN3jpt24mesh_sort_scatter_kernelE": 256 * 4 + 2 * WAVES * 256 * 4,  # the digits' next positions; counts and offsets per wave
    "_ZN3jpt21mesh_root_word_kernelE": 0,
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc in this environment"
    out = str(tmp_path_factory.mktemp("isa") / "mesh_rebuild.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_rebuild_kernels_use_no_scratch_and_the_lds_they_declare(isa, name):
    lds, scratch, vgprs = metadata(isa, name)
    print("%s: vgprs %d, scratch %d B, LDS %d B" % (name, vgprs, scratch, lds))
    assert scratch == 0, "%s: .private_segment_fixed_size %d" % (name, scratch)
    assert KERNELS[name] <= lds <= KERNELS[name] + 64   # (the arrays, plus at most their alignment padding)
