"""Budgets of the skin kernel (jpt_scene_pose_mesh; CPU: hipcc cross-compiles to ISA without a GPU), from the kernel metadata alone:
mesh_skin_kernel exists in every instantiation the launcher picks from (influences 0 / 4 / 8), none of them uses scratch or LDS.  The
VGPR counts are printed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_skin.hip")
# <influences>
INSTANCES = ("ILi0EE", "ILi4EE", "ILi8EE")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "skin.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


def metadata(isa, inst):
    """(LDS bytes, scratch bytes per lane, VGPRs) of mesh_skin_kernel<inst>, from its metadata record (the fields of a record are
    sorted by name: the LDS size precedes .name, the scratch size and the VGPR count follow it)"""
    at = isa.find(".name:           _ZN3jpt12_GLOBAL__N_116mesh_skin_kernel" + inst)
    assert at >= 0, "kernel not found in the ISA: mesh_skin_kernel" + inst

    def field(name, text):
        return int(re.search(r"\." + name + r":\s+(\d+)", text).group(1))
    before, after = isa[max(0, at - 400):at], isa[at:at + 1200]
    return (field("group_segment_fixed_size", before[before.rfind(".group_segment_fixed_size"):]), field("private_segment_fixed_size", after),
            field("vgpr_count", after))


@pytest.mark.parametrize("inst", INSTANCES)
def test_skin_kernel_uses_no_scratch(isa, inst):
    lds, scratch, vgprs = metadata(isa, inst)
    print("mesh_skin_kernel%s: vgprs %d, scratch %d B, LDS %d B" % (inst, vgprs, scratch, lds))
    assert scratch == 0, "mesh_skin_kernel%s: .private_segment_fixed_size %d" % (inst, scratch)
    assert lds == 0
