"""Budgets of the moment kernel of jpt_set_bake_directional (CPU: hipcc cross-compiles jpt_kernels_bake_dir.hip to ISA without a GPU,
with the compile and the flags of tests/test_lightmap_budgets.py), read from the code object's metadata alone: the file holds one
kernel, it uses no scratch and no LDS, and its registers leave eight waves per SIMD (53 VGPRs)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_bake_dir.hip")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata of the cross-compiled file"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the library itself could not have been built"
    out = str(tmp_path_factory.mktemp("isa") / "bake_dir.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    text = open(out).read()
    text = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", entry)}
    return kernels


def test_the_moment_kernel_uses_no_scratch_and_no_lds(metadata):
    assert len(metadata) == 1, sorted(metadata)
    (name, use), = metadata.items()
    assert "12bake_moments" in name, name
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                              use["private_segment_fixed_size"]))
    assert use["private_segment_fixed_size"] == 0
    assert use["group_segment_fixed_size"] == 0
    assert use["vgpr_count"] <= 64          # 512 VGPRs per SIMD lane / 64: eight waves per SIMD
