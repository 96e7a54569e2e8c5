"""Budgets of the kernels of jpt_set_variance and jpt_noise_estimate (CPU: hipcc cross-compiles jpt_kernels_variance.hip to ISA without a
GPU, with the compile and the flags of tests/test_bake_dir_budgets.py), read from the code object's metadata alone: the file holds
three kernels; the moment kernel uses no scratch and no LDS and its registers leave eight waves per SIMD, the estimate keeps its bins
in at most 2 KB of LDS, and none of them spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_variance.hip")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata of the cross-compiled file"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the library itself could not have been built"
    out = str(tmp_path_factory.mktemp("isa") / "variance.s")
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


def one(metadata, word):
    found = [(n, u) for n, u in metadata.items() if word in n]
    assert len(found) == 1, (word, sorted(metadata))
    name, use = found[0]
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                              use["private_segment_fixed_size"]))
    return use


def test_the_file_holds_three_kernels(metadata):
    assert len(metadata) == 3, sorted(metadata)


def test_the_moment_kernel_uses_no_scratch_and_no_lds(metadata):
    use = one(metadata, "16variance_moments")
    assert use["private_segment_fixed_size"] == 0
    assert use["group_segment_fixed_size"] == 0
    assert use["vgpr_count"] <= 64          # 512 VGPRs per SIMD lane / 64: eight waves per SIMD


def test_the_estimate_kernel_keeps_its_bins_in_two_kb_of_lds(metadata):
    use = one(metadata, "21noise_estimate_kernel")
    assert use["private_segment_fixed_size"] == 0
    assert 0 < use["group_segment_fixed_size"] <= 2048
    assert use["vgpr_count"] <= 64


def test_the_resolve_uses_no_scratch(metadata):
    use = one(metadata, "20noise_resolve_kernel")
    assert use["private_segment_fixed_size"] == 0
