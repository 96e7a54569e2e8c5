"""Budgets of jpt_bake_finish's kernels (CPU: hipcc cross-compiles jpt_kernels_lightmap.hip to ISA without a GPU, with the compile and
the flags of tests/test_bake_budgets.py), read from the code object's metadata alone: no kernel of the file uses scratch, and the two
staged filter instantiations (halo 2 and halo 4: tile and border of colour and both guides in LDS) stay within 64 KiB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_lightmap.hip")

# mangled-name fragments of the kernels jpt_bake_finish launches; the staged ones: HALO = 2 FIRST, HALO = 4
KERNELS = ("23lightmap_prepare_kernel", "22lightmap_dilate_kernel", "22lightmap_filter_kernelILi2ELb1EE", "22lightmap_filter_kernelILi4ELb0EE",
           "22lightmap_filter_kernelILi0ELb0EE")
STAGED = {"22lightmap_filter_kernelILi2ELb1EE": (32 + 4) * (8 + 4) * 48, "22lightmap_filter_kernelILi4ELb0EE": (32 + 8) * (8 + 8) * 48}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata of the cross-compiled file"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "lightmap.s")
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


def test_every_kernel_of_the_file_is_known_and_uses_no_scratch(metadata):
    assert len(metadata) == len(KERNELS), sorted(metadata)
    for name, use in sorted(metadata.items()):
        assert any(k in name for k in KERNELS), name
        print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                                  use["private_segment_fixed_size"]))
        assert use["private_segment_fixed_size"] == 0, name


@pytest.mark.parametrize("kernel", sorted(STAGED))
def test_the_staged_passes_fit_their_lds(metadata, kernel):
    name = [n for n in metadata if kernel in n]
    assert len(name) == 1, (kernel, sorted(metadata))
    lds = metadata[name[0]]["group_segment_fixed_size"]
    print(kernel, "LDS %d B, vgprs %d" % (lds, metadata[name[0]]["vgpr_count"]))
    assert lds <= 64 * 1024
    assert lds == STAGED[kernel]          # tile + halo, three float4 images: nothing else is staged
    for other, use in metadata.items():
        if not any(k in other for k in STAGED):
            assert use["group_segment_fixed_size"] == 0, other
