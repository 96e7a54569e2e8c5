"""Budgets of the kernels of the variance-guided jpt_denoise (CPU: hipcc cross-compiles jpt_kernels_denoise_var.hip to ISA without a GPU,
with the compile and the flags of tests/test_variance_budgets.py), read from the code object's metadata alone: six instantiations of one
kernel, none with scratch; the tiled ones keep eight waves per SIMD and no more LDS than the tiled atrous_kernel of the same halo (the
variance travels in the colour's .w: no fourth tile); the gathered ones are held at the registers measured."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc")

# the gathered instantiations (HALO 0; LAST, not LAST): VGPRs as measured when they were written
GATHER_VGPRS = {"17atrous_var_kernelILi0ELb0ELb1EE": 54, "17atrous_var_kernelILi0ELb0ELb0EE": 52}
TILED = {"17atrous_var_kernelILi2ELb1ELb1EE": "13atrous_kernelILi2ELb1ELb1EE", "17atrous_var_kernelILi2ELb1ELb0EE": "13atrous_kernelILi2ELb1ELb0EE",
         "17atrous_var_kernelILi4ELb0ELb1EE": "13atrous_kernelILi4ELb0ELb1EE", "17atrous_var_kernelILi4ELb0ELb0EE": "13atrous_kernelILi4ELb0ELb0EE"}


def compile_metadata(tmp, source):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata of the cross-compiled file"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the library itself could not have been built"
    out = str(tmp / (source + ".s"))
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    text = open(out).read()
    text = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", entry)}
    return kernels


@pytest.fixture(scope="module")
def guided(tmp_path_factory):
    return compile_metadata(tmp_path_factory.mktemp("isa"), "jpt_kernels_denoise_var.hip")


@pytest.fixture(scope="module")
def unguided(tmp_path_factory):
    return compile_metadata(tmp_path_factory.mktemp("isa"), "jpt_kernels_denoise.hip")


def one(metadata, word):
    found = [(n, u) for n, u in metadata.items() if word in n]
    assert len(found) == 1, (word, sorted(metadata))
    name, use = found[0]
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                              use["private_segment_fixed_size"]))
    return use


def test_the_file_holds_the_six_instantiations_and_none_uses_scratch(guided):
    assert len(guided) == 6 and all("17atrous_var_kernel" in n for n in guided), sorted(guided)
    for word in list(TILED) + list(GATHER_VGPRS):
        assert one(guided, word)["private_segment_fixed_size"] == 0, word


@pytest.mark.parametrize("kernel", sorted(TILED))
def test_a_tiled_pass_keeps_eight_waves_and_the_lds_of_the_unguided_one(guided, unguided, kernel):
    use, before = one(guided, kernel), one(unguided, TILED[kernel])
    assert use["vgpr_count"] <= 64          # 512 VGPRs per SIMD lane / 64: eight waves per SIMD
    assert 0 < use["group_segment_fixed_size"] <= before["group_segment_fixed_size"]


@pytest.mark.parametrize("kernel", sorted(GATHER_VGPRS))
def test_a_gathered_pass_keeps_its_registers_and_uses_no_lds(guided, kernel):
    use = one(guided, kernel)
    assert use["vgpr_count"] <= GATHER_VGPRS[kernel]
    assert use["group_segment_fixed_size"] == 0
