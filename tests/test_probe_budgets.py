"""Register budgets of the probe forms of the bounce-0 kernels (jpt_set_probes; CPU: hipcc cross-compiles to ISA without a GPU), with
the compile, the flags and the parsing of tests/test_bake_budgets.py: wf2_primary_probe and wf2_primary_env_probe exist in every COUNT
/ W4 / TAIL instantiation the pinhole kernels have and take the probes where the pinhole takes the sky cull; the instantiations a
render of the benchmark scenes launches use no more VGPRs than the pinhole kernel of the same instantiation READ FROM THE SAME ISA (the
same waves per SIMD; nothing is hard-coded), and no more scratch than the lens kernels' budgets (tests/test_lens_budgets.py).  And of
jpt_kernels_probe.hip, from its own ISA: the projection kernel uses no scratch and an LDS size that admits its four waves."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc")

# instantiation -> (most bytes of scratch per lane, most scratch instructions in the body): the lens kernels' budgets
SCRATCH = {"ILb0ELb1ELb0E": (320, 14), "ILb0ELb1ELb1E": (1100, 96)}
INSTANCES = ("ILb0ELb0ELb0E", "ILb0ELb1ELb0E", "ILb0ELb1ELb1E", "ILb1ELb0ELb0E", "ILb1ELb1ELb0E", "ILb1ELb1ELb1E")
PINHOLE = {"17wf2_primary_probe": "11wf2_primary", "21wf2_primary_env_probe": "15wf2_primary_env"}


def compile_isa(tmp_path_factory, source, stem):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / (stem + ".s"))
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_wf2.hip", "wf2")


@pytest.fixture(scope="module")
def probe_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_probe.hip", "probe")


def usage(isa, kernel):
    """(VGPRs, bytes of scratch per lane, scratch instructions in the body) of the kernel whose mangled name holds `kernel`"""
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    return int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))


def test_the_probe_kernels_exist_in_every_instantiation(isa):
    for name in ("17wf2_primary_probe", "21wf2_primary_env_probe", "11wf2_primary", "15wf2_primary_env"):
        for inst in INSTANCES:
            assert re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + name + inst, isa), name + inst
    # and they take the probes where the pinhole kernels take the sky cull
    for name in PINHOLE:
        for inst in INSTANCES:
            assert re.search(name + inst + r"\S*8ProbeDev", isa) and not re.search(name + inst + r"\S*7SkyCull", isa), name + inst
    assert re.search(r"11wf2_primaryILb0ELb1ELb0E\S*7SkyCull", isa)


@pytest.mark.parametrize("inst", sorted(SCRATCH))
@pytest.mark.parametrize("kernel", sorted(PINHOLE))
def test_probe_kernels_keep_the_pinhole_kernels_waves(isa, kernel, inst):
    scratch, scratch_ops = SCRATCH[inst]
    got, pinhole = usage(isa, kernel + inst), usage(isa, PINHOLE[kernel] + inst)
    print(kernel + inst, "vgprs %d scratch %d B scratch instructions %d" % got, "-- pinhole: vgprs %d scratch %d B scratch instructions %d" % pinhole)
    assert got[0] <= pinhole[0], "%s: %d VGPRs, the pinhole kernel of the same ISA has %d (a wave per SIMD less)" % (kernel + inst, got[0], pinhole[0])
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d (spills?)" % (
        kernel + inst, got[1], got[2], scratch, scratch_ops)


def test_the_projection_kernel_uses_no_scratch_and_its_lds_admits_four_waves(probe_isa):
    text = probe_isa[probe_isa.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - (?=\.)", text)[1:]
    assert len(entries) == 1, len(entries)                     # one kernel in the file
    name = re.search(r"\.name:\s+(\S+)", entries[0]).group(1)
    assert "20probe_project_kernel" in name, name
    use = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|max_flat_workgroup_size):\s+(\d+)", entries[0])}
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                              use["private_segment_fixed_size"]))
    assert use["private_segment_fixed_size"] == 0
    body = re.search(r"\n" + re.escape(name) + r":.*?s_endpgm", probe_isa, re.S).group(0)
    assert not re.search(r"\bscratch_(?:load|store)", body)
    assert use["max_flat_workgroup_size"] == 256               # four waves: four probes per block
    assert use["group_segment_fixed_size"] == 1024 * 9 * 4     # the table of the largest tile, nothing else: 36 KB of a block's 64 KiB
    assert use["group_segment_fixed_size"] <= 64 * 1024
    assert use["vgpr_count"] <= 128                            # (four waves of 256 threads fit a SIMD's registers with room to spare)
