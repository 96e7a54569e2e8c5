"""Register budgets of the lens forms of the bounce-0 kernels (jpt_set_lens; CPU: hipcc cross-compiles to ISA without a GPU), with the
compile and the flags of tests/test_register_budgets.py: wf2_primary_lens and wf2_primary_env_lens exist in every COUNT / W4 / TAIL
instantiation the pinhole kernels have, and the ones a render of the benchmark scenes launches keep the pinhole kernels' budgets
 -- seven waves per SIMD, the stack's scratch and nothing more."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_wf2.hip")

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body): wf2_primary's
BUDGETS = {
    "16wf2_primary_lensILb0ELb1ELb0E": (72, 320, 14),
    "16wf2_primary_lensILb0ELb1ELb1E": (72, 1100, 96),      # (TAIL: 944 B and 92 instructions reached, the lens words live across the out-of-line call)
    "20wf2_primary_env_lensILb0ELb1ELb0E": (72, 320, 14),
    "20wf2_primary_env_lensILb0ELb1ELb1E": (72, 1100, 96),
}
INSTANCES = ("ILb0ELb0ELb0E", "ILb0ELb1ELb0E", "ILb0ELb1ELb1E", "ILb1ELb0ELb0E", "ILb1ELb1ELb0E", "ILb1ELb1ELb1E")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "wf2.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


def test_the_lens_kernels_exist_in_every_instantiation(isa):
    for name in ("16wf2_primary_lens", "20wf2_primary_env_lens", "11wf2_primary", "15wf2_primary_env"):
        for inst in INSTANCES:
            assert re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + name + inst, isa), name + inst
    # and they take the lens where the pinhole kernels take the sky cull
    assert re.search(r"16wf2_primary_lensILb0ELb1ELb0E\S*7LensDev", isa) and not re.search(r"16wf2_primary_lensILb0ELb1ELb0E\S*7SkyCull", isa)


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_lens_kernels_keep_the_pinhole_budgets(isa, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    got = (int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body)))
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d (a wave per SIMD less)" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d (spills?)" % (
        kernel, got[1], got[2], scratch, scratch_ops)
