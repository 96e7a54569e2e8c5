"""Register budgets of the environment-sampling kernels (jpt_set_environment_sampling, JPT_ENV_SAMPLING_MIS; CPU: hipcc
cross-compiles to ISA without a GPU).  wf2_occlude keeps the whole traversal stack in LDS: no scratch at all.  The wf2_shade_mis
instantiations are pinned at what they take, with no scratch: the map sample, its lookup, the BRDF evaluation and the shadow-queue
store cost the two filtered forms one register over wf2_shade_env's 72 (73: still five waves per SIMD under the kernel's launch
bounds), the others none."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_wf2.hip")

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body)
BUDGETS = {
    "13wf2_shade_misILb0ELb0ELi0E": (67, 0, 0),
    "13wf2_shade_misILb0ELb0ELi1E": (73, 0, 0),
    "13wf2_shade_misILb0ELb0ELi2E": (73, 0, 0),
    "13wf2_shade_misILb0ELb1ELi0E": (64, 0, 0),   # the paths' last vertices (no map sample): eight waves, as wf2_shade's
    "11wf2_occludeILb0ELb0EE": (128, 0, 0),
    "11wf2_occludeILb0ELb1EE": (128, 0, 0),
}


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


def usage(isa, kernel):
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0)
    return int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_env_sampling_kernels_keep_their_budgets(isa, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    got = usage(isa, kernel)
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d" % (
        kernel, got[1], got[2], scratch, scratch_ops)
