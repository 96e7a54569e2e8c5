"""Register budgets of the environment-map kernels (jpt_set_environment; CPU: hipcc cross-compiles to ISA without a GPU).  The
*_env instantiations of wf2_primary and wf2_shade must fit the budgets tests/test_register_budgets.py pins for their default
siblings: a render with a map must not lose a wave per SIMD, nor put scratch traffic into the walk.  wf2_primary_env queues its
misses for wf2_shade_env instead of looking them up itself (jpt_wf2_paths.h): the lookup inlined there cost the walk spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_wf2.hip")

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body): the
# default siblings' budgets
BUDGETS = {
    "15wf2_primary_envILb0ELb1ELb0E": (72, 320, 14),
    "15wf2_primary_envILb0ELb1ELb1E": (72, 1100, 90),
    "13wf2_shade_envILb0ELb0ELi0E": (72, 0, 0),
    "13wf2_shade_envILb0ELb0ELi1E": (72, 0, 0),
    "13wf2_shade_envILb0ELb0ELi2E": (72, 0, 0),
    "13wf2_shade_envILb0ELb1ELi0E": (64, 0, 0),
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
def test_environment_kernels_keep_their_siblings_budgets(isa, kernel):
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    got = usage(isa, kernel)
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d (a wave per SIMD less)" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d (spills?)" % (
        kernel, got[1], got[2], scratch, scratch_ops)


def test_the_accumulation_with_a_map_has_no_scratch(isa):
    assert usage(isa, "18wf2_accumulate_env")[1:] == (0, 0)
