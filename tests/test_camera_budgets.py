"""Register budgets of the camera-model forms of the kernels (jpt_set_camera_model; CPU: hipcc cross-compiles to ISA without a GPU),
from the ISA dump of tests/test_register_budgets.py (its fixture, its compile, its flags): wf2_primary_cam and wf2_primary_env_cam
exist in every COUNT / W4 / TAIL instantiation the pinhole kernels have, the ones a render of the benchmark scenes launches stay within
the VGPR step of their launch bound (72: seven waves per SIMD, the lens forms' step) with the scratch the build gave when they were
written, and guide_cam_kernel and query_pixel_rays_cam use no scratch."""
import os
import re
import shutil
import subprocess

import pytest

from test_register_budgets import isa  # noqa: F401  (the module-scoped fixture: jpt_kernels_wf2.hip compiled to gfx950 assembly)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel (mangled-name fragment) -> (most VGPRs, most bytes of scratch per lane, most scratch instructions in the body): the figures of
# the build, beside the lens forms' (72, 320, 13 / 11) and (72, 944, 94 / 92) from the same dump
BUDGETS = {
    "15wf2_primary_camILb0ELb1ELb0E": (72, 320, 11),
    "15wf2_primary_camILb0ELb1ELb1E": (72, 944, 82),       # (TAIL: the out-of-line cooperative walk behind the loop)
    "19wf2_primary_env_camILb0ELb1ELb0E": (72, 320, 11),
    "19wf2_primary_env_camILb0ELb1ELb1E": (72, 944, 74),
}
INSTANCES = ("ILb0ELb0ELb0E", "ILb0ELb1ELb0E", "ILb0ELb1ELb1E", "ILb1ELb0ELb0E", "ILb1ELb1ELb0E", "ILb1ELb1ELb1E")
NO_SCRATCH = {"jpt_kernels_denoise.hip": ("16guide_cam_kernelILb1EE", "16guide_cam_kernelILb0EE"), "jpt_kernels_query.hip": ("20query_pixel_rays_camE",)}


def figures(text, kernel):
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", text, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    body = re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", text, re.S).group(0)
    return int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", body))


def test_the_camera_kernels_exist_in_every_instantiation(isa):  # noqa: F811
    for name in ("15wf2_primary_cam", "19wf2_primary_env_cam", "11wf2_primary", "15wf2_primary_env"):
        for inst in INSTANCES:
            assert re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + name + inst, isa), name + inst
    # and they take the model where the pinhole kernels take the sky cull
    assert re.search(r"15wf2_primary_camILb0ELb1ELb0E\S*11CamModelDev", isa) and not re.search(r"15wf2_primary_camILb0ELb1ELb0E\S*7SkyCull", isa)


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_camera_kernels_stay_within_their_vgpr_step_and_pinned_scratch(isa, kernel):  # noqa: F811
    vgprs, scratch, scratch_ops = BUDGETS[kernel]
    got = figures(isa, kernel)
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs, "%s: %d VGPRs, budget %d (a wave per SIMD less)" % (kernel, got[0], vgprs)
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, pinned at %d / %d (spills?)" % (
        kernel, got[1], got[2], scratch, scratch_ops)


@pytest.mark.parametrize("source", sorted(NO_SCRATCH))
def test_guide_and_picking_forms_use_no_scratch(tmp_path, source):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path / "out.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "gdpathtracing_amd", "csrc", source)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    text = open(out).read()
    for kernel in NO_SCRATCH[source]:
        got = figures(text, kernel)
        print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
        assert got[1] == 0 and got[2] == 0, "%s: scratch %d B / %d instructions" % (kernel, got[1], got[2])
