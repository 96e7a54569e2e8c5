"""Budgets of the kernels of jpt_scene_rebuild_tlas (CPU: hipcc cross-compiles to ISA without a GPU), from the kernel metadata alone:
the order kernel in both instantiations (keys in LDS / in device memory), the template kernel and the tail copy exist, none uses
scratch, and the LDS of the order kernel is what its arrays add up to -- under the 64 KiB a block gets without asking.  The VGPR counts
are printed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_tlas.hip")
# bounds (6 words) + digit positions (256 words) + wave totals (4 words) + counts and offsets (16 waves x 256 digits x 2 B each)
ORDER_LDS_FIXED = 6 * 4 + 256 * 4 + 4 * 4 + 2 * 16 * 256 * 2
LDS_KEYS = 2048   # kTlasLdsKeys: two buffers of 8-byte keys
KERNELS = {
    "_ZN3jpt17tlas_order_kernelILb1EE": (ORDER_LDS_FIXED + 2 * LDS_KEYS * 8, ORDER_LDS_FIXED + 2 * LDS_KEYS * 8 + 64),
    "_ZN3jpt17tlas_order_kernelILb0EE": (ORDER_LDS_FIXED, ORDER_LDS_FIXED + 64),
    "_ZN3jpt20tlas_template_kernelE": (0, 0),
    "_ZN3jpt21tlas_tail_copy_kernelE": (0, 0),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc in this environment"
    out = str(tmp_path_factory.mktemp("isa") / "tlas.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


def metadata(isa, name):
    """(LDS bytes, scratch bytes per lane, VGPRs) of the kernel, from its metadata record (the fields of a record are sorted by name:
    the LDS size precedes .name, the scratch size and the VGPR count follow it)"""
    at = isa.find(".name:           " + name)
    assert at >= 0, "kernel not found in the ISA: " + name

    def field(key, text):
        return int(re.search(r"\." + key + r":\s+(\d+)", text).group(1))
    before, after = isa[max(0, at - 400):at], isa[at:at + 1200]
    return (field("group_segment_fixed_size", before[before.rfind(".group_segment_fixed_size"):]), field("private_segment_fixed_size", after),
            field("vgpr_count", after))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_rebuild_kernels_use_no_scratch_and_the_lds_they_declare(isa, name):
    lds, scratch, vgprs = metadata(isa, name)
    print("%s: vgprs %d, scratch %d B, LDS %d B" % (name, vgprs, scratch, lds))
    assert scratch == 0, "%s: .private_segment_fixed_size %d" % (name, scratch)
    least, most = KERNELS[name]   # (the arrays, plus at most their alignment padding)
    assert least <= lds <= most
    assert lds <= 64 * 1024
