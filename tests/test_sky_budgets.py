"""Budgets of jpt_set_sky's kernel (jpt_kernels_sky.hip; CPU: hipcc cross-compiles to ISA without a GPU), with the compile and the flags
of tests/test_probe_budgets.py: one streaming ALU kernel that reads nothing from global memory -- its parameter block arrives with
scalar loads from the kernel-argument segment --, uses no scratch, no LDS and no atomics, and writes each texel with one 16-byte store."""
import re

import pytest

from test_probe_budgets import compile_isa


@pytest.fixture(scope="module")
def sky_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_sky.hip", "sky")


def kernels(isa):
    """[(mangled name, the metadata fields, the body)] of every kernel in the file"""
    text = isa[isa.index("amdhsa.kernels:"):]
    found = []
    for entry in re.split(r"\n  - (?=\.)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        use = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|max_flat_workgroup_size):\s+(\d+)", entry)}
        body = re.search(r"\n" + re.escape(name) + r":.*?s_endpgm", isa, re.S).group(0)
        found.append((name, use, body))
    return found


def test_one_kernel_within_its_budgets(sky_isa):
    found = kernels(sky_isa)
    assert len(found) == 1 and "sky_kernel" in found[0][0], [k[0] for k in found]
    name, use, body = found[0]
    valu, salu = len(re.findall(r"\n\s+v_\w+", body)), len(re.findall(r"\n\s+s_\w+", body))
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B, %d vector and %d scalar instructions" % (
        name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"], use["private_segment_fixed_size"], valu, salu))
    assert use["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_(?:load|store)", body)
    assert use["group_segment_fixed_size"] == 0 and not re.search(r"\bds_(?:read|write|load|store)", body)
    assert not re.search(r"\b(?:global|flat|buffer|ds)_atomic", body)
    assert use["max_flat_workgroup_size"] == 256
    assert use["vgpr_count"] <= 128               # no memory latency to hide: four waves per SIMD are ample


def test_nothing_is_loaded_and_every_texel_leaves_as_one_16_byte_store(sky_isa):
    _, _, body = kernels(sky_isa)[0]
    loads = re.findall(r"\b((?:global|flat|buffer)_load_\w+)", body)
    stores = re.findall(r"\b((?:global|flat|buffer)_store_\w+)", body)
    print("loads", loads, "stores", stores)
    assert loads == []
    assert stores == ["global_store_dwordx4"]
