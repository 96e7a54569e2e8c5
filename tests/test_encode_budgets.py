"""Budgets of jpt_encode's kernel (jpt_kernels_encode.hip; CPU: hipcc cross-compiles to ISA without a GPU), with the compile and the
flags of tests/test_probe_budgets.py: the three instantiations of the one streaming kernel use no scratch and no LDS, few enough VGPRs
for eight waves per SIMD, and move their texels with 16-byte loads and 16-byte stores."""
import re

import pytest

from test_probe_budgets import compile_isa

KERNELS = {"ILi1E": "RGBA16F", "ILi2E": "RGB9E5", "ILi3E": "RGBE8"}      # encode_kernel<JPT_ENCODE_*>
TEXELS_PER_THREAD = {"RGBA16F": 2, "RGB9E5": 4, "RGBE8": 4}               # of the vector path: one 16-byte store


@pytest.fixture(scope="module")
def encode_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_encode.hip", "encode")


def kernels(isa):
    """{format name: (mangled name, the metadata fields, the body)} of every kernel in the file"""
    text = isa[isa.index("amdhsa.kernels:"):]
    found = {}
    for entry in re.split(r"\n  - (?=\.)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        use = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|max_flat_workgroup_size):\s+(\d+)", entry)}
        body = re.search(r"\n" + re.escape(name) + r":.*?s_endpgm", isa, re.S).group(0)
        m = re.search(r"13encode_kernel(ILi\dE)", name)
        found[KERNELS[m.group(1)] if m else name] = (name, use, body)
    return found


def test_one_kernel_per_format_and_nothing_else(encode_isa):
    assert sorted(kernels(encode_isa)) == sorted(KERNELS.values())


@pytest.mark.parametrize("fmt", sorted(KERNELS.values()))
def test_no_scratch_no_lds_and_eight_waves_of_registers(encode_isa, fmt):
    name, use, body = kernels(encode_isa)[fmt]
    print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                              use["private_segment_fixed_size"]))
    assert use["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_(?:load|store)", body)
    assert use["group_segment_fixed_size"] == 0 and not re.search(r"\bds_(?:read|write|load|store)", body)
    assert not re.search(r"\b(?:global|flat|buffer|ds)_atomic", body)
    assert use["max_flat_workgroup_size"] == 256
    assert use["vgpr_count"] <= 64                              # 512 per SIMD lane shared by eight waves


@pytest.mark.parametrize("fmt", sorted(KERNELS.values()))
def test_the_texels_move_in_16_byte_loads_and_stores(encode_isa, fmt):
    _, _, body = kernels(encode_isa)[fmt]
    loads = re.findall(r"\b((?:global|flat|buffer)_load_\w+)", body)
    stores = re.findall(r"\b((?:global|flat|buffer)_store_\w+)", body)
    print(fmt, "loads", sorted(set(loads)), len(loads), "stores", sorted(set(stores)), len(stores))
    per = TEXELS_PER_THREAD[fmt]
    # every texel is read as one 16-byte load: those of the vector path and the one of the tail's loop
    assert set(loads) == {"global_load_dwordx4"} and len(loads) == per + 1, loads
    # the vector path writes one 16-byte store; the only other store is the tail's, one texel wide
    tail = "global_store_dwordx2" if fmt == "RGBA16F" else "global_store_dword"
    assert sorted(stores) == sorted(["global_store_dwordx4", tail]), stores
