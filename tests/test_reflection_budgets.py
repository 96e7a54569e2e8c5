"""Register budgets of the cube forms of the bounce-0 kernels (jpt_set_reflection_probes; CPU: hipcc cross-compiles to ISA without a
GPU), with the compile, the flags and the parsing of tests/test_probe_budgets.py: wf2_primary_cube and wf2_primary_env_cube exist in
every COUNT / W4 / TAIL instantiation the pinhole kernels have and take the reflection probes where the pinhole takes the sky cull; the
instantiations a render of the benchmark scenes launches use no more VGPRs than the pinhole kernel of the same instantiation READ FROM
THE SAME ISA (the same waves per SIMD; nothing is hard-coded), and no more scratch than the lens kernels' budgets
(tests/test_lens_budgets.py).  And of jpt_kernels_reflection.hip, from its own ISA: the chain and prefilter kernels use no scratch, and
the prefilter's LDS and registers admit at least four waves per SIMD."""
import re

import pytest

from test_probe_budgets import INSTANCES, SCRATCH, compile_isa, usage

PINHOLE = {"16wf2_primary_cube": "11wf2_primary", "20wf2_primary_env_cube": "15wf2_primary_env"}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_wf2.hip", "wf2")


@pytest.fixture(scope="module")
def refl_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory, "jpt_kernels_reflection.hip", "reflection")


def test_the_cube_kernels_exist_in_every_instantiation(isa):
    for name in list(PINHOLE) + list(PINHOLE.values()):
        for inst in INSTANCES:
            assert re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + name + inst, isa), name + inst
    # and they take the reflection probes where the pinhole kernels take the sky cull
    for name in PINHOLE:
        for inst in INSTANCES:
            assert re.search(name + inst + r"\S*7CubeDev", isa) and not re.search(name + inst + r"\S*7SkyCull", isa), name + inst
    assert re.search(r"11wf2_primaryILb0ELb1ELb0E\S*7SkyCull", isa)


@pytest.mark.parametrize("inst", sorted(SCRATCH))
@pytest.mark.parametrize("kernel", sorted(PINHOLE))
def test_cube_kernels_keep_the_pinhole_kernels_waves(isa, kernel, inst):
    scratch, scratch_ops = SCRATCH[inst]
    got, pinhole = usage(isa, kernel + inst), usage(isa, PINHOLE[kernel] + inst)
    print(kernel + inst, "vgprs %d scratch %d B scratch instructions %d" % got, "-- pinhole: vgprs %d scratch %d B scratch instructions %d" % pinhole)
    assert got[0] <= pinhole[0], "%s: %d VGPRs, the pinhole kernel of the same ISA has %d (a wave per SIMD less)" % (kernel + inst, got[0], pinhole[0])
    assert got[1] <= scratch and got[2] <= scratch_ops, "%s: scratch %d B / %d instructions, budget %d / %d (spills?)" % (
        kernel + inst, got[1], got[2], scratch, scratch_ops)


def test_the_chain_and_prefilter_kernels_use_no_scratch_and_the_prefilter_admits_four_waves(refl_isa):
    text = refl_isa[refl_isa.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - (?=\.)", text)[1:]
    assert len(entries) == 2, len(entries)                     # two kernels in the file
    seen = {}
    for entry in entries:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        use = {f: int(v) for f, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|max_flat_workgroup_size):\s+(\d+)", entry)}
        print("%s: vgprs %d, sgprs %d, LDS %d B, scratch %d B" % (name, use["vgpr_count"], use["sgpr_count"], use["group_segment_fixed_size"],
                                                                  use["private_segment_fixed_size"]))
        assert use["private_segment_fixed_size"] == 0, name
        body = re.search(r"\n" + re.escape(name) + r":.*?s_endpgm", refl_isa, re.S).group(0)
        assert not re.search(r"\bscratch_(?:load|store)", body), name
        assert use["max_flat_workgroup_size"] == 256, name
        seen["chain" if "17refl_chain_kernel" in name else "prefilter" if "21refl_prefilter_kernel" in name else name] = use
    assert sorted(seen) == ["chain", "prefilter"], sorted(seen)
    assert seen["chain"]["group_segment_fixed_size"] == 0
    pre = seen["prefilter"]
    # the level's table, nothing else: 256 entries of 16 B and 256 level bytes.  Four waves per SIMD are 16 per CU, four blocks of 256
    # threads: their LDS must fit a CU's 160 KiB, and 512 VGPRs per SIMD lane shared by four waves are 128 each
    assert pre["group_segment_fixed_size"] == 256 * 16 + 256
    assert 4 * pre["group_segment_fixed_size"] <= 160 * 1024
    assert pre["vgpr_count"] <= 128
