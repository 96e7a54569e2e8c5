"""Budgets of the kernels of jpt_denoise's history stage (CPU: hipcc cross-compiles jpt_kernels_denoise_history.hip to ISA without a
GPU, with the compile and the flags of tests/test_denoise_var_budgets.py), read from the code object's metadata alone: three kernels,
none with scratch; the two forms of the first filter pass over a pre-formed (i, v) image keep eight waves per SIMD and the LDS of
atrous_var_kernel<2, ...>, whose shape they share; history_kernel is held at the registers measured when it was written and its LDS is
the three staged tiles (and the word __syncthreads_or votes through)."""
import pytest

from test_denoise_var_budgets import compile_metadata, one

HISTORY_VGPRS = 52                    # as measured when history_kernel was written
TILES = 3 * (32 + 4) * (8 + 4) * 16   # (c, X, n) of the 32 x 8 tile and its 2-pixel halo, 16 B each
VOTE = 256                            # what the compiler sets aside for the block-wide vote
PRE = {"21atrous_var_pre_kernelILb1EE": "17atrous_var_kernelILi2ELb1ELb1EE", "21atrous_var_pre_kernelILb0EE": "17atrous_var_kernelILi2ELb1ELb0EE"}


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    return compile_metadata(tmp_path_factory.mktemp("isa"), "jpt_kernels_denoise_history.hip")


@pytest.fixture(scope="module")
def guided(tmp_path_factory):
    return compile_metadata(tmp_path_factory.mktemp("isa"), "jpt_kernels_denoise_var.hip")


def test_the_file_holds_three_kernels_and_none_uses_scratch(stage):
    assert len(stage) == 3, sorted(stage)
    for word in ["14history_kernel"] + list(PRE):
        assert one(stage, word)["private_segment_fixed_size"] == 0, word


@pytest.mark.parametrize("kernel", sorted(PRE))
def test_the_first_pass_keeps_eight_waves_and_the_lds_of_the_guided_one(stage, guided, kernel):
    use, before = one(stage, kernel), one(guided, PRE[kernel])
    assert use["vgpr_count"] <= 64          # 512 VGPRs per SIMD lane / 64: eight waves per SIMD
    assert 0 < use["group_segment_fixed_size"] <= before["group_segment_fixed_size"]


def test_history_kernel_keeps_its_registers_and_stages_three_tiles(stage):
    use = one(stage, "14history_kernel")
    assert use["vgpr_count"] <= 128 and use["vgpr_count"] <= HISTORY_VGPRS
    assert TILES <= use["group_segment_fixed_size"] <= TILES + VOTE
