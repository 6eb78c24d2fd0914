"""GPU: the one-launch recurrent middle of the causal block (aum_stream_block_tm) on the device library -- bit equality with the three
launches it replaces, the partition property, the fp64 oracle, AUM_STREAM_NO_COMMIT, the refusals, and Mamba.step_chunk /
AudioMamba streaming with the fused path on against off (tests/stream_block_checks.py).  On the commit before the feature every test
here fails at the missing symbol / AttributeError."""
import pytest
import torch

import aum_hip
import stream_block_checks as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_T = bc.MAX_T


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", ["small", "base"])
def test_fused_equals_three_launches_bitwise(shape, dt, lib):
    for T in (1, 8, 9, 16, 17, 33, MAX_T):
        bc.check_fused_equals_three(shape, dt, (T,), (0,), 2, lib, DEV)
    bc.check_fused_equals_three(shape, dt, (3, 0, 17), (2, 0, 3), 4, lib, DEV)
    bc.check_fused_equals_three(shape, dt, (5, 2, 9), None, 4, lib, DEV, null_idx=True)
    if shape == "base":
        bc.check_fused_equals_three(shape, dt, (8,) * 8, tuple(range(8)), 8, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", ["small", "base"])
def test_partition_bitwise(shape, dt, lib):
    bc.check_partition(shape, dt, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", ["small", "base"])
def test_vs_fp64_oracle(shape, dt, lib):
    bc.check_vs_oracle(shape, dt, 33, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_no_commit_reads_and_does_not_write(dt, lib):
    bc.check_no_commit("base", dt, lib, DEV)


def test_refusals_touch_nothing(lib):
    bc.check_refusals(lib, DEV)


@pytest.mark.parametrize("d_model", [384, 768])
def test_step_chunk_fused_on_equals_off(d_model):
    bc.check_mamba_arms(d_model, DEV)


def test_model_streams_and_reads_equal_between_arms():
    bc.check_model_arms(DEV)
