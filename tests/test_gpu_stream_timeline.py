"""GPU: peek rows every P rows of streaming inference on the device library -- k_convt_chunk_peeks and k_stream_scan_chunk_peeks against
the chain of aum_*_tm_chunk_var calls with and without the PEEK_LAST flag, bit for bit, and against an fp64 recurrence; the refusals;
Mamba.step_chunk(peek_every=) in bf16 and AudioMamba.stream_timeline / stream_timeline_many at embed 64 (library x/dt) and 192 (the padded
48-column x/dt kernels) with and without bf16 autocast (tests/stream_timeline_checks.py).
On the commit before the feature every test here fails: the library has no aum_*_tm_chunk_peeks symbols, aum_hip no *_chunk_peeks
functions, `peek_every=` raises a TypeError and AudioMamba has no stream_timeline."""
import pytest
import torch

import aum_hip
import stream_block_checks as bc
import stream_timeline_checks as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("dim", tc.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peeks_equal_the_chain_of_peek_last_calls(op, dt, dim, lib):
    for P in tc.PERIODS:
        tc.check_peeks_equal_chain(op, dt, dim, P, lib, DEV, kind=tc.PERIODS.index(P) + tc.DIMS.index(dim))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_a_sequence_without_a_peek_row_is_the_plain_call(op, dt, lib):
    for P in (1, 8):
        tc.check_no_peek_row_is_plain_var(op, dt, 384, P, lib, DEV)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peeks_against_the_fp64_recurrence(op, dt, lib):
    tc.check_vs_fp64(op, dt, lib, DEV)


@pytest.mark.parametrize("op", ["conv", "scan"])
def test_refusals_touch_nothing(op, lib):
    tc.check_refusals(op, lib, DEV)


def _mamba(d_model):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(11)
    return Mamba(d_model, bimamba_type="none", layer_idx=0).to(DEV).to(torch.bfloat16)


@pytest.mark.parametrize("d_model", [192, 384])
def test_step_chunk_peek_every(d_model):
    """bf16 module on the ladder: outputs within the 16-bit output bar (the in_proj GEMM sees another row count than in the group calls),
    the caches bit for bit"""
    m = _mamba(d_model)
    torch.manual_seed(3)
    bar = bc.OUT_BAR["bf16"]
    tc.check_mamba_peek_every(m, torch.randn(2, 27, d_model, device=DEV).to(torch.bfloat16), 8, DEV, bar)
    smap = aum_hip.seq_map([9, 3, 0, 4], [3, 0, 1, 2], device=DEV)
    tc.check_mamba_peek_every(m, torch.randn(1, 16, d_model, device=DEV).to(torch.bfloat16), 3, DEV, bar, seq_map=smap, pool_rows=4)


def test_step_chunk_exclusive_arguments():
    tc.check_mamba_exclusive_arguments(_mamba(192), DEV)


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_timeline_matches_the_per_column_loop(embed_dim, autocast):
    tc.check_model_timeline(embed_dim, DEV, autocast)


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_timeline_many_matches_sessions_served_alone(embed_dim, autocast):
    tc.check_model_timeline_many(embed_dim, DEV, autocast)


def test_model_timeline_refusals_touch_nothing():
    tc.check_model_timeline_refusals(DEV)
