"""CPU: peek rows every P rows of streaming inference on the lane-array build of the kernel sources (tests/emu) -- convc_unit / scanc_unit
with PEEKS run as host code through aum_conv1d_tm_chunk_peeks / aum_scan_tm_chunk_peeks, the binding, the ladder's host loop,
Mamba.step_chunk(peek_every=) and AudioMamba.stream_timeline / stream_timeline_many (tests/stream_timeline_checks.py).  The device kernels
are held to the same checks in tests/test_gpu_stream_timeline.py.
On the commit before the feature every test here fails: the library has no aum_*_tm_chunk_peeks symbols, aum_hip no *_chunk_peeks
functions, `peek_every=` raises a TypeError and AudioMamba has no stream_timeline."""
import os
import sys

import pytest
import torch

import aum_hip
import stream_timeline_checks as tc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture()
def emu_as_product(lib):
    old = aum_hip._product
    aum_hip._product = lib
    yield
    aum_hip._product = old


def test_names_are_declared_and_exported(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aum_hip.h")).read()
    for name in ("aum_conv1d_tm_chunk_peeks", "aum_scan_tm_chunk_peeks"):
        assert f"int {name}(" in header and name in aum_hip.EXPORTS and hasattr(lib.c, name)
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13
    import ctypes
    for peeks, var in ((aum_hip.ConvTmChunkPeeksArgs, aum_hip.ConvTmChunkVarArgs), (aum_hip.ScanTmChunkPeeksArgs, aum_hip.ScanTmChunkVarArgs)):
        assert ctypes.sizeof(peeks) == ctypes.sizeof(var) + 8 and peeks.peek_every.offset == ctypes.sizeof(var) and peeks.base.offset == 0


@pytest.mark.parametrize("P", tc.PERIODS)
@pytest.mark.parametrize("dim", tc.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peeks_equal_the_chain_of_peek_last_calls(op, dt, dim, P, lib):
    tc.check_peeks_equal_chain(op, dt, dim, P, lib, "cpu", kind=tc.PERIODS.index(P) + tc.DIMS.index(dim))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_a_sequence_without_a_peek_row_is_the_plain_call(op, dt, lib):
    for P in (1, 8):
        tc.check_no_peek_row_is_plain_var(op, dt, 128, P, lib, "cpu")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peeks_against_the_fp64_recurrence(op, dt, lib):
    tc.check_vs_fp64(op, dt, lib, "cpu")


@pytest.mark.parametrize("op", ["conv", "scan"])
def test_refusals_touch_nothing(op, lib):
    tc.check_refusals(op, lib, "cpu")


def test_ladder_loops_over_the_groups_where_the_packed_kernels_refuse(lib):
    tc.check_host_loop(lib)


def _mamba():
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(4)
    return Mamba(64, bimamba_type="none", layer_idx=0)


def test_step_chunk_peek_every_fixed_batch(emu_as_product):
    m = _mamba()
    torch.manual_seed(8)
    for P, T in ((4, 17), (1, 6), (8, 9), (3, 3)):
        tc.check_mamba_peek_every(m, torch.randn(2, T, 64), P, "cpu", 1e-4)


def test_step_chunk_peek_every_packed_sessions(emu_as_product):
    m = _mamba()
    torch.manual_seed(9)
    smap = aum_hip.seq_map([9, 3, 0, 4], [3, 0, 1, 2], device="cpu")
    tc.check_mamba_peek_every(m, torch.randn(1, 16, 64), 3, "cpu", 1e-4, seq_map=smap, pool_rows=4)


def test_step_chunk_exclusive_arguments(emu_as_product):
    tc.check_mamba_exclusive_arguments(_mamba(), "cpu")


@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_timeline_matches_the_per_column_loop(embed_dim, emu_as_product):
    tc.check_model_timeline(embed_dim, "cpu")


@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_timeline_many_matches_sessions_served_alone(embed_dim, emu_as_product):
    tc.check_model_timeline_many(embed_dim, "cpu")


def test_model_timeline_refusals_touch_nothing(emu_as_product):
    tc.check_model_timeline_refusals("cpu")
