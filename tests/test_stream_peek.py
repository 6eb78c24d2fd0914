"""CPU: the peek row of streaming inference on the lane-array build of the kernel sources (tests/emu) -- convc_unit / scanc_unit with PEEK
run as host code through aum_conv1d_tm_chunk_var / aum_scan_tm_chunk_var, aum_stream_block_tm as their host composition (its sb_split
hands the flag on), the binding, Mamba.step_chunk(peek=) on the ladder and AudioMamba.stream_push / stream_push_many(read=)
(tests/stream_peek_checks.py).  The one-launch kernel is held to the same checks on the device (tests/test_gpu_stream_peek.py).
On the commit before the feature every test here fails: the `peek=` / `read=` keyword raises a TypeError, aum_hip.STREAM_PEEK_LAST is an
AttributeError, and the raw call with the flag is refused with AUM_E_UNSUPPORTED where it must be taken."""
import os
import sys

import pytest
import torch

import aum_hip
import stream_block_checks as bc
import stream_peek_checks as pc

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


@pytest.mark.parametrize("case", list(pc.CASES))
@pytest.mark.parametrize("shape,dt", [("small", "bf16"), ("small", "f16")])
def test_peek_equals_commit_then_uncommitted_last_row(shape, dt, case, lib):
    lens, rows, nrows = pc.CASES[case]
    pc.check_peek_equals_two_calls(shape, dt, lens, rows, nrows, lib, "cpu")


def test_flag_values_and_raw_call_with_the_flag_is_taken(lib):
    assert (aum_hip.STREAM_PEEK_LAST, aum_hip.CONV_PEEK_LAST, aum_hip.SCAN_PEEK_LAST) == (2, 8, 64)
    assert aum_hip.STREAM_PEEK_LAST & aum_hip.STREAM_NO_COMMIT == 0
    assert aum_hip.CONV_PEEK_LAST & (aum_hip.CONV_SILU | aum_hip.CONV_REVERSE | 4) == 0
    assert aum_hip.SCAN_PEEK_LAST & (1 | 2 | 4 | 8 | 16 | aum_hip.SCAN_DELTA_ACTIVATED) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aum_hip.h")).read()
    for name, val in (("AUM_STREAM_PEEK_LAST", 2), ("AUM_CONV_PEEK_LAST", 8), ("AUM_SCAN_PEEK_LAST", 64)):
        assert f"#define {name} {val}u" in header
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13
    o, live, smap = pc.setup("small", "bf16", (5,), (0,), 1, "cpu")
    y = torch.zeros(5, o["dim"], dtype=o["x"].dtype)
    scratch = torch.zeros(int(lib.c.aum_stream_block_scratch_bytes(5, o["dim"], 56)), dtype=torch.uint8)
    a = bc.raw_args(o, smap, y, scratch, lib)
    a.flags = aum_hip.STREAM_PEEK_LAST
    assert bc.call_raw(a, y, lib) == 0


def test_flag_off_changes_nothing(lib):
    pc.check_flag_off_unchanged("small", "bf16", lib, "cpu")


def test_limits_count_the_peek_row(lib):
    pc.check_limits(lib, "cpu")


def test_fixed_batch_with_peek_goes_through_the_packed_kernels(lib):
    pc.check_fixed_batch_goes_packed("small", "bf16", lib, "cpu")


def test_fixed_batch_entry_points_refuse_the_flags(lib):
    x, cs = torch.randn(1, 3, 64), torch.randn(1, 64, 4)
    a = aum_hip.ConvTmChunkArgs()
    y, held = aum_hip._conv_chunk_operands(a, "t", lib, x, cs, torch.randn(64, 4), None, True, None)
    snap = cs.clone()
    assert lib.c.aum_conv1d_tm_chunk(aum_hip.C_byref(a), None) == 0 and not torch.equal(cs, snap)
    a.flags |= aum_hip.CONV_PEEK_LAST
    snap = cs.clone()
    assert lib.c.aum_conv1d_tm_chunk(aum_hip.C_byref(a), None) == -4 and torch.equal(cs, snap)


def test_ladder_loops_over_sessions_where_the_packed_kernels_refuse(lib):
    pc.check_host_loop(lib)


def _mamba():
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(4)
    return Mamba(64, bimamba_type="none", layer_idx=0)


def test_step_chunk_peek_fp32_ladder(emu_as_product):
    """fp32 on the emulator: outputs within 1e-4; the caches torch.equal those of the call on the rows before the peek row where the host
    matmul's row results do not depend on its row count (the in_proj rows are then the same rows), else within CACHE_BAR"""
    m = _mamba()
    torch.manual_seed(8)
    for T in (5, 2, 9):
        pc.check_mamba_peek(m, torch.randn(2, T, 64), "cpu", 1e-4, pc.CACHE_BAR, exact_caches=True)
    # T == 1: the peek alone, nothing committed
    h = torch.randn(2, 1, 64)
    c, s = torch.randn(2, m.d_inner, 4), torch.randn(2, m.d_inner, 16) * 0.3
    c0, s0 = c.clone(), s.clone()
    with torch.no_grad():
        out, _, _ = m.step_chunk(h, c, s, peek=True)
        ref, _, _ = m.step_chunk(h, c0.clone(), s0.clone())
    assert torch.equal(c, c0) and torch.equal(s, s0)
    assert pc.rel_err(out.numpy(), ref.numpy()) < 1e-4
    with pytest.raises(NotImplementedError):
        m.step_chunk(h, c, s, peek=True, commit=False)          # the uncommitted read stays the one-launch path's


def test_step_chunk_peek_packed_sessions(emu_as_product):
    m = _mamba()
    torch.manual_seed(9)
    smap = aum_hip.seq_map([4, 1, 0, 9], [3, 0, 1, 2], device="cpu")
    pc.check_mamba_peek(m, torch.randn(1, 14, 64), "cpu", 1e-4, pc.CACHE_BAR, seq_map=smap, pool_rows=4, exact_caches=True)


def test_model_push_read_matches_push_then_read(emu_as_product):
    pc.check_model_push_read(64, "cpu")


def test_model_push_many_read_matches_sessions_served_alone(emu_as_product):
    pc.check_model_push_many_read(64, "cpu")


def test_model_read_refusals_touch_nothing(emu_as_product):
    pc.check_model_read_refusals("cpu")
