"""GPU: PACKED streaming prefill on the MI355X -- the checks of tests/stream_prefill_packed_checks.py on libaum_hip.so:
k_convt_prefill_var bit-equal to conv1d_tm_prefill per session, k_scant_fwd_state_var / k_scant_seg_fwd_state_var bit-equal to
scan_tm_fwd_state per session and inside the oracle bars, packing invariance with NaN neighbours, Mamba.prefill_chunk(seq_map=)
(d_inner 256 with dt_rank 24 runs aum_xdt_tm_fwd) and AudioMamba.stream_prefill_many(packed=True).  Every test fails on the commit
before the feature (missing symbol / AttributeError / unknown keyword)."""
import pytest

import aum_hip
import stream_checks as sc
import stream_prefill_checks as pc
import stream_prefill_packed_checks as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = ("f32", "bf16", "f16")


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


def test_symbols_exported_abi_unchanged(lib):
    for name in ("aum_conv1d_tm_prefill_var", "aum_scan_tm_fwd_state_var", "aum_scan_tm_fwd_state_var_carry_bytes"):
        assert name in aum_hip.EXPORTS and hasattr(lib.c, name)
    assert lib.c.aum_abi_version() == 13


@pytest.mark.parametrize("dt,dim,k", [("f32", 64, 0), ("bf16", 256, 0), ("f16", 64, 3), ("bf16", 64, 2), ("f32", 256, 5), ("f16", 256, 5)])
def test_conv(lib, dt, dim, k):
    pk.check_conv(dt, sc.CONV_KINDS[k], dim, lib, DEV)


def test_conv_zero_window(lib):
    pk.check_conv("bf16", sc.CONV_KINDS[0], 72, lib, DEV, zero_window=True)


@pytest.mark.parametrize("dt,dim,k", [("f32", 64, 0), ("bf16", 256, 1), ("f16", 64, 2), ("f32", 256, 5), ("bf16", 64, 5), ("f16", 256, 0)])
def test_scan_uncut(lib, dt, dim, k):
    pk.check_scan(dt, pc.KINDS[k], dim, lib, DEV, pk.SCAN_LENS, state_oracle=pk.session_state_oracle(dt, pc.KINDS[k], dim, DEV, pk.SCAN_LENS))


@pytest.mark.parametrize("dt,dim,k", [("f32", 256, 0), ("bf16", 64, 1), ("f16", 256, 3)])
def test_scan_cut_coinciding_ranges(lib, dt, dim, k):
    pk.check_scan(dt, pc.KINDS[k], dim, lib, DEV, pk.CUT_LENS, range_len=8, state_oracle=pk.session_state_oracle(dt, pc.KINDS[k], dim, DEV, pk.CUT_LENS))


@pytest.mark.parametrize("dt", DTS)
def test_scan_cut_other_ranges(lib, dt):
    lens = (513, 130)
    pk.check_scan(dt, pc.KINDS[0], 64, lib, DEV, lens, range_len=128, bitwise=False, state_oracle=pk.session_state_oracle(dt, pc.KINDS[0], 64, DEV, lens))


def test_scan_cut_1024_in_8(lib):
    lens = (1024, 300)
    pk.check_scan("f32", pc.KINDS[3], 64, lib, DEV, lens, range_len=128, bitwise=False,
                  state_oracle=pk.session_state_oracle("f32", pc.KINDS[3], 64, DEV, lens))


@pytest.mark.parametrize("dt,range_len", [("f32", 0), ("bf16", 0), ("f16", 8)])
def test_packing_invariance_scan(lib, dt, range_len):
    pk.check_packing_invariance(dt, pc.KINDS[0], 64, lib, DEV, range_len)


def test_packing_invariance_conv(lib):
    pk.check_conv_packing_invariance("bf16", 72, lib, DEV)


def test_refusals(lib):
    pk.check_refusals(lib, DEV)


@pytest.mark.parametrize("d_model,dt_rank", [(128, 24), (32, "auto")])
@pytest.mark.parametrize("dt", DTS)
def test_block(lib, d_model, dt_rank, dt):
    pk.check_block(d_model, dt_rank, dt, lib, DEV)


def test_model_packed_prefill(lib):
    pk.check_model(lib, DEV)


def test_model_refusals_touch_nothing(lib):
    pk.check_model_refusals(lib, DEV)
