"""GPU: a streaming hop through all blocks in one library call on the device library -- k_stream_in and k_stream_out through
aum_stream_in_tm / aum_stream_out_tm, the C loop of aum_stream_layers around k_stream_block, and AudioMamba.stream_stack / stack=: the
checks of tests/stream_stack_checks.py on the MI355X (tests/test_stream_stack.py runs them on the lane-array build).  On the commit
before the feature every test here fails: the entry points and the methods do not exist."""
import pytest
import torch

import aum_hip
import stream_stack_checks as ss

pytestmark = pytest.mark.gpu
DEV = "cuda"
WID = lambda w: f"{w[0]}x{w[1]}"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("with_res", [False, True], ids=["first_block", "residual"])
@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_norm_prologue_bitwise(lib, widths, dtype, with_res):
    for total in (1, 17, 73):
        ss.check_norm_prologue(lib, DEV, widths, dtype, total, with_res)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_exact_inputs(lib, widths, dtype):
    ss.pooled_conditions(widths, dtype)
    for total in ss.TOTALS:
        ss.out_conditions(widths, dtype, total)
        ss.in_conditions(widths, dtype, total)
        ss.check_out_exact(lib, DEV, widths, dtype, total)
        ss.check_in_exact(lib, DEV, widths, dtype, total)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_random_inputs_interval(lib, widths, dtype):
    for total in ss.TOTALS:
        ss.check_out_interval(lib, DEV, widths, dtype, total)
        ss.check_in_interval(lib, DEV, widths, dtype, total)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_partition_bitwise(lib, widths, dtype):
    ss.check_partition(lib, DEV, widths, dtype)


@pytest.mark.parametrize("mode", ["commit", "peek", "no_commit"])
@pytest.mark.parametrize("map_name", sorted(ss.MAPS))
@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_chain_is_the_composition(lib, widths, dtype, map_name, mode):
    ss.check_chain(lib, DEV, widths, dtype, map_name, mode)


def test_refusals_touch_nothing(lib):
    ss.check_refusals(lib, DEV)


@pytest.mark.parametrize("embed_dim", [384, 192], ids=["small", "tiny"])
def test_model_arms_against_offline(lib, embed_dim):
    ss.check_model_arms(lib, DEV, embed_dim)


def test_hop_cut_bitwise(lib):
    ss.check_hop_cut(lib, DEV)


def test_one_call_per_hop(lib):
    ss.check_one_call(lib, DEV)


def test_stack_cache(lib):
    ss.check_stack_cache(lib, DEV)
