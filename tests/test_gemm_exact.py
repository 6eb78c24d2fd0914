"""Exact-arithmetic and per-element checks of the projection products (tests/gemm_exact_checks.py) on the host.  First the conditions on
the exact inputs, on the fp64 reference alone, for every case and dtype, before any kernel runs.  Then the host library: its aum_gemm_tn,
aum_gemm_wgrad, aum_dtproj_tm_fwd, aum_xdt_tm_fwd and aum_xdt_tm_bwd are plain loops (tests/emu/aum_emu.cpp) -- their runs here check the
expectations, the wrappers and the loops' one rounding; the MFMA kernels are held by tests/test_gpu_gemm_exact.py -- while aum_proj_fwd /
_bwd_data / _bwd_weight are the lane-array build of csrc/proj_kernels.h, whose tile and fragment arithmetic runs here."""
import os
import sys

import pytest

import aum_hip
import gemm_exact_checks as GE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

cid = lambda c: "x".join(map(str, c))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


# ---- the inputs, on the reference alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
def test_input_conditions(dtype):
    """conditions 1-4 of gemm_exact_checks.check_conditions for every Part A case: exact fp32 sums in any order, inside the normal range,
    enough inexact results and ties in both directions, and a result that changes under the two wrong rounding modes"""
    for c in GE.GEMM_CASES:
        GE.gemm_conditions(c, dtype)
    for c in GE.WGRAD_CASES:
        GE.wgrad_conditions(c, dtype)
    for c in GE.DTPROJ_CASES:
        GE.dtproj_conditions(c, dtype)
    for c in GE.XDT_CASES:
        GE.xdt_conditions(c, dtype)
    for c in GE.XDT_BWD_CASES:
        GE.xdt_bwd_conditions(c, dtype)
    for c in GE.PROJ_CASES:
        GE.proj_conditions(c, dtype)
    GE.print_shares()


def test_rounding_helpers():
    """the 16-bit grid helpers on values worked by hand: 257 is a bf16 tie that goes down to 256 (even), 259 one that goes up to 260;
    2049 / 2051 the same in fp16; 258.5 is inexact and no tie"""
    import torch
    for dtype, vals in ((GE.BF16, (257.0, 259.0, 258.5, -257.0)), (GE.FP16, (2049.0, 2051.0, 2050.5, -2049.0))):
        step = vals[0] - 1.0
        r = GE.roundings(torch.tensor(vals, dtype=torch.float64), dtype)
        assert r["rne"].double().tolist() == [step, step + 4, step + 2, -step]
        assert r["rz"].tolist() == [step, step + 2, step + 2, -step]
        assert r["rha"].tolist() == [step + 2, step + 4, step + 2, -step - 2]
        assert r["tie"].tolist() == [True, True, False, True] and r["tie_down"].tolist() == [True, False, False, True]
        assert r["inexact"].all()


# ---- Part A ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.GEMM_CASES, ids=cid)
def test_gemm_tn_exact(emu, case, dtype):
    GE.check_gemm_exact(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.WGRAD_CASES, ids=cid)
def test_gemm_wgrad_exact(emu, case, dtype):
    GE.check_wgrad_exact(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.DTPROJ_CASES, ids=cid)
def test_dtproj_tm_exact(emu, case, dtype):
    GE.check_dtproj_exact(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_CASES, ids=cid)
def test_xdt_tm_fwd_exact(emu, case, dtype):
    GE.check_xdt_exact(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_BWD_CASES, ids=cid)
def test_xdt_tm_bwd_exact(emu, case, dtype):
    GE.check_xdt_bwd_exact(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.PROJ_CASES, ids=lambda c: c[0])
def test_proj_exact(emu, case, dtype):
    GE.check_proj_exact(emu, "cpu", case, dtype)


# ---- Part B ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.GEMM_CASES, ids=cid)
def test_gemm_tn_interval(emu, case, dtype):
    GE.check_gemm_interval(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.WGRAD_CASES, ids=cid)
def test_gemm_wgrad_interval(emu, case, dtype):
    GE.check_wgrad_interval(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.DTPROJ_CASES, ids=cid)
def test_dtproj_tm_interval(emu, case, dtype):
    GE.check_dtproj_interval(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_CASES, ids=cid)
def test_xdt_tm_fwd_interval(emu, case, dtype):
    GE.check_xdt_interval(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_BWD_CASES, ids=cid)
def test_xdt_tm_bwd_interval(emu, case, dtype):
    GE.check_xdt_bwd_interval(emu, "cpu", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.PROJ_CASES, ids=lambda c: c[0])
def test_proj_interval(emu, case, dtype):
    GE.check_proj_interval(emu, "cpu", case, dtype)


# ---- Part C ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("family", ("gemm_auto", "dtproj", "xdt"))
def test_edges(emu, family, dtype):
    GE.check_edges(emu, "cpu", family, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("family", ("gemm_auto", "dtproj", "xdt"))
def test_subnormal_inputs(emu, family, dtype):
    """the host loops convert 16-bit subnormals to fp32 exactly and multiply them there: the rounded fp64 product, as the contract says"""
    GE.check_subnormal_inputs(emu, "cpu", family, dtype, flushed=False)
