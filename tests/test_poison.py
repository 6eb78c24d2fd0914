"""Poison checks (tests/poison_checks.py) on the host: the lane-array build executes the conv and scan kernel bodies that hipcc compiles for
gfx950, so their masks, tails and row offsets are held to the rule here without a GPU.  The dt / x-dt projections and the two GEMMs are
plain loops behind the shared argument rules in that build (tests/emu/aum_emu.cpp): their runs here check the layouts and the checks
themselves; the MFMA kernels' own masks are held by tests/test_gpu_poison.py."""
import os
import sys

import pytest
import torch

import aum_hip
import poison_checks as PC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
dt_id = lambda d: str(d).split(".")[-1]


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("case", PC.CONV_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
def test_conv_tm_poison(emu, case, dtype, reverse):
    for silu in (True, False):
        PC.check_conv_tm_poison(emu, "cpu", case, dtype, reverse, silu)


@pytest.mark.parametrize("case,segments", PC.SCAN_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else f"seg{v}")
@pytest.mark.parametrize("direction", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_scan_tm_poison(emu, case, segments, direction, dtype):
    PC.check_scan_tm_poison(emu, "cpu", case, dtype, direction, segments)


@pytest.mark.parametrize("case", PC.DTPROJ_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dtproj_tm_poison(emu, case):
    PC.check_dtproj_poison(emu, "cpu", *case, torch.bfloat16)


@pytest.mark.parametrize("case", PC.XDT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xdt_tm_poison(emu, case):
    PC.check_xdt_poison(emu, "cpu", *case[:3], torch.bfloat16, *case[3:])


def test_xdt_tm_tiny_poison(emu):
    PC.check_xdt_tiny_poison(emu, "cpu", "bf16")


@pytest.mark.parametrize("case", PC.XDT_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xdt_tm_bwd_poison(emu, case):
    PC.check_xdt_bwd_poison(emu, "cpu", case[0], case[1], torch.float16, case[2])


@pytest.mark.parametrize("case", PC.GEMM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gemm_tn_poison(emu, case):
    """(the host loop has one schedule: the flags are the device kernels')"""
    PC.check_gemm_poison(emu, "cpu", *case, torch.bfloat16)


@pytest.mark.parametrize("case", PC.GEMM_WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gemm_wgrad_poison(emu, case):
    PC.check_gemm_wgrad_poison(emu, "cpu", *case[:4], torch.bfloat16, *case[4:])
