"""Gradient-home checks (tests/grad_home_checks.py) on the host: the lane-array build stands where libaum_hip.so would, so the destinations of
the sums and of the scan's parameter sums, the home bookkeeping of selective_scan_interface (grad_home, its claims, _homed, the d A_log
hand-over) and the RMSNorm weight home run here in fp32.  GPU-only, held by tests/test_gpu_grad_home.py: the homes of the x_proj, dt_proj,
in_proj and out_proj weights (the x/dt and weight-gradient MFMA kernels are asked for on the device only: ssi._xdt_bwd, _wgrad_tm), 16-bit
autocast, the fp64 oracle's bars (derived for 16-bit autocast) and a home that lives on the CPU while the parameter does not."""
import os
import sys

import pytest
import torch

import aum_hip
import grad_home_checks as GH

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    old = aum_hip._product
    aum_hip._product = lib = aum_hip.Lib(build_emu.build(), host=True)
    yield lib
    aum_hip._product = old


@pytest.fixture
def ssi(emu, monkeypatch):
    import mamba_ssm.ops.selective_scan_interface as m
    monkeypatch.setattr(m, "_TM_MIN_WAVES", 1)
    return m


@pytest.mark.parametrize("shape", GH.SUM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_sum_rows_dest(emu, shape, dtype):
    GH.check_sum_rows_dest(emu, "cpu", shape, dtype)


@pytest.mark.parametrize("which", range(len(GH.SUM_MULTI_SETS)), ids=["one_launch", "two_stage_set"])
def test_sum_rows_multi_dest(emu, which):
    GH.check_sum_rows_multi_dest(emu, "cpu", *GH.SUM_MULTI_SETS[which])


@pytest.mark.parametrize("case", GH.WGRAD_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_gemm_wgrad_dest(emu, case):
    GH.check_gemm_wgrad_dest(emu, "cpu", case, torch.bfloat16)


@pytest.mark.parametrize("case,segments", GH.SCAN_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else f"seg{v}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_scan_param_dest(emu, case, segments, dtype):
    GH.check_scan_param_dest(emu, "cpu", case, dtype, segments)


def test_unfit_dest(emu):
    GH.check_unfit_dest(emu, "cpu", torch.bfloat16)


@pytest.mark.parametrize("case", GH.BLOCK_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("head", [0, 1], ids=["aligned16", "off4"])
def test_block_homes(ssi, case, head):
    GH.check_block_homes(ssi, case, None, "cpu", head)


@pytest.mark.parametrize("head", [0, 1], ids=["aligned16", "off4"])
def test_model_homes(ssi, head):
    GH.check_model_homes(ssi, None, "cpu", head)


def test_frozen(ssi):
    GH.check_frozen(ssi, None, "cpu")


def test_unfit_homes(ssi):
    GH.check_unfit_homes(ssi, GH.BLOCK_CASES[1], None, "cpu")


def test_da_xa_handover(ssi, monkeypatch):
    GH.check_da_xa_handover(ssi, monkeypatch, None, "cpu")


def test_a_used_twice(ssi):
    GH.check_a_used_twice(ssi, None, "cpu")
