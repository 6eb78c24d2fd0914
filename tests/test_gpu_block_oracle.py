"""The fused Mamba block under 16-bit autocast at the widths its fast kernels take (d_inner 768 / 1536, dt_rank 24 / 48) against the fp64
oracle of the whole block -- output, d xz and every parameter gradient -- on both layouts, both 16-bit types, and with each A/B switch
of the existing arm-against-arm tests on either side: block_oracle_checks.check_block (bars: 2.2 x what the stored 16-bit tensors
cost the fp64 computation itself, measured when the test runs; the launches each arm is about are asserted by name)."""
import pytest
import torch

import aum_hip
import block_oracle_checks as BC
import cases

pytestmark = pytest.mark.gpu

_DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
_SWITCH_CASES = [BC.WIDE["v1_d768_l65"], BC.WIDE["v2_d384_l65"]]


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.mark.parametrize("case", cases.INNER_WIDE_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("layout", ["token_major", "channel_major"])
@_DTYPES
def test_block_vs_oracle(monkeypatch, case, layout, dtype):
    """as dispatched: token-major on conv_tm / the fused x/dt kernels / scan_tm / the skinny aum_gemm_wgrad with delta handed over
    activated, channel-major on the row kernels and aum_proj_*"""
    BC.check_block(case, dtype, layout, {}, "cuda", monkeypatch)


@pytest.mark.parametrize("case", _SWITCH_CASES, ids=lambda c: c[0])
def test_block_vs_oracle_gemm_hip(monkeypatch, case):
    """out_proj and its data gradient on aum_gemm_tn whatever _HIP_GEMM_FASTER says (Bi-Bi: through out_proj_shared, as Mamba.forward)"""
    BC.check_block(case, torch.bfloat16, "token_major", {"_GEMM_MODE": "hip", "_HIP_GEMM": True}, "cuda", monkeypatch,
                   shared_out_proj=case[1] == "v2")


@pytest.mark.parametrize("case", _SWITCH_CASES, ids=lambda c: c[0])
def test_block_vs_oracle_delta_in_scan(monkeypatch, case):
    """dt_bias and the softplus inside both scans (the other side of test_gpu_delta_activated._block_ab)"""
    BC.check_block(case, torch.bfloat16, "token_major", {"_DELTA_IN_XDT": False}, "cuda", monkeypatch)


@pytest.mark.parametrize("case", _SWITCH_CASES, ids=lambda c: c[0])
def test_block_vs_oracle_xdt_bwd_library(monkeypatch, case):
    """the x_proj / dt_proj gradients as five library calls (the other side of test_gpu_xdt_small._block_pair)"""
    BC.check_block(case, torch.bfloat16, "token_major", {"_XDT_BWD_HIP": False}, "cuda", monkeypatch)
