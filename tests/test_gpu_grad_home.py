"""Gradient-home checks (tests/grad_home_checks.py) of the product library on an MI355X: destinations at every 4-byte offset of a 16-byte
boundary, and the token-major block and a depth-2 model with hand-attached homes against a copy without, under bf16 and fp16 autocast.
Run with -m gpu."""
import pytest
import torch

import aum_hip
import grad_home_checks as GH

pytestmark = pytest.mark.gpu

HALVES = [torch.bfloat16, torch.float16]
dt_id = lambda d: str(d).split(".")[-1]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.fixture
def ssi(lib, monkeypatch):
    import mamba_ssm.ops.selective_scan_interface as m
    monkeypatch.setattr(m, "_TM_MIN_WAVES", 1)
    return m


@pytest.mark.parametrize("shape", GH.SUM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=dt_id)
def test_sum_rows_dest(lib, shape, dtype):
    GH.check_sum_rows_dest(lib, "cuda", shape, dtype)


@pytest.mark.parametrize("which", range(len(GH.SUM_MULTI_SETS)), ids=["one_launch", "two_stage_set"])
def test_sum_rows_multi_dest(lib, which):
    GH.check_sum_rows_multi_dest(lib, "cuda", *GH.SUM_MULTI_SETS[which])


@pytest.mark.parametrize("case", GH.WGRAD_CASES, ids=lambda c: "x".join(map(str, c[:4])))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_gemm_wgrad_dest(lib, case, dtype):
    GH.check_gemm_wgrad_dest(lib, "cuda", case, dtype)


@pytest.mark.parametrize("case,segments", GH.SCAN_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else f"seg{v}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=dt_id)
def test_scan_param_dest(lib, case, segments, dtype):
    GH.check_scan_param_dest(lib, "cuda", case, dtype, segments)


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_unfit_dest(lib, dtype):
    GH.check_unfit_dest(lib, "cuda", dtype)


def test_block_without_homes_meets_the_oracle(ssi):
    GH.check_oracle_once(ssi, "cuda")


@pytest.mark.parametrize("case", GH.BLOCK_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
@pytest.mark.parametrize("head", [0, 1], ids=["aligned16", "off4"])
def test_block_homes(ssi, case, dtype, head):
    GH.check_block_homes(ssi, case, dtype, "cuda", head)


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
@pytest.mark.parametrize("head", [0, 1], ids=["aligned16", "off4"])
def test_model_homes(ssi, dtype, head):
    GH.check_model_homes(ssi, dtype, "cuda", head)


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_frozen(ssi, dtype):
    GH.check_frozen(ssi, dtype, "cuda")


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_unfit_homes(ssi, dtype):
    GH.check_unfit_homes(ssi, GH.BLOCK_CASES[1], dtype, "cuda")


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_da_xa_handover(ssi, monkeypatch, dtype):
    GH.check_da_xa_handover(ssi, monkeypatch, dtype, "cuda")


@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_a_used_twice(ssi, dtype):
    GH.check_a_used_twice(ssi, dtype, "cuda")
