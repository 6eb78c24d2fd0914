"""Poison checks (tests/poison_checks.py) of the product library on an MI355X: NaN and large finite values in everything the token-major
training kernels do not own, sentinels around everything they write.  Run with -m gpu."""
import pytest
import torch

import aum_hip
import poison_checks as PC

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALVES = [torch.bfloat16, torch.float16]
dt_id = lambda d: str(d).split(".")[-1]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.mark.parametrize("case", PC.CONV_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
def test_conv_tm_poison(lib, case, dtype, reverse):
    for silu in (True, False):
        PC.check_conv_tm_poison(lib, "cuda", case, dtype, reverse, silu)


@pytest.mark.parametrize("case,segments", PC.SCAN_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else f"seg{v}")
@pytest.mark.parametrize("direction", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_scan_tm_poison(lib, case, segments, direction, dtype):
    PC.check_scan_tm_poison(lib, "cuda", case, dtype, direction, segments)


@pytest.mark.parametrize("case", PC.DTPROJ_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_dtproj_tm_poison(lib, case, dtype):
    PC.check_dtproj_poison(lib, "cuda", *case, dtype)


@pytest.mark.parametrize("case", PC.XDT_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_xdt_tm_poison(lib, case, dtype):
    PC.check_xdt_poison(lib, "cuda", *case[:3], dtype, *case[3:])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_xdt_tm_tiny_poison(lib, dt):
    PC.check_xdt_tiny_poison(lib, "cuda", dt)


@pytest.mark.parametrize("case", PC.XDT_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_xdt_tm_bwd_poison(lib, case, dtype):
    PC.check_xdt_bwd_poison(lib, "cuda", case[0], case[1], dtype, case[2])


@pytest.mark.parametrize("case", PC.GEMM_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
@pytest.mark.parametrize("sched", ["auto", "lockstep", "pipelined", "paced"])
def test_gemm_tn_poison(lib, case, dtype, sched):
    """every schedule flag; the paced-store kernel needs seven K-steps per tile: named on a shorter product it is refused, nothing written"""
    flags = {"auto": 0, "lockstep": aum_hip.GEMM_LOCKSTEP, "pipelined": aum_hip.GEMM_PIPELINED, "paced": aum_hip.GEMM_PACED}[sched]
    PC.check_gemm_poison(lib, "cuda", *case, dtype, flags=flags, refused=(sched == "paced" and case[2] < 448))


@pytest.mark.parametrize("case", PC.GEMM_WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", HALVES, ids=dt_id)
def test_gemm_wgrad_poison(lib, case, dtype):
    PC.check_gemm_wgrad_poison(lib, "cuda", *case[:4], dtype, *case[4:])
