"""Exact-arithmetic and per-element checks of the projection products (tests/gemm_exact_checks.py) of the product library on an MI355X: the MFMA
kernels of gemm_kernels.h, gemm_ps_kernels.h, dtproj_kernels.h, xdt_kernels.h, xdt_fwd_body.inc and proj_kernels.h, bit for bit against the
rounded fp64 product on exact inputs (Part A), inside the derived per-element interval on the usual randn inputs (Part B), and bit for bit
on the edges (Part C).  Run with -m gpu.  Measured on the MI355X: 185 cases in 2.8 s (the slowest, the first launch, 0.27 s; the fp64
references on the host included)."""
import pytest
import torch

import aum_hip
import gemm_exact_checks as GE

pytestmark = pytest.mark.gpu

cid = lambda c: "x".join(map(str, c))
ALL_SCHEDS = tuple(GE.SCHEDS)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


# ---- Part A ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.GEMM_CASES, ids=cid)
def test_gemm_tn_exact(lib, case, dtype):
    """every schedule bit-equal to the rounded fp64 product, hence to each other; the paced flag below k = 448 refused"""
    outs = GE.check_gemm_exact(lib, "cuda", case, dtype, ALL_SCHEDS)
    assert len(outs) == (4 if case[2] >= GE.PACED_MIN_K else 3)
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.WGRAD_CASES, ids=cid)
def test_gemm_wgrad_exact(lib, case, dtype):
    GE.check_wgrad_exact(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.DTPROJ_CASES, ids=cid)
def test_dtproj_tm_exact(lib, case, dtype):
    GE.check_dtproj_exact(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_CASES, ids=cid)
def test_xdt_tm_fwd_exact(lib, case, dtype):
    """x_dbl, delta from the EXPECTED rounded x_dbl, and the softplus form's x_dbl bit-equal to the plain form's"""
    GE.check_xdt_exact(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_BWD_CASES, ids=cid)
def test_xdt_tm_bwd_exact(lib, case, dtype):
    GE.check_xdt_bwd_exact(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.PROJ_CASES, ids=lambda c: c[0])
def test_proj_exact(lib, case, dtype):
    GE.check_proj_exact(lib, "cuda", case, dtype)


# ---- Part B ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.GEMM_CASES, ids=cid)
def test_gemm_tn_interval(lib, case, dtype):
    """every schedule inside the interval, and the schedules bit-equal to each other on real-valued inputs too"""
    GE.check_gemm_interval(lib, "cuda", case, dtype, ALL_SCHEDS)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.WGRAD_CASES, ids=cid)
def test_gemm_wgrad_interval(lib, case, dtype):
    GE.check_wgrad_interval(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.DTPROJ_CASES, ids=cid)
def test_dtproj_tm_interval(lib, case, dtype):
    GE.check_dtproj_interval(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_CASES, ids=cid)
def test_xdt_tm_fwd_interval(lib, case, dtype):
    GE.check_xdt_interval(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.XDT_BWD_CASES, ids=cid)
def test_xdt_tm_bwd_interval(lib, case, dtype):
    GE.check_xdt_bwd_interval(lib, "cuda", case, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("case", GE.PROJ_CASES, ids=lambda c: c[0])
def test_proj_interval(lib, case, dtype):
    GE.check_proj_interval(lib, "cuda", case, dtype)


def test_report_ratios():
    """prints the Part B table of this run (the header of gemm_exact_checks.py records the MI355X's)"""
    GE.print_ratios()


# ---- Part C ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("family", GE.EDGE_FAMILIES)
def test_edges(lib, family, dtype):
    GE.check_edges(lib, "cuda", family, dtype)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=GE.dt_id)
@pytest.mark.parametrize("family", GE.EDGE_FAMILIES)
def test_subnormal_inputs(lib, family, dtype):
    """16-bit subnormal inputs (integers times 2^-24 in fp16, 2^-133 in bf16) against weights scaled so that the results are normal.
    Observed on the MI355X: the matrix unit does not flush them -- every kernel and schedule returns the rounded fp64 product bit for bit,
    which is what the contract (exact products) says and what GE.MFMA_FLUSHES_SUBNORMAL_INPUTS = False for both types holds them to.  Were
    a part to flush, the table would say so and the case would be held to the flushed product exactly; it is never left loose."""
    GE.check_subnormal_inputs(lib, "cuda", family, dtype, flushed=GE.MFMA_FLUSHES_SUBNORMAL_INPUTS[dtype])
