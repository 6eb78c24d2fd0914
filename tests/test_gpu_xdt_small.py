"""AuM-Small widths of the x_proj / dt_proj backward on the GPU: aum_xdt_tm_bwd at dx_dbl rows of 56 columns / dt_rank 24 and the skinny
aum_gemm_wgrad at k = 24 / 56 against fp64 (the rules of kernel_checks.check_xdt_bwd / check_gemm_wgrad, restated width by width in
xdt_small_checks.py), the half fragments against poisoned neighbours, and one Mamba block of AuM-Small's width on the kernel path
against the library path."""
import pytest
import torch

import aum_hip
import kernel_checks as KC
import xdt_small_checks as XC

pytestmark = pytest.mark.gpu

CASES = [(1, 256, 0), (33, 256, 8), (127, 512, 0), (145, 768, 16), (300, 1024, 8), (2305, 768, 0)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_xdt_tm_bwd_small(lib, case, dtype):
    """one token; a ragged last wave and workgroup; both du read-ahead depths (dim % 512); AuM-Small's 768; padded pitches"""
    XC.check_xdt_bwd_w(lib, "cuda", case[0], case[1], dtype, case[2], *XC.SMALL)


def test_xdt_tm_bwd_base_width_same_rule(lib):
    """the (48, 80) instance through the same twin: the column count became a template constant, the results keep the rule"""
    XC.check_xdt_bwd_w(lib, "cuda", 33, 256, torch.bfloat16, 8, *XC.BASE)
    XC.check_xdt_bwd_w(lib, "cuda", 33, 256, torch.float16, 8, *XC.BASE)


def test_xdt_tm_bwd_small_lds_residue(lib):
    """the result does not depend on what earlier kernels left in LDS: the padded halves of the fragments (W_dt^T rows 24..31 of the slab,
    tile columns 56..63, W_x^T chunk 7) are stale LDS, and the forward kernel -- same LDS footprint -- runs on different data before
    each of two launches.  Bit-equal results."""
    res = []
    for seed, scale in ((1, 1.0), (2, 1e30)):
        g = torch.Generator().manual_seed(seed)
        u = (scale * torch.randn(2048, 768, generator=g)).bfloat16().cuda()
        wx = torch.randn(56, 768, generator=g).bfloat16().cuda()
        wdt = torch.randn(768, 24, generator=g).bfloat16().cuda()
        aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib)          # (1e30 operands: infinities and NaNs in its tiles and slabs)
        dx, du = XC.check_xdt_bwd_w(lib, "cuda", 145, 768, torch.bfloat16, 0, *XC.SMALL)
        res.append((dx.clone(), du.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_xdt_tm_bwd_small_nan_tails(lib, dtype):
    """W_dt^T and W_x^T are leading blocks of larger NaN-filled buffers: the rows behind W_dt^T's 24th and the columns behind every W_x^T
    row's 56th are poison.  Finite and within the rule -- an unmasked half fragment multiplies them in"""
    XC.check_xdt_bwd_w(lib, "cuda", 145, 768, dtype, 0, *XC.SMALL, nan_tails=True)
    XC.check_xdt_bwd_w(lib, "cuda", 33, 256, dtype, 8, *XC.SMALL, nan_tails=True)


@pytest.mark.parametrize("t", [513, 2305])
@pytest.mark.parametrize("k,pad_x", [(24, 32), (56, 0)], ids=["k24_of56", "k56"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gemm_wgrad_small(lib, t, k, pad_x, dtype):
    """d W_dt (768, 24) from the dt block of 56-column x_dbl rows and d W_x^T (768, 56): split by split against fp64, partial-sum mode and
    summed mode agree; the default split count and an uneven one (a ragged and, at 513 tokens, empty splits)"""
    XC.check_gemm_wgrad_w(lib, "cuda", t, 768, k, aum_hip.gemm_wgrad_splits(768, k), dtype, 0, pad_x)
    XC.check_gemm_wgrad_w(lib, "cuda", t, 768, k, 5, dtype, 8, pad_x)


def test_gemm_wgrad_small_nan_neighbours(lib):
    """k = 24 is the leading block of rows whose other columns are NaN (and k = 56 of 64-column rows): the chunks behind the operand's
    width are not multiplied into stored results"""
    g = torch.Generator().manual_seed(11)
    y = torch.randn(513, 768, generator=g).bfloat16().cuda()
    for k, width in ((24, 56), (56, 64)):
        xf = torch.full((513, width), float("nan"), dtype=torch.bfloat16, device="cuda")
        xf[:, :k] = torch.randn(513, k, generator=g).bfloat16().cuda()
        out = aum_hip.gemm_wgrad(y, xf[:, :k], lib=lib)
        ref = y.double().t() @ xf[:, :k].double()
        assert bool(torch.isfinite(out).all()) and KC.rel_err(KC.N(out), ref.cpu().numpy()) < 1e-5, k


def _block_pair(monkeypatch, btype, dtype, dout_scale=1.0):
    """one Mamba block of AuM-Small's width (d_model 384: d_inner 768, dt_rank 24) on the token-major kernels under autocast, forward and
    backward from the same inputs: as dispatched, then with the x/dt backward on the library path (ssi._XDT_BWD_HIP False)"""
    import mamba_ssm.ops.selective_scan_interface as ssi
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(5)
    m = Mamba(384, bimamba_type=btype).cuda()
    assert (m.d_inner, m.dt_rank, m.d_state) == (768, 24, 16)
    x = 0.5 * torch.randn(2, 65, 384, device="cuda")
    w = dout_scale * torch.randn(2, 65, 384, device="cuda") / 100
    monkeypatch.setattr(ssi, "_TM_MIN_WAVES", 0)          # (2 x 12 x 2 waves: the dispatch would pick the channel-major block at this batch)
    calls = []
    real = aum_hip.xdt_tm_bwd
    monkeypatch.setattr(aum_hip, "xdt_tm_bwd", lambda *a, **k: (calls.append(a[3].shape), real(*a, **k))[1])
    res = []
    for hip in (True, False):
        if not hip:
            monkeypatch.setattr(ssi, "_XDT_BWD_HIP", False)
        n0 = len(calls)
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            y = m(xi)
        (y.float() * w).sum().backward()
        torch.cuda.synchronize()
        if hip:
            assert len(calls) > n0 and all(s == (768, 56) for s in calls), "the block did not take aum_xdt_tm_bwd at AuM-Small's width"
        else:
            assert len(calls) == n0, "the library path called the kernel"
        res.append(dict(dx=xi.grad.float().clone(), **{k: p_.grad.float().clone() for k, p_ in m.named_parameters()}))
    for k in res[0]:
        assert bool(torch.isfinite(res[0][k]).all()) and bool(torch.isfinite(res[1][k]).all()), k
        e = KC.rel_err(KC.N(res[0][k]), KC.N(res[1][k]))
        print(f"block {btype} {dtype} {k}: kernel vs library path rel_err {e:.3e} (bound {4 * KC.TOL_BF16:.1e})")
        assert e < 4 * KC.TOL_BF16, (k, e)


@pytest.mark.parametrize("btype", ["v1", "v2"])
def test_block_small_kernel_vs_library_bf16(monkeypatch, btype):
    _block_pair(monkeypatch, btype, torch.bfloat16)


def test_block_small_kernel_vs_library_fp16_scaled(monkeypatch):
    """the fp16 recipe: a GradScaler-sized dout (x 1024)"""
    _block_pair(monkeypatch, "v2", torch.float16, dout_scale=1024.0)
