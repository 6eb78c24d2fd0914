"""AuM-Small widths of the x_proj / dt_proj backward on the host: the argument rules (csrc/xdt_args.h, csrc/gemm_args.h, shared by the device
library and the tests-only host build) and the binding take dx_dbl rows of 56 columns with dt_rank 24 and the skinny weight-gradient widths
k = 24 / 56; the host build's plain loops hold the contract the device kernel is held to in test_gpu_xdt_small.py."""
import os
import sys

import pytest
import torch

import aum_hip
import xdt_small_checks as XC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("case", [(1, 256, 0), (33, 256, 8)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_xdt_tm_bwd_small_contract(emu, case, dtype):
    """aum_xdt_tm_bwd at (rank, ncols) = (24, 56): dx_dbl rounded once, dB | dC bit-equal, du from the rounded dx_dbl, in place"""
    XC.check_xdt_bwd_w(emu, "cpu", case[0], case[1], dtype, case[2], *XC.SMALL)


def test_xdt_tm_bwd_small_nan_tails(emu):
    """the operands' neighbours in memory are not operands: NaN behind W_dt^T's last row and behind every W_x^T row's last column"""
    XC.check_xdt_bwd_w(emu, "cpu", 33, 256, torch.bfloat16, 8, *XC.SMALL, nan_tails=True)


def _ops(dim, ncols, rank, ntok=5, dbc_cols=32, dtype=torch.bfloat16):
    z = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt)
    return z(ntok, dim), z(ntok, dbc_cols, dt=torch.float32), z(rank, dim), z(dim, ncols), z(ntok, dim)


def test_xdt_tm_bwd_supported_pairs():
    """the binding's rule: (ncols, rank) is (80, 48) or (56, 24), nothing in between"""
    assert aum_hip.xdt_tm_bwd_supported(*_ops(768, 56, 24))
    assert aum_hip.xdt_tm_bwd_supported(*_ops(256, 56, 24, dtype=torch.float16))
    assert aum_hip.xdt_tm_bwd_supported(*_ops(768, 80, 48))
    assert not aum_hip.xdt_tm_bwd_supported(*_ops(768, 80, 24))
    assert not aum_hip.xdt_tm_bwd_supported(*_ops(768, 56, 48))
    assert not aum_hip.xdt_tm_bwd_supported(*_ops(768, 56, 24, dbc_cols=24))
    assert not aum_hip.xdt_tm_bwd_supported(*_ops(384, 56, 24))
    assert not aum_hip.xdt_tm_bwd_supported(*_ops(768, 64, 32))


@pytest.mark.parametrize("pair", [(80, 24), (56, 48), (64, 32), (56, 16)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_xdt_tm_bwd_refused_pair_leaves_du(emu, pair):
    """the C side's xdt_bwd_check refuses every other (ncols, rank) pair before anything is written"""
    ncols, rank = pair
    ntok, dim = 7, 256
    g = torch.Generator().manual_seed(3)
    ddelta, du = torch.randn(ntok, dim, generator=g).bfloat16(), torch.randn(ntok, dim, generator=g).bfloat16()
    dbc = torch.randn(ntok, ncols - rank, generator=g)
    wdt_t, wx_t = torch.randn(rank, dim, generator=g).bfloat16(), torch.randn(dim, ncols, generator=g).bfloat16()
    dx = torch.full((ntok, ncols), 7.0, dtype=torch.bfloat16)
    du_in = du.clone()
    with pytest.raises(RuntimeError):
        aum_hip.xdt_tm_bwd(ddelta, dbc, wdt_t, wx_t, du, lib=emu)
    assert torch.equal(du, du_in)
    a = aum_hip.XdtBwdArgs()
    a.ddelta, a.dbc, a.wdt_t, a.wx_t, a.du, a.dx_dbl = (t.data_ptr() for t in (ddelta, dbc, wdt_t, wx_t, du, dx))
    a.ntok, a.dim, a.rank, a.ncols = ntok, dim, rank, ncols
    a.ldd, a.lddbc, a.ldwdt, a.ldwx, a.ldu, a.ldx, a.dtype = dim, ncols - rank, dim, ncols, dim, ncols, aum_hip.AUM_BF16
    assert emu.c.aum_xdt_tm_bwd(aum_hip.C_byref(a), None) == -4          # AUM_E_UNSUPPORTED
    assert torch.equal(du, du_in) and bool((dx == 7.0).all())
    a.rank, a.ncols, a.lddbc, a.ldwx, a.ldx = 24, 56, 32, 56, 56          # the same struct with the Small pair is taken
    wx2, dbc2, dx2 = wx_t[:, :1].expand(dim, 56).contiguous(), torch.zeros(ntok, 32), torch.zeros(ntok, 56, dtype=torch.bfloat16)
    wd2 = torch.zeros(24, dim, dtype=torch.bfloat16)
    a.dbc, a.wdt_t, a.wx_t, a.dx_dbl = dbc2.data_ptr(), wd2.data_ptr(), wx2.data_ptr(), dx2.data_ptr()
    assert emu.c.aum_xdt_tm_bwd(aum_hip.C_byref(a), None) == 0


def test_gemm_wgrad_supported_small_widths():
    y = torch.zeros(100, 768, dtype=torch.bfloat16)
    for k in (24, 56, 48, 80):
        assert aum_hip.gemm_wgrad_supported(y, torch.zeros(100, k, dtype=torch.bfloat16)), k
    x_dbl = torch.zeros(100, 56, dtype=torch.bfloat16)
    assert aum_hip.gemm_wgrad_supported(y, x_dbl[:, :24])          # the dt block of AuM-Small's x_dbl rows, read in place
    for k in (40, 32, 16, 64):
        assert not aum_hip.gemm_wgrad_supported(y, torch.zeros(100, k, dtype=torch.bfloat16)), k


def test_gemm_wgrad_refuses_k40(emu):
    y, x = torch.zeros(100, 256, dtype=torch.bfloat16), torch.zeros(100, 40, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        aum_hip.gemm_wgrad(y, x, splits=2, lib=emu)
    part = torch.zeros(2, 256, 40)
    a = aum_hip.GemmWArgs()
    a.y, a.x, a.part = y.data_ptr(), x.data_ptr(), part.data_ptr()
    a.t, a.ldy, a.ldx, a.n, a.k, a.splits, a.dtype = 100, 256, 40, 256, 40, 2, aum_hip.AUM_BF16
    assert emu.c.aum_gemm_wgrad(aum_hip.C_byref(a), None) == -4


@pytest.mark.parametrize("case", [(300, 256, 24, 3, 0, 32), (300, 256, 56, 3, 8, 0)], ids=lambda c: "x".join(map(str, c)))
def test_gemm_wgrad_small_contract(emu, case):
    """the host twin of aum_gemm_wgrad at k = 24 (the dt block of 56-column x_dbl rows) and k = 56 against fp64, split by split"""
    XC.check_gemm_wgrad_w(emu, "cpu", *case[:4], torch.bfloat16, *case[4:])
