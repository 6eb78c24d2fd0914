"""GPU: the activated delta of the token-major block -- aum_xdt_tm_fwd writing softplus(raw + dt_bias) once (AUM_XDT_DELTA_SOFTPLUS) and the
token-major scans reading it as it is (AUM_SCAN_DELTA_ACTIVATED) -- against fp64 references, and the AuM-Base blocks with the switch on
and off.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

import aum_hip
import cases
import delta_act_checks as DA
import kernel_checks as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()


def _xdt_activated(lib, ntok, dim, rank, ncols, dtype, with_bias=True, seed=0):
    g = torch.Generator().manual_seed(seed + ntok + dim)
    u = torch.randn(ntok, dim, generator=g).to(dtype).cuda()
    wx = (torch.randn(ncols, dim, generator=g) / dim ** 0.5).to(dtype).cuda()
    wdt = (torch.randn(dim, rank, generator=g) * 2 / rank ** 0.5).to(dtype).cuda()
    bias = None
    if with_bias:           # dt_bias init range (-7 .. -2), and channels past the softplus threshold / at 0
        bias = torch.empty(dim).uniform_(-7.0, -2.0, generator=g)
        bias[::97] = 25.0
        bias[5::101] = 0.0
        bias = bias.cuda()
    x_dbl, delta = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib, delta_bias=bias, delta_softplus=True)
    x0, raw = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib)
    assert torch.equal(x_dbl, x0)                                             # x_dbl does not depend on the mode
    pre = x_dbl[:, :rank].double() @ wdt.double().t()
    if bias is not None:
        pre = pre + bias.double()
    ref = torch.where(pre > 20, pre, torch.log1p(torch.exp(pre.clamp(max=20))))
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    # one 16-bit rounding of the fp32 value (relative), the fp32 accumulation and softplus (a few fp32 ulps), fp16 subnormals (absolute)
    err = (delta.double() - ref).abs()
    bound = (ulp + 2.0 ** -18) * ref.abs() + 2.0 ** -24
    assert bool((err <= bound).all()), (ntok, dim, str(dtype), (err / bound).max().item())
    x2, d2 = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib, delta_bias=bias, delta_softplus=True)
    assert torch.equal(x_dbl, x2) and torch.equal(delta, d2)                  # bitwise repeatable
    return delta, raw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_xdt_activated_headline_shape(lib, dtype):
    """the bench's launch: 64 x 513 tokens, d_inner 1536, dt_rank 48"""
    _xdt_activated(lib, 64 * 513, 1536, 48, 80, dtype)


@pytest.mark.parametrize("shape", [(145, 768, 48, 80), (1, 256, 48, 80), (300, 512, 24, 56), (2053, 1536, 48, 80)], ids=str)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_xdt_activated_small(lib, shape, dtype):
    """ragged token counts (a partial last wave), AuM-Small's 56-column rows, no bias"""
    _xdt_activated(lib, *shape, dtype)
    _xdt_activated(lib, *shape, dtype, with_bias=False, seed=1)


ACT_CASES = [c for c in cases.SCAN_TM_CASES if c[5] and c[8]]           # with z and delta_softplus: the block's scans


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scan_tm_activated(lib, case, mode, dtype):
    DA.check_scan_tm_activated(lib, "cuda", case, dtype, reverse=(mode == "rev"), bidir=(mode == "bidir"))


@pytest.mark.parametrize("case", [c for c in ACT_CASES if c[3] >= 9], ids=lambda c: c[0])       # time segments: rows of two blocks or more
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scan_tm_activated_segments(lib, case, mode, dtype):
    DA.check_scan_tm_activated(lib, "cuda", case, dtype, reverse=(mode == "rev"), bidir=(mode == "bidir"), segments=3)


@pytest.mark.parametrize("segments", [1, 4])
def test_scan_tm_activated_headline_grid_b64(lib, segments):
    """the Fo-Bi scan pair at the bench's launch (64 x 513, d_inner 1536, bf16, the block's row layouts): the activated mode on
    delta = bf16(softplus(raw + bias)) against (i) the fp64 oracle on sampled rows and (ii) the in-scan mode on raw + bias over whole
    tensors, every output and gradient (the two differ by where the one 16-bit rounding of delta happens)"""
    torch.manual_seed(5)
    Bsz, L, E, N, R = 64, 513, 1536, 16, 48
    bf = lambda t: t.bfloat16()
    xz = bf(torch.randn(Bsz, L, 2 * E, device="cuda"))
    u, z = xz[:, :, :E], xz[:, :, E:]
    raw = bf(0.5 * torch.randn(Bsz, L, E, device="cuda"))
    x_dbl = bf(torch.randn(Bsz, L, R + 2 * N, device="cuda"))
    Bm, Cm = x_dbl[:, :, R:R + N], x_dbl[:, :, R + N:]
    A = -torch.arange(1, N + 1, device="cuda", dtype=torch.float32).repeat(E, 1) * (1 + 0.1 * torch.rand(E, N, device="cuda"))
    A_b = A * (1 + 0.1 * torch.rand(E, N, device="cuda"))
    D, bias = torch.rand(E, device="cuda") + 0.5, torch.full((E,), -4.0, device="cuda") + torch.rand(E, device="cuda")
    dout = bf(torch.randn(Bsz, L, E, device="cuda"))
    act = bf(torch.nn.functional.softplus(raw.double() + bias.double()))
    res = {}
    for mode, dl in (("in_scan", raw), ("activated", act)):
        ck = aum_hip.scan_tm_ckpt(Bsz, L, E, N, True, "cuda", dtype=torch.bfloat16)
        out, pre = aum_hip.scan_tm_fwd(u, dl, A, Bm, Cm, D, z, bias, True, A_b=A_b, want_out_pre=True, ckpt=ck, lib=lib, segments=segments,
                                       delta_activated=mode == "activated")
        g = aum_hip.scan_tm_bwd(u, dl, A, Bm, Cm, D, z, bias, dout, pre, ck, True, A_b=A_b, lib=lib, segments=segments,
                                delta_activated=mode == "activated")
        res[mode] = dict(out=out, out_pre=pre, **{k: g[k] for k in ("du", "ddelta", "dz", "dBC", "dA", "dA_b", "dD", "ddelta_bias")})
        for k, v in res[mode].items():
            assert bool(torch.isfinite(v).all()), (mode, k)
    rel = lambda a, b: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
    for k in res["in_scan"]:
        assert rel(res["activated"][k], res["in_scan"][k]) < 2e-2, (k, rel(res["activated"][k], res["in_scan"][k]))
    f = lambda t: t.float().cpu().numpy()
    zero = torch.zeros_like(bias)
    for b, es in {0: [0, 63, 64], 37: [767, 768], 63: [1535]}.items():
        ro, rp, gr = KC._tm_rows_vs_oracle(KC.O, b, es, u, act, z, Bm, Cm, A, A_b, D, zero, dout, softplus=False)
        sl = lambda t: f(t[b][:, es]).T[None]
        assert KC.rel_err(sl(res["activated"]["out"]), ro) < KC.TOL_BF16
        assert KC.rel_err(sl(res["activated"]["out_pre"]), rp) < KC.TOL_BF16
        sig = 1.0 / (1.0 + np.exp(-(sl(raw).astype(np.float64) + f(bias)[es][None, :, None])))
        for k, ref in (("du", gr["du"]), ("dz", gr["dz"]), ("ddelta", gr["ddelta"] * sig)):
            assert KC.rel_err(sl(res["activated"][k]), ref) < 4 * KC.TOL_BF16, (k, b)


def _block_ab(monkeypatch, btype, dtype, batch=16):
    """one AuM-Base block (768, Fo-Bi = v1 / Bi-Bi = v2) forced onto the token-major kernels, under autocast, switch on and off"""
    import mamba_ssm.ops.selective_scan_interface as ssi
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(4)
    m = Mamba(768, bimamba_type=btype).cuda()
    x = 0.5 * torch.randn(batch, 513, 768, device="cuda")
    w = torch.randn(batch, 513, 768, device="cuda") / 100
    monkeypatch.setattr(ssi, "_TM_MIN_WAVES", 0)
    res = []
    for on in (True, False):
        monkeypatch.setattr(ssi, "_DELTA_IN_XDT", on)
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            y = m(xi)
        (y.float() * w).sum().backward()
        res.append((y.float().detach(), xi.grad.clone(), {k: p_.grad.clone() for k, p_ in m.named_parameters()}))
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    assert not torch.equal(res[0][0], res[1][0])                          # the switch changes the path
    assert rel(res[0][0], res[1][0]) < 2e-2 and rel(res[0][1], res[1][1]) < 2e-2
    for k in res[0][2]:
        assert bool(torch.isfinite(res[0][2][k]).all()), k
        assert rel(res[0][2][k], res[1][2][k]) < 3e-2, k
    return res


@pytest.mark.parametrize("btype", ["v1", "v2"])
def test_block_activated_vs_in_scan_bf16(monkeypatch, btype):
    res = _block_ab(monkeypatch, btype, torch.bfloat16)
    assert any("dt_proj.bias" in k for k in res[0][2])                     # the bias gradient comes from the activated path's scan


def test_block_activated_vs_in_scan_fp16(monkeypatch):
    _block_ab(monkeypatch, "v1", torch.float16, batch=8)
