"""Width-parameterised twins of kernel_checks.check_xdt_bwd / check_gemm_wgrad for the AuM-Small widths of aum_xdt_tm_bwd (dx_dbl of 56
columns, dt_rank 24) and of the skinny aum_gemm_wgrad (k = 24 / 56).  Same rules, same bounds as the originals; (R, C) and the operands
are arguments so that one body serves the host build (test_xdt_small.py) and the device library (test_gpu_xdt_small.py)."""
import torch

import aum_hip
from conftest import rel_err

SMALL = (24, 56)        # (dt_rank, dt_rank + 2 d_state) of AuM-Small
BASE = (48, 80)


def ulp_of(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def xdt_bwd_operands(dev, ntok, dim, dtype, R, C, pad=0, nan_tails=False):
    """the operands of check_xdt_bwd at widths (R, C).  nan_tails: wx_t and wdt_t are the LEADING part of larger buffers whose tails are
    NaN -- what lies behind the last row of W_dt^T and behind the last column of W_x^T's last row is poison, not zeros"""
    g = torch.Generator().manual_seed(ntok * 5 + dim + R)
    ddf = torch.randn(ntok, dim + pad, generator=g).to(dtype).to(dev)
    duf = torch.randn(ntok, dim + pad, generator=g).to(dtype).to(dev)
    dbc = torch.randn(ntok, C - R, generator=g).to(dev)
    wdt_t = (torch.randn(R, dim, generator=g) / dim ** 0.5).to(dtype).to(dev)
    wx_t = (torch.randn(dim, C, generator=g) / C ** 0.5).to(dtype).to(dev)
    if nan_tails:
        big_dt = torch.full((R + 40, dim + 8), float("nan"), dtype=dtype, device=dev)
        big_dt[:R, :dim] = wdt_t
        wdt_t = big_dt[:R, :dim]
        # rows of pitch C + 8: the eight columns a padded K-step would take from behind EVERY row's end are NaN, and so are the rows behind
        big_x = torch.full((dim + 64, C + 8), float("nan"), dtype=dtype, device=dev)
        big_x[:dim, :C] = wx_t
        wx_t = big_x[:dim, :C]
    return dict(ddf=ddf, duf=duf, ddelta=ddf[:, :dim], du=duf[:, :dim], dbc=dbc, wdt_t=wdt_t, wx_t=wx_t)


def assert_xdt_bwd(op, dx, du_in, tail_in, dtype, R, C, tag=()):
    """the rules of check_xdt_bwd on a finished call: dx = the returned dx_dbl, op["du"] updated in place from du_in"""
    ntok, dim = op["ddelta"].shape
    ulp = ulp_of(dtype)
    assert dx.shape == (ntok, C) and bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(op["du"].float()).all()), ("finite",) + tuple(tag)
    ref_r = op["ddelta"].double().cpu() @ op["wdt_t"].double().cpu().t()
    er = (dx[:, :R].double().cpu() - ref_r).abs().max().item()
    print(f"xdt_bwd {tuple(tag)} R={R} C={C} ntok={ntok} dim={dim}: dt block err {er:.3e} (bound {1.01 * ulp * ref_r.abs().max().item():.3e})")
    assert er <= 1.01 * ulp * ref_r.abs().max().item(), ("dx_dbl dt block", ntok, dim, er) + tuple(tag)
    assert torch.equal(dx[:, R:].cpu(), op["dbc"].to(dtype).cpu()), ("dx_dbl B | C block",) + tuple(tag)
    ref_u = du_in + dx.double().cpu() @ op["wx_t"].double().cpu().t()
    eu = (op["du"].double().cpu() - ref_u).abs().max().item()
    print(f"    du err {eu:.3e} (bound {1.01 * ulp * ref_u.abs().max().item():.3e})")
    assert eu <= 1.01 * ulp * ref_u.abs().max().item(), ("du", ntok, dim, eu) + tuple(tag)
    assert torch.equal(op["duf"][:, dim:], tail_in), ("columns behind the du rows were written",) + tuple(tag)


def check_xdt_bwd_w(lib, dev, ntok, dim, dtype, pad=0, R=24, C=56, nan_tails=False):
    """aum_xdt_tm_bwd at (R, C) under the rules of kernel_checks.check_xdt_bwd: dx_dbl[:, :R] within 1.01 ulp x max|ref| of the fp64 product
    of the 16-bit operands, dx_dbl[:, R:] bit-equal to the rounded fp32 dB | dC rows, du within the same bound of fp64 (du_in + the
    kernel's OWN rounded dx_dbl . W_x^T), nothing written behind the du rows.  Returns (dx_dbl, du) for bitwise comparisons."""
    op = xdt_bwd_operands(dev, ntok, dim, dtype, R, C, pad, nan_tails)
    du_in = op["du"].double().cpu()
    tail_in = op["duf"][:, dim:].clone()
    dx = aum_hip.xdt_tm_bwd(op["ddelta"], op["dbc"], op["wdt_t"], op["wx_t"], op["du"], lib=lib)
    assert_xdt_bwd(op, dx, du_in, tail_in, dtype, R, C, tag=("nan_tails",) if nan_tails else ())
    return dx, op["du"]


def check_gemm_wgrad_w(lib, dev, t, n, k, splits, dtype, pad_y=0, pad_x=0):
    """kernel_checks.check_gemm_wgrad, bound for bound (every split's partial tile against the fp64 product of its token range, the summed
    result, bitwise repeatable), plus: the partial-sum mode and the summed mode agree -- the sum of the returned partial tiles in split
    order IS the summed result"""
    g = torch.Generator().manual_seed(t * 7 + n + k + splits)
    y_full = (torch.randn(t, n + pad_y, generator=g)).to(dtype).to(dev)
    x_full = (torch.randn(t, k + pad_x, generator=g)).to(dtype).to(dev)
    y, x = y_full[:, pad_y:], x_full[:, :k]
    assert aum_hip.gemm_wgrad_supported(y, x, splits)
    part = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib, partials=True)
    assert part.shape == (splits, n, k) and part.dtype == torch.float32 and bool(torch.isfinite(part).all())
    chunk = (((t + splits - 1) // splits) + 63) // 64 * 64
    yd, xd = y.double().cpu(), x.double().cpu()
    scale = float((yd.t() @ xd).abs().max()) + 1e-30
    for s_ in range(splits):
        t0, t1 = min(s_ * chunk, t), min((s_ + 1) * chunk, t)
        ref = yd[t0:t1].t() @ xd[t0:t1]
        err = (part[s_].double().cpu() - ref).abs().max().item()
        assert err <= 2e-6 * scale * max(1.0, (t1 - t0) ** 0.5 / 8), (t, n, k, splits, s_, err, scale)      # fp32 accumulation of exact 16-bit products
    total = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib)
    assert total.shape == (n, k)
    assert rel_err(total.double().cpu().numpy(), (yd.t() @ xd).numpy()) < 1e-5
    assert torch.equal(total, aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib))
    assert torch.equal(total, aum_hip.sum_rows(part, lib=lib)), "partial-sum mode and summed mode disagree"
    assert rel_err(total.double().cpu().numpy(), part.double().sum(0).cpu().numpy()) < 1e-6
