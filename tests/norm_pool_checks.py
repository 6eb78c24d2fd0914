"""Add + RMSNorm + mean over a sample's tokens (aum_rmsnorm_pool_fwd / _bwd) and the operator on top of it; shared by
tests/test_norm_pool.py (CPU, lane-array library) and tests/test_gpu_norm_pool.py (device library).

The kernels compute, for sample s of `per` rows:

  forward    z = x + residual;  rstd = 1 / sqrt(mean(z^2) + eps);  y = round(z * rstd * weight)  -- aum_rmsnorm_fwd's rows, not stored;
             pooled[s] = round(sum_r y[s, r] / per), the sum in fp32 over the ROUNDED rows in a fixed order
  backward   g[s] = round(dpooled[s] / per);  dx, dresidual_in of every row = aum_rmsnorm_bwd's for dy = g[s];  dweight = sum_rows g * xhat

Bounds (none comes from what the kernels return):
  pooled     against m = the fp64 mean of aum_rmsnorm_fwd's own y rows: half an ulp of the output dtype at |m| (the one final rounding) plus
             per * 2^-23 * mean|y| (fp32 accumulation of per terms and one fp32 division: at most per + 1 roundings of 2^-24 of a running
             sum that mean|y| * per bounds, divided by per -- stated with the factor 2 of slack the issue gives)
  pooled     against the fp64 statement of the whole expression: 1e-2 of its largest element, drop_path_checks.py's bar for a 16-bit y
  dweight    against the fp64 sum of the same per-row terms g * xhat (xhat = residual_out * rstd in fp64 from the kernel's own saved
             tensors): the terms are formed in fp32 (2 roundings each: xhat, the product) and added in fp32 in some order over `rows` terms:
             (rows + 2) * 2^-24 * sum|terms|, again doubled to 2^-23
Shapes are the issue's: one row, the double-cls pair, 9 rows (no multiple of the 4 rows of a wave), 65 and 514 (three and seventeen 32-row
chunks: the second launch), at 192 and 768 columns (one and two 512-column chunks, both ragged)."""
import numpy as np
import pytest
import torch

import aum_hip
from conftest import rel_err
from drop_path_checks import Framed, bits, f64, launch, same_bits

COLS = [192, 768]
SHAPES = [(1, 1), (3, 2), (2, 9), (2, 65), (1, 514)]
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -4


def case_id(c):
    return f"s{c[0]}_p{c[1]}"


def dtype_id(d):
    return str(d).split(".")[-1]


def inputs(case, cols, dtype, dev, seed=0):
    samples, per = case
    g = torch.Generator().manual_seed(1000 * seed + 100 * samples + per + cols)
    rows = samples * per
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"x": r(rows, cols).to(dtype), "residual": 1.5 * r(rows, cols), "weight": 1.0 + 0.3 * r(cols), "dpooled": r(samples, cols).to(dtype)}
    return {k: v.to(dev) for k, v in t.items()}


def ulp_half(m, dtype):
    """half an ulp of `dtype` at |m| (fp64 array); subnormal range: half the smallest step"""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(m), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - mant)


def run_fwd(lib, t, per):
    return aum_hip.rmsnorm_pool_fwd(t["x"], t["weight"], t["residual"], per, EPS, lib=lib)


def broadcast_g(t, per):
    """g = round(dpooled / per), one row per row of the sample"""
    g = (t["dpooled"].float() / per).to(t["dpooled"].dtype)
    return g.repeat_interleave(per, dim=0).contiguous()


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def check_forward(lib, dev, case, cols, dtype):
    samples, per = case
    t = inputs(case, cols, dtype, dev)
    pooled, rstd, res_out = run_fwd(lib, t, per)
    y, rstd0, res0 = aum_hip.rmsnorm_fwd(t["x"], t["weight"], t["residual"], EPS, lib=lib)
    same_bits(rstd, rstd0, "rstd")
    same_bits(res_out, res0, "residual_out")
    yy = f64(y).reshape(samples, per, cols)
    m = yy.mean(axis=1)
    bound = ulp_half(m, dtype) + per * 2.0 ** -23 * np.abs(yy).mean(axis=1)
    err = np.abs(f64(pooled) - m)
    print(f"{case_id(case)} c{cols} {dtype_id(dtype)} pooled: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    z = f64(t["x"]) + f64(t["residual"])
    ref = (z / np.sqrt((z ** 2).mean(axis=1, keepdims=True) + EPS) * f64(t["weight"])).reshape(samples, per, cols).mean(axis=1)
    e = rel_err(f64(pooled), ref)
    print(f"  against the fp64 expression: {e:.3e}")
    assert e < 1e-2, e
    # eval: nothing saved, the same pooled bits
    p2, r2, o2 = aum_hip.rmsnorm_pool_fwd(t["x"], t["weight"], t["residual"], per, EPS, save=False, lib=lib)
    assert r2 is None and o2 is None
    same_bits(p2, pooled, "pooled without the saved tensors")


# ---- backward --------------------------------------------------------------------------------------------------------------------
def check_backward(lib, dev, case, cols, dtype):
    samples, per = case
    t = inputs(case, cols, dtype, dev, seed=1)
    _, rstd, res_out = run_fwd(lib, t, per)
    dx, dw, dres = aum_hip.rmsnorm_pool_bwd(t["dpooled"], res_out, t["weight"], rstd, per, lib=lib)
    g = broadcast_g(t, per)
    dx0, dw0, dres0 = aum_hip.rmsnorm_bwd(g, res_out, t["weight"], rstd, None, True, x_dtype=dtype, lib=lib)
    same_bits(dx, dx0, "dx")
    same_bits(dres, dres0, "dresidual_in")
    assert dres.dtype == torch.float32 and dx.dtype == dtype
    terms = f64(g) * (f64(res_out) * f64(rstd)[:, None])
    bound = (samples * per + 2) * 2.0 ** -23 * np.abs(terms).sum(axis=0) + 1e-30
    err = np.abs(f64(dw) - terms.sum(axis=0))
    print(f"{case_id(case)} c{cols} {dtype_id(dtype)} dweight: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ---- isolation -------------------------------------------------------------------------------------------------------------------
def check_isolation(lib, dev, case, cols, dtype):
    """sample 0 alone, in the batch, behind other samples and next to a NaN sample: the same pooled and dx bits"""
    samples, per = case
    t = inputs(case, cols, dtype, dev, seed=2)
    extra = inputs((2, per), cols, dtype, dev, seed=3)

    def go(order, poison=None):
        """order: (source, sample) pairs making up the batch"""
        pick = lambda k, rows: torch.cat([(t if src == "t" else extra)[k][i * rows:(i + 1) * rows] for src, i in order]).clone()
        u = {"x": pick("x", per), "residual": pick("residual", per), "dpooled": pick("dpooled", 1), "weight": t["weight"]}
        if poison is not None:
            u["x"][poison * per:(poison + 1) * per] = float("nan")
            u["dpooled"][poison] = float("nan")
        pooled, rstd, res_out = run_fwd(lib, u, per)
        dx, _, dres = aum_hip.rmsnorm_pool_bwd(u["dpooled"], res_out, u["weight"], rstd, per, lib=lib)
        return pooled, dx, dres

    alone = go([("t", 0)])
    for what, order, at, poison in (("whole batch", [("t", i) for i in range(samples)], 0, None),
                                    ("behind two other samples", [("e", 0), ("e", 1), ("t", 0)], 2, None),
                                    ("between samples, one of them NaN", [("e", 1), ("t", 0), ("e", 0)], 1, 0)):
        got = go(order, poison)
        same_bits(got[0][at:at + 1], alone[0], f"pooled: {what}")
        same_bits(got[1][at * per:(at + 1) * per], alone[1], f"dx: {what}")
        same_bits(got[2][at * per:(at + 1) * per], alone[2], f"dresidual_in: {what}")
        assert bool(torch.isfinite(got[0][at].float()).all())
    again = go([("t", 0)])
    same_bits(again[0], alone[0], "pooled run to run")


# ---- memory and arguments: the C ABI on buffers of the test's own ------------------------------------------------------------------
def framed(lib, case, cols, dtype, dev):
    samples, per = case
    rows = samples * per
    nchunk = int(lib.c.aum_rmsnorm_pool_partial_rows(per))
    assert nchunk == (per + 31) // 32
    n_part = int(lib.c.aum_rmsnorm_bwd_partial_rows(rows, cols, 0))
    return {"pooled": Framed(samples, cols, dtype, dev), "residual_out": Framed(rows, cols, torch.float32, dev),
            "rstd": Framed(1, rows, torch.float32, dev), "pool_partial": Framed(samples * nchunk, cols, torch.float32, dev, pad=0),
            "dx": Framed(rows, cols, dtype, dev), "dresidual_in": Framed(rows, cols, torch.float32, dev),
            "dweight_partial": Framed(n_part, cols, torch.float32, dev, pad=0)}


def raw_args(t, case, cols, out):
    samples, per = case
    p, dt = aum_hip._ptr, aum_hip._DT
    f, b = aum_hip.NormPoolArgs(), aum_hip.NormPoolArgs()
    for q in (f, b):
        a = q.base
        a.weight, a.rows, a.cols, a.eps = p(t["weight"]), samples * per, cols, EPS
        a.x_dtype = a.y_dtype = dt[t["x"].dtype]
        a.res_dtype = dt[torch.float32]
        q.rows_per_sample = per
    a = f.base
    a.x, a.residual, a.residual_out, a.rstd_out = p(t["x"]), p(t["residual"]), p(out["residual_out"].view), p(out["rstd"].view)
    a.row_stride_x, a.row_stride_res, a.row_stride_res_out = t["x"].stride(0), t["residual"].stride(0), out["residual_out"].view.stride(0)
    f.pooled, f.pool_partial, f.row_stride_pooled = p(out["pooled"].view), p(out["pool_partial"].view), out["pooled"].view.stride(0)
    a = b.base
    a.x, a.rstd_in, a.dx, a.dresidual_in = p(out["residual_out"].view), p(out["rstd"].view), p(out["dx"].view), p(out["dresidual_in"].view)
    a.dweight_partial = p(out["dweight_partial"].view)
    a.row_stride_x, a.row_stride_dx, a.row_stride_dres_in = (out[k].view.stride(0) for k in ("residual_out", "dx", "dresidual_in"))
    b.dpooled, b.row_stride_dpooled = p(t["dpooled"]), t["dpooled"].stride(0)
    return f, b


def check_guards(lib, dev, case, cols, dtype):
    samples, per = case
    t = inputs(case, cols, dtype, dev, seed=4)
    out = framed(lib, case, cols, dtype, dev)
    f, b = raw_args(t, case, cols, out)
    assert launch(lib, lib.c.aum_rmsnorm_pool_fwd, f, t["x"]) == 0
    assert launch(lib, lib.c.aum_rmsnorm_pool_bwd, b, t["x"]) == 0
    for k, fr in out.items():
        fr.intact(f"{k} {case_id(case)} c{cols}")
    nchunk = (per + 31) // 32
    part = out["pool_partial"].view
    if nchunk == 1:
        assert bool(torch.isnan(part).all()), "a one-chunk sample needs no partial rows and writes none"
    else:
        assert bool(torch.isfinite(part).all()), "every partial row holds a chunk's sums"
    n_sums = int(lib.c.aum_rmsnorm_bwd_partial_rows(samples * per, cols, 0))
    assert bool(torch.isfinite(out["dweight_partial"].view[:n_sums]).all())
    pooled, rstd, res_out = run_fwd(lib, t, per)
    dx, _, dres = aum_hip.rmsnorm_pool_bwd(t["dpooled"], res_out, t["weight"], rstd, per, lib=lib)
    for k, ref in (("pooled", pooled), ("residual_out", res_out), ("dx", dx), ("dresidual_in", dres)):
        same_bits(out[k].view.contiguous(), ref, k)
    same_bits(out["rstd"].view[0].contiguous(), rstd, "rstd")


def check_argument_rules(lib, dev):
    case, cols, dtype = (2, 65), 192, torch.bfloat16
    t = inputs(case, cols, dtype, dev, seed=5)
    fwd_out, bwd_out = ("pooled", "residual_out", "rstd", "pool_partial"), ("dx", "dresidual_in", "dweight_partial")

    def refused(which, edit, want):
        out = framed(lib, case, cols, dtype, dev)
        f, b = raw_args(t, case, cols, out)
        if which == "bwd":
            assert launch(lib, lib.c.aum_rmsnorm_pool_fwd, f, t["x"]) == 0
        q = f if which == "fwd" else b
        edit(q)
        fn = lib.c.aum_rmsnorm_pool_fwd if which == "fwd" else lib.c.aum_rmsnorm_pool_bwd
        assert launch(lib, fn, q, t["x"]) == want, (which, want)
        for k in (fwd_out if which == "fwd" else bwd_out):
            out[k].untouched(k)

    for which in ("fwd", "bwd"):
        refused(which, lambda q: setattr(q.base, "x", None), E_NULL)
        refused(which, lambda q: setattr(q.base, "weight", None), E_NULL)
        refused(which, lambda q: setattr(q, "rows_per_sample", 4), E_SHAPE)             # 130 rows
        refused(which, lambda q: setattr(q, "rows_per_sample", 0), E_SHAPE)
        refused(which, lambda q: setattr(q.base, "cols", 196), E_UNSUPPORTED)           # not a multiple of 8
        refused(which, lambda q: setattr(q.base, "cols", 2056), E_UNSUPPORTED)          # past the vectorised kernels
        refused(which, lambda q: setattr(q.base, "res_dtype", 1), E_UNSUPPORTED)        # a 16-bit residual stream
        refused(which, lambda q: (setattr(q.base, "x_dtype", 0), setattr(q.base, "y_dtype", 0)), E_UNSUPPORTED)
        refused(which, lambda q: setattr(q.base, "flags", 2), E_UNSUPPORTED)
        refused(which, lambda q: setattr(q, "reserved", 1), E_UNSUPPORTED)
    refused("fwd", lambda q: setattr(q.base, "residual", None), E_NULL)
    refused("fwd", lambda q: setattr(q, "pooled", None), E_NULL)
    refused("fwd", lambda q: setattr(q, "pool_partial", None), E_NULL)                  # 65 rows: three chunks need their rows
    refused("fwd", lambda q: setattr(q.base, "rstd_out", None), E_UNSUPPORTED)          # both saved tensors or neither
    for k in ("dpooled",):
        refused("bwd", lambda q: setattr(q, k, None), E_NULL)
    for k in ("rstd_in", "dx", "dresidual_in", "dweight_partial"):
        refused("bwd", lambda q: setattr(q.base, k, None), E_NULL)
    assert lib.c.aum_rmsnorm_pool_fwd(None, None) == E_NULL and lib.c.aum_rmsnorm_pool_bwd(None, None) == E_NULL
    assert lib.c.aum_rmsnorm_pool_partial_rows(0) == 0 and lib.c.aum_rmsnorm_pool_partial_rows(32) == 1
    assert lib.c.aum_rmsnorm_pool_partial_rows(33) == 2
    # the binding refuses the same before any launch
    with pytest.raises(ValueError):
        aum_hip.rmsnorm_pool_fwd(t["x"], t["weight"], t["residual"], 4, EPS, lib=lib)
    with pytest.raises(ValueError):
        aum_hip.rmsnorm_pool_fwd(t["x"], t["weight"], None, 65, EPS, lib=lib)
    with pytest.raises(RuntimeError):
        aum_hip.rmsnorm_pool_fwd(t["x"].float(), t["weight"], t["residual"], 65, EPS, lib=lib)
    with pytest.raises(RuntimeError):
        aum_hip.rmsnorm_pool_fwd(t["x"][:, :100], t["weight"][:100], t["residual"][:, :100], 65, EPS, lib=lib)


# ---- operator --------------------------------------------------------------------------------------------------------------------
def check_operator(dev, case, cols, dtype):
    """rms_norm_pool_fn against rms_norm_pool_ref under autograd: the twin differentiates through the 16-bit rounding of y as torch does
    (straight through), the kernel's g is the rounded dpooled / per: both are 16-bit statements of the same gradient -> the 1e-2 bar"""
    from mamba_ssm.ops.triton.layernorm import rms_norm_pool_fn, rms_norm_pool_ref
    samples, per = case
    t = inputs(case, cols, dtype, dev, seed=6)
    dl = t["dpooled"].float()

    def go(fn, flat):
        x, r, w = (t[k].clone().requires_grad_(True) for k in ("x", "residual", "weight"))
        xs, rs = (x, r) if flat else (x.reshape(samples, per, cols), r.reshape(samples, per, cols))
        out = fn(xs, w, rs, EPS, rows_per_sample=per if flat else None)
        (out.float() * dl).sum().backward()
        return {"pooled": out.detach(), "dx": x.grad, "dresidual": r.grad, "dweight": w.grad}

    got, ref = go(rms_norm_pool_fn, False), go(rms_norm_pool_ref, False)
    assert got["pooled"].shape == (samples, cols) and got["pooled"].dtype == dtype
    assert got["dx"].dtype == dtype and got["dresidual"].dtype == torch.float32
    for k in got:
        e = rel_err(f64(got[k]), f64(ref[k]))
        print(f"operator {case_id(case)} c{cols} {dtype_id(dtype)} {k}: {e:.3e}")
        assert e < 1e-2, (k, e)
    flat = go(rms_norm_pool_fn, True)
    for k in got:
        same_bits(flat[k], got[k], f"{k}: (B L, D) with rows_per_sample")
    with torch.no_grad():
        same_bits(rms_norm_pool_fn(t["x"].reshape(samples, per, cols), t["weight"], t["residual"].reshape(samples, per, cols), EPS), got["pooled"],
                  "no grad mode")
    with pytest.raises(ValueError):
        rms_norm_pool_fn(t["x"], t["weight"], t["residual"], EPS)                     # 2-D without rows_per_sample
    with pytest.raises(ValueError):
        rms_norm_pool_fn(t["x"].reshape(samples, per, cols), t["weight"], None, EPS)


def check_operator_grad_home(dev):
    from mamba_ssm.ops import selective_scan_interface as ssi
    from mamba_ssm.ops.triton.layernorm import rms_norm_pool_fn
    g = torch.Generator().manual_seed(8)
    cols, SENTINEL = 768, 7.0
    x, r = torch.randn(3, 5, cols, generator=g).bfloat16().to(dev), torch.randn(3, 5, cols, generator=g).to(dev)
    w = torch.nn.Parameter((1 + 0.3 * torch.randn(cols, generator=g)).to(dev))
    rms_norm_pool_fn(x, w, r).float().sum().backward()
    want = w.grad.clone()
    w.grad = None
    bucket = torch.full((cols + 16,), SENTINEL, device=dev)
    home = bucket[8:8 + cols]
    w._aum_grad_home = home
    hits = ssi.HOME_HITS[0]
    rms_norm_pool_fn(x, w, r).float().sum().backward()
    assert ssi.HOME_HITS[0] == hits + 1
    same_bits(home, want, "the gradient in its home")
    assert w.grad is not None and w.grad.data_ptr() == home.data_ptr()
    assert bool((bucket[:8] == SENTINEL).all()) and bool((bucket[8 + cols:] == SENTINEL).all())


def check_cpu_twin_without_library(monkeypatch):
    """CPU tensors and no library that takes them: the function is its twin"""
    from mamba_ssm.ops.triton.layernorm import rms_norm_pool_fn, rms_norm_pool_ref
    monkeypatch.setattr(aum_hip, "_product", None)
    monkeypatch.setattr(aum_hip, "rmsnorm_pool_fwd", lambda *a, **k: pytest.fail("a kernel was launched"))
    t = inputs((2, 9), 192, torch.bfloat16, "cpu", seed=9)
    x, r = t["x"].reshape(2, 9, 192), t["residual"].reshape(2, 9, 192)
    same_bits(rms_norm_pool_fn(x, t["weight"], r, EPS), rms_norm_pool_ref(x, t["weight"], r, EPS), "twin")
