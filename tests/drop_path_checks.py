"""Stochastic depth inside the add + RMSNorm kernels (aum_rmsnorm_drop_fwd / _bwd) and up through the op layer, the model and the
launcher; shared by tests/test_drop_path.py (CPU, lane-array library) and tests/test_gpu_drop_path.py (device library).

The kernels compute, with s = row_scale[row // rows_per_scale] (one fp32 factor per sample):

  forward    pre = s * x + residual (one fp32 fma; s == 0: pre = residual, x not read);  residual_out = pre;
             rstd = 1 / sqrt(mean(pre^2) + eps);  y = pre * rstd * weight
  backward   xhat = residual_out * rstd;  g = (weight * dy - xhat * mean(xhat * weight * dy)) * rstd + dresidual_out;
             dresidual_in = g;  dx = s * g (s == 0: +0);  dweight = sum over rows of dy * xhat

`reference()` below states exactly that in fp64 numpy.  The bars are the project's: 1e-4 of the fp64 tensor's largest
element for an fp32 tensor, 1e-2 for a 16-bit one.

Shapes are (batch, rows per sample, cols[, generic flag]): the smallest at which each routine can go wrong -- one ragged 512-column chunk
with the sample boundaries inside a backward wave's run of rows, two / three / four chunks, the generic wave form by width and by flag,
and the one-row-per-sample call of the model's final norm.  Every scale vector holds a 0, a 1 and a 1 / 0.9; the two shapes with a batch
of 2 cannot hold three values at once and are run on two vectors that do so together, a 0 in each."""
import numpy as np
import pytest
import torch

import aum_hip
from conftest import rel_err

SHAPES = [(5, 37, 192, False), (3, 11, 768, False), (2, 9, 1536, False), (2, 5, 2048, False), (2, 5, 2056, False), (3, 7, 200, True),
          (4, 1, 768, False)]
DTYPES = [(torch.bfloat16, torch.float32), (torch.float16, torch.float32), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)]
EPS = 1e-5
KEPT = float(np.float32(1.0) / np.float32(0.9))
GUARD, PAD, SENTINEL = 3, 8, 7.0        # guard rows in front of and behind an output, pad columns behind each of its rows, their value


def shape_id(c):
    return f"b{c[0]}_p{c[1]}_c{c[2]}" + ("_generic" if c[3] else "")


def dtype_id(d):
    return "-".join(str(t).split(".")[-1] for t in d)


def bar(dtype):
    return 1e-4 if dtype == torch.float32 else 1e-2


def scale_vectors(batch):
    """the scale vectors of a shape: each holds a 0; one vector holds 0, 1 and 1 / 0.9 where the batch has room for three values"""
    if batch >= 3:
        return [([0.0, KEPT, 1.0, 0.0, KEPT] * batch)[:batch]]
    return [[0.0, KEPT], [1.0, 0.0]]


def inputs(case, dtypes, dev, seed=0):
    """x, residual, weight, dy, dresidual_out of a case: the 16-bit ones already rounded, the same values on every device"""
    batch, per, cols, _ = case
    xd, rd = dtypes
    g = torch.Generator().manual_seed(1000 * seed + batch * 100 + per + cols)
    rows = batch * per
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"x": r(rows, cols).to(xd), "residual": (1.5 * r(rows, cols)).to(rd), "weight": 1.0 + 0.3 * r(cols), "dy": r(rows, cols).to(xd),
         "dres": (0.5 * r(rows, cols)).to(rd)}
    return {k: v.to(dev) for k, v in t.items()}


def f64(t):
    return t.detach().double().cpu().numpy()


def reference(t, scale, per, res_out=None, rstd=None):
    """the formulas of the module docstring in fp64.  Forward from x / residual / weight; the backward takes the saved residual_out and
    rstd it is handed (the kernel's own forward outputs, as the kernel does), or the fp64 ones."""
    s = np.repeat(np.asarray(scale, np.float32).astype(np.float64), per)[:, None]
    x, res, w = f64(t["x"]), f64(t["residual"]), f64(t["weight"])
    pre = np.where(s == 0, res, s * np.where(s == 0, 0.0, x) + res)
    rs = 1.0 / np.sqrt((pre ** 2).mean(axis=1) + EPS)
    out = {"residual_out": pre, "rstd": rs, "y": pre * rs[:, None] * w}
    xs = pre if res_out is None else f64(res_out)
    rb = (rs if rstd is None else f64(rstd))[:, None]
    dy, dres = f64(t["dy"]), f64(t["dres"])
    xhat = xs * rb
    g = (w * dy - xhat * (xhat * w * dy).mean(axis=1, keepdims=True)) * rb + dres
    out.update(dresidual_in=g, dx=s * g, dweight=(dy * xhat).sum(axis=0))
    return out


def run(lib, t, scale, case, dres=True):
    """forward and backward through the binding -> dict of the six outputs plus rstd"""
    _, per, _, generic = case
    s = torch.tensor(scale, dtype=torch.float32, device=t["x"].device)
    y, rstd, res_out = aum_hip.rmsnorm_drop_fwd(t["x"], t["weight"], t["residual"], s, per, EPS, generic=generic, lib=lib)
    dx, dw, dres_in = aum_hip.rmsnorm_drop_bwd(t["dy"], res_out, t["weight"], rstd, s, per, t["dres"] if dres else None, x_dtype=t["x"].dtype,
                                               generic=generic, lib=lib)
    assert dx.data_ptr() != dres_in.data_ptr()          # always two buffers, equal dtypes included
    return {"y": y, "rstd": rstd, "residual_out": res_out, "dx": dx, "dweight": dw, "dresidual_in": dres_in}


def run_unscaled(lib, t, case):
    """the same call on aum_rmsnorm_fwd / _bwd"""
    generic = case[3]
    y, rstd, res_out = aum_hip.rmsnorm_fwd(t["x"], t["weight"], t["residual"], EPS, generic=generic, lib=lib)
    dx, dw, dres_in = aum_hip.rmsnorm_bwd(t["dy"], res_out, t["weight"], rstd, t["dres"], True, x_dtype=t["x"].dtype, generic=generic, lib=lib)
    return {"y": y, "rstd": rstd, "residual_out": res_out, "dx": dx, "dweight": dw, "dresidual_in": dres_in}


def bits(t):
    """the tensor's bit patterns (NaN-safe, signed-zero-aware equality)"""
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(bits(a), bits(b)), what


# ---- 1: against fp64 -------------------------------------------------------------------------------------------------------------
def check_vs_fp64(lib, dev, case, dtypes):
    t = inputs(case, dtypes, dev)
    for scale in scale_vectors(case[0]):
        got = run(lib, t, scale, case)
        ref = reference(t, scale, case[1], got["residual_out"], got["rstd"])
        for k in ("residual_out", "rstd", "y", "dresidual_in", "dx", "dweight"):
            e = rel_err(f64(got[k]), ref[k])
            print(f"{shape_id(case)} {dtype_id(dtypes)} {scale} {k}: {e:.3e}")
            assert e < bar(got[k].dtype), (k, e, scale)


# ---- 2: all-ones scale is the unscaled kernel ------------------------------------------------------------------------------------
def check_ones_is_unscaled(lib, dev, case, dtypes):
    t = inputs(case, dtypes, dev, seed=1)
    got, ref = run(lib, t, [1.0] * case[0], case), run_unscaled(lib, t, case)
    for k in ("y", "rstd", "residual_out", "dx", "dresidual_in", "dweight"):
        same_bits(got[k], ref[k], k)


# ---- 3: zero scale ---------------------------------------------------------------------------------------------------------------
def check_zero_scale(lib, dev, case, dtypes):
    t = inputs(case, dtypes, dev, seed=2)
    batch, per = case[:2]
    got = run(lib, t, [0.0] * batch, case)
    same_bits(got["residual_out"], t["residual"], "residual_out is the residual")
    ref = run_unscaled(lib, dict(t, x=torch.zeros_like(t["x"])), case)
    for k in ("y", "rstd", "dresidual_in", "dweight"):
        same_bits(got[k], ref[k], k)
    assert int(bits(got["dx"]).ne(0).sum()) == 0, "dx of a dropped sample is +0, sign bit included"
    # a dropped sample's x is not read: NaN and inf there change no output bit
    for scale in scale_vectors(batch):
        clean = run(lib, t, scale, case)
        bad = t["x"].clone().view(batch, per, -1)
        for b, s in enumerate(scale):
            if s == 0.0:
                bad[b, :, 0::2] = float("nan")
                bad[b, :, 1::2] = float("inf")
        dirty = run(lib, dict(t, x=bad.view(batch * per, -1)), scale, case)
        for k in clean:
            same_bits(dirty[k], clean[k], f"{k} with NaN / inf in the dropped samples' x")
            assert bool(torch.isfinite(dirty[k].float()).all()), k


# ---- 4: samples do not see each other --------------------------------------------------------------------------------------------
def check_samples_independent(lib, dev, case, dtypes):
    t = inputs(case, dtypes, dev, seed=3)
    batch, per = case[:2]
    for scale in scale_vectors(batch):
        mixed = run(lib, t, scale, case)
        for v in sorted(set(scale)):
            whole = run(lib, t, [v] * batch, case)
            for b in [b for b, s in enumerate(scale) if s == v]:
                for k in ("y", "residual_out", "dx", "dresidual_in"):
                    same_bits(mixed[k][b * per:(b + 1) * per], whole[k][b * per:(b + 1) * per], f"{k} of sample {b} (scale {v})")


# ---- 5 / 6: the C ABI on buffers of the test's own -------------------------------------------------------------------------------
class Framed:
    """an output as the interior of a sentinel-filled buffer: GUARD rows in front and behind, PAD columns behind every row"""

    def __init__(self, rows, cols, dtype, dev, pad=PAD):
        self.buf = torch.full((rows + 2 * GUARD, cols + pad), SENTINEL, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + rows, :cols]
        self.view.fill_(float("nan"))

    def intact(self, what):
        rows, cols = self.view.shape
        for name, g in (("in front of the first row", self.buf[:GUARD]), ("behind the last row", self.buf[GUARD + rows:]),
                        ("behind a row's last column", self.buf[GUARD:GUARD + rows, cols:])):
            assert bool((g == SENTINEL).all()), f"{what}: wrote {name}"

    def untouched(self, what):
        self.intact(what)
        assert bool(torch.isnan(self.view.float()).all()), f"{what}: a refused call wrote"


def raw_args(lib, t, scale, case, out):
    """NormDropArgs of the forward and of the backward over the Framed outputs `out`"""
    batch, per, cols, generic = case
    dt = aum_hip._DT
    p = aum_hip._ptr
    f, b = aum_hip.NormDropArgs(), aum_hip.NormDropArgs()
    for d in (f, b):
        a = d.base
        a.weight, a.rows, a.cols, a.eps = p(t["weight"]), batch * per, cols, EPS
        a.x_dtype = a.y_dtype = dt[t["x"].dtype]
        a.res_dtype = dt[t["residual"].dtype]
        a.flags = 2 if generic else 0
        d.row_scale, d.rows_per_scale = p(scale), per
    a = f.base
    a.x, a.residual, a.y, a.residual_out, a.rstd_out = p(t["x"]), p(t["residual"]), p(out["y"].view), p(out["residual_out"].view), p(out["rstd"].view)
    a.row_stride_x, a.row_stride_res = t["x"].stride(0), t["residual"].stride(0)
    a.row_stride_y, a.row_stride_res_out = out["y"].view.stride(0), out["residual_out"].view.stride(0)
    a = b.base
    a.x, a.dy, a.dresidual_out, a.rstd_in = p(out["residual_out"].view), p(t["dy"]), p(t["dres"]), p(out["rstd"].view)
    a.dx, a.dresidual_in, a.dweight_partial = p(out["dx"].view), p(out["dresidual_in"].view), p(out["dweight_partial"].view)
    a.row_stride_x, a.row_stride_dy, a.row_stride_dres_out = out["residual_out"].view.stride(0), t["dy"].stride(0), t["dres"].stride(0)
    a.row_stride_dx, a.row_stride_dres_in = out["dx"].view.stride(0), out["dresidual_in"].view.stride(0)
    return f, b


def framed_outputs(lib, t, case, dev):
    batch, per, cols, generic = case
    rows = batch * per
    xd, rd = t["x"].dtype, t["residual"].dtype
    n_part = int(lib.c.aum_rmsnorm_bwd_partials(rows))          # the size to allocate; partial_rows of them hold sums
    out = {"y": Framed(rows, cols, xd, dev), "residual_out": Framed(rows, cols, rd, dev), "dx": Framed(rows, cols, xd, dev),
           "dresidual_in": Framed(rows, cols, rd, dev),
           "dweight_partial": Framed(n_part, cols, torch.float32, dev, pad=0),      # contiguous by contract: no pad columns
           "rstd": Framed(1, rows, torch.float32, dev)}                              # one row of `rows` values
    return out


def launch(lib, fn, args, like):
    rc = fn(aum_hip.C_byref(args), lib.stream(like))
    if not lib.host:
        torch.cuda.synchronize()
    return rc


def check_guards(lib, dev, case, dtypes):
    """the outputs inside sentinel guards: the guards come back intact and the interiors are the binding's bits"""
    t = inputs(case, dtypes, dev, seed=4)
    batch, per, cols, generic = case
    for scale in scale_vectors(batch):
        out = framed_outputs(lib, t, case, dev)
        s = torch.tensor(scale, dtype=torch.float32, device=dev)
        f, b = raw_args(lib, t, s, case, out)
        assert launch(lib, lib.c.aum_rmsnorm_drop_fwd, f, t["x"]) == 0
        assert launch(lib, lib.c.aum_rmsnorm_drop_bwd, b, t["x"]) == 0
        for k, fr in out.items():
            fr.intact(f"{k} {shape_id(case)} {scale}")
        n_sums = int(lib.c.aum_rmsnorm_bwd_partial_rows(batch * per, cols, 2 if generic else 0))
        assert bool(torch.isnan(out["dweight_partial"].view[n_sums:]).all()), "partial rows past aum_rmsnorm_bwd_partial_rows were written"
        ref = run(lib, t, scale, case)
        for k in ("y", "residual_out", "dx", "dresidual_in"):
            same_bits(out[k].view.contiguous(), ref[k], k)
        same_bits(out["rstd"].view[0].contiguous(), ref["rstd"], "rstd")
        # the binding adds the same partial rows in fp32, in a fixed order: n_sums roundings of at most 2^-24 of the running sum each
        part = f64(out["dweight_partial"].view[:n_sums])
        assert bool((np.abs(part.sum(0) - f64(ref["dweight"])) <= n_sums * 2.0 ** -23 * np.abs(part).sum(0) + 1e-30).all()), "dweight"


def check_argument_rules(lib, dev):
    """NULL row_scale / residual / dresidual_in and rows that are not whole samples: the family's error code, nothing written"""
    case = (3, 7, 200, False)
    t = inputs(case, (torch.bfloat16, torch.float32), dev, seed=5)
    s = torch.tensor(scale_vectors(3)[0], dtype=torch.float32, device=dev)
    E_NULL, E_SHAPE = -1, -2

    def refused(which, edit, want):
        out = framed_outputs(lib, t, case, dev)
        f, b = raw_args(lib, t, s, case, out)
        if which == "bwd":                      # the backward reads the forward's outputs: give it finite ones, then look at its own
            assert launch(lib, lib.c.aum_rmsnorm_drop_fwd, f, t["x"]) == 0
        a = f if which == "fwd" else b
        edit(a)
        fn = lib.c.aum_rmsnorm_drop_fwd if which == "fwd" else lib.c.aum_rmsnorm_drop_bwd
        assert launch(lib, fn, a, t["x"]) == want, (which, want)
        for k in (("y", "residual_out", "rstd") if which == "fwd" else ("dx", "dresidual_in", "dweight_partial")):
            out[k].untouched(k)

    for which in ("fwd", "bwd"):
        refused(which, lambda a: setattr(a, "row_scale", None), E_NULL)
        refused(which, lambda a: setattr(a, "rows_per_scale", 4), E_SHAPE)           # 21 rows
        refused(which, lambda a: setattr(a, "rows_per_scale", 0), E_SHAPE)
        refused(which, lambda a: setattr(a, "reserved", 1), -4)                      # AUM_E_UNSUPPORTED: the field is for later use
    refused("fwd", lambda a: setattr(a.base, "residual", None), E_NULL)
    refused("fwd", lambda a: setattr(a.base, "residual_out", None), E_NULL)
    refused("bwd", lambda a: setattr(a.base, "dresidual_in", None), E_NULL)
    assert lib.c.aum_rmsnorm_drop_fwd(None, None) == E_NULL and lib.c.aum_rmsnorm_drop_bwd(None, None) == E_NULL
    # the binding refuses the same before any launch
    with pytest.raises(ValueError):
        aum_hip.rmsnorm_drop_fwd(t["x"], t["weight"], None, s, 7, EPS, lib=lib)
    with pytest.raises(ValueError):
        aum_hip.rmsnorm_drop_fwd(t["x"], t["weight"], t["residual"], s, 4, EPS, lib=lib)
    with pytest.raises(ValueError):
        aum_hip.rmsnorm_drop_fwd(t["x"], t["weight"], t["residual"], s[:2], 7, EPS, lib=lib)


# ---- 7: op layer -----------------------------------------------------------------------------------------------------------------
class Launches:
    """counts the binding's norm launches by name (the library in use must be aum_hip's product library, or the injected one)"""
    NAMES = ("rmsnorm_fwd", "rmsnorm_bwd", "rmsnorm_drop_fwd", "rmsnorm_drop_bwd")

    def __init__(self, monkeypatch):
        self.n = {k: 0 for k in self.NAMES}
        for k in self.NAMES:
            monkeypatch.setattr(aum_hip, k, self._counting(k, getattr(aum_hip, k)))

    def _counting(self, name, real):
        def f(*a, **kw):
            self.n[name] += 1
            return real(*a, **kw)
        return f

    def scaled(self):
        return self.n["rmsnorm_drop_fwd"] + self.n["rmsnorm_drop_bwd"]

    def unscaled(self):
        return self.n["rmsnorm_fwd"] + self.n["rmsnorm_bwd"]


def check_op_layer(dev, dtypes, prenorm, monkeypatch):
    """rms_norm_fn(row_scale=s) under autograd against rms_norm_ref(row_scale=s, upcast=True): outputs and the gradients of x, residual
    and weight; row_scale=None launches the unscaled names only"""
    from mamba_ssm.ops.triton.layernorm import RMSNorm, rms_norm_fn, rms_norm_ref
    xd, rd = dtypes
    batch, length, cols = 3, 11, 768
    g = torch.Generator().manual_seed(7)
    mk = lambda *s: torch.randn(*s, generator=g)
    x0, r0, w0 = mk(batch, length, cols).to(xd).to(dev), mk(batch, length, cols).to(rd).to(dev), (1 + 0.3 * mk(cols)).to(dev)
    dy, dr = mk(batch, length, cols).to(dev), mk(batch, length, cols).to(dev)
    s = torch.tensor(scale_vectors(batch)[0], dtype=torch.float32, device=dev)

    def go(fn, **kw):
        x, r, w = (v.clone().requires_grad_(True) for v in (x0, r0, w0))
        out = fn(x, w, None, residual=r, prenorm=prenorm, eps=EPS, row_scale=s, **kw)
        y, ro = out if prenorm else (out, None)
        loss = (y.float() * dy).sum() + ((ro.float() * dr).sum() if prenorm else 0)
        loss.backward()
        return {"y": y, "residual_out": ro, "dx": x.grad, "dresidual": r.grad, "dweight": w.grad}

    counts = Launches(monkeypatch)
    got = go(rms_norm_fn, residual_in_fp32=True)
    assert counts.n == {"rmsnorm_fwd": 0, "rmsnorm_bwd": 0, "rmsnorm_drop_fwd": 1, "rmsnorm_drop_bwd": 1}
    ref = go(rms_norm_ref, upcast=True)
    for k, v in got.items():
        if v is not None:
            e = rel_err(f64(v), f64(ref[k]))
            print(f"op layer {dtype_id(dtypes)} prenorm={prenorm} {k}: {e:.3e}")
            assert e < bar(xd), (k, e)          # the bar of the call's I/O: the fp32 dweight of a 16-bit call sums 16-bit saved rows
    assert got["dx"].dtype == xd and got["dresidual"].dtype == rd
    assert int(bits(got["dx"][0]).ne(0).sum()) == 0            # sample 0 is dropped: its mixer receives +0
    # None: the unscaled pair and nothing else; the module's forward hands the keyword on
    x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    norm = RMSNorm(cols, eps=EPS).to(dev)
    y = norm(x, residual=r, prenorm=False, residual_in_fp32=True)
    y.float().sum().backward()
    assert counts.n == {"rmsnorm_fwd": 1, "rmsnorm_bwd": 1, "rmsnorm_drop_fwd": 1, "rmsnorm_drop_bwd": 1}
    y2 = norm(x0, residual=r0, row_scale=torch.ones_like(s))
    assert counts.n["rmsnorm_drop_fwd"] == 2
    same_bits(y2, y.detach(), "RMSNorm.forward(row_scale=ones) is the unscaled module")
    with pytest.raises(ValueError):
        rms_norm_fn(x0, w0, None, residual=None, row_scale=s)
    with pytest.raises(ValueError):
        rms_norm_fn(x0, w0, None, residual=r0, row_scale=s[:2])


def check_op_layer_grad_home(dev):
    """a homed weight (ssi.GradHomes: the parameter's place in a gradient bucket) receives the scaled backward's gradient in place"""
    from mamba_ssm.ops import selective_scan_interface as ssi
    from mamba_ssm.ops.triton.layernorm import rms_norm_fn
    g = torch.Generator().manual_seed(8)
    cols = 768
    x, r = torch.randn(3, 5, cols, generator=g).to(dev), torch.randn(3, 5, cols, generator=g).to(dev)
    s = torch.tensor(scale_vectors(3)[0], dtype=torch.float32, device=dev)
    w = torch.nn.Parameter((1 + 0.3 * torch.randn(cols, generator=g)).to(dev))
    rms_norm_fn(x, w, None, residual=r, row_scale=s).sum().backward()
    want = w.grad.clone()
    w.grad = None
    bucket = torch.full((cols + 16,), SENTINEL, device=dev)
    home = bucket[8:8 + cols]
    w._aum_grad_home = home                     # what ssi.adopt_grad_homes leaves behind a DistributedDataParallel backward
    hits = ssi.HOME_HITS[0]
    rms_norm_fn(x, w, None, residual=r, row_scale=s).sum().backward()
    assert ssi.HOME_HITS[0] == hits + 1
    same_bits(home, want, "the gradient in its home")
    assert w.grad is not None and w.grad.data_ptr() == home.data_ptr(), "the parameter's .grad is the home"
    assert bool((bucket[:8] == SENTINEL).all()) and bool((bucket[8 + cols:] == SENTINEL).all())


# ---- 8 / 9: model ----------------------------------------------------------------------------------------------------------------
# the smallest configuration of the model tests (golden/cases.py MODEL_CASES: 64 channels, 128 x 128 frames, 10 classes), at depth 4, batch 4
MODEL_KW = dict(spectrogram_size=(128, 128), depth=4, embed_dim=64, num_classes=10)
MODEL_BATCH = 4


def fixed_table(depth, batch, dev):
    """(depth + 1, batch) factors: row 0 ones, every other row a 0 and a 1 / keep of its own"""
    t = torch.ones(depth + 1, batch)
    for i in range(1, depth + 1):
        keep = 1.0 - 0.1 * i
        t[i] = torch.tensor(([0.0, 1.0 / keep] * batch)[(i % 2):(i % 2) + batch])
    return t.to(dev)


def _reference_way(real, rounded=False):
    """the same model with the factor as a torch multiply in front of the UNSCALED rms_norm_fn `real` (what the reference's Block does).
    rounded: timm's DropPath to the letter -- the factor and the product in the activations' type (a figure to report, not a bar)"""
    def mul_then_norm(x, *a, row_scale=None, **kw):
        if row_scale is not None and rounded:
            x = x * row_scale.reshape((-1,) + (1,) * (x.dim() - 1)).to(x.dtype)
        elif row_scale is not None:
            # hidden * s[:, None, None] as torch forms it: s is an fp32 tensor, so the product is fp32 whatever the activations' type (the
            # unscaled kernels then add the residual to it: two fp32 roundings where the scaled kernels' fma has one); its gradient,
            # g * s in fp32, is rounded once to the activations' type on its way to the mixer, as the scaled backward rounds its dx
            x = x * row_scale.reshape((-1,) + (1,) * (x.dim() - 1))
        return real(x, *a, **kw)
    return mul_then_norm


def check_model(dev, bidirectional, autocast, monkeypatch):
    import aum.model as M
    torch.manual_seed(11)
    kw = dict(MODEL_KW, if_bidirectional=True, bimamba_type="none") if bidirectional else dict(MODEL_KW, bimamba_type="v1")
    model = M.AudioMamba(drop_path_rate=0.2, **kw).to(dev).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("norm.weight") or n.endswith("norm_f.weight"):
                p.add_(0.2 * torch.randn_like(p))
    table = fixed_table(kw["depth"], MODEL_BATCH, dev)
    for i in range(1, kw["depth"] + 1):
        assert bool((table[i] == 0).any()) and bool((table[i] > 1).any())
    monkeypatch.setattr(model, "drop_scales", lambda batch, device: table)
    x = torch.randn(MODEL_BATCH, 128, 128, device=dev)
    dl = torch.randn(MODEL_BATCH, 10, device=dev)

    def go():
        model.zero_grad()
        with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16, enabled=autocast):
            logits = model(x)
        (logits.float() * dl).sum().backward()
        return logits.detach().float(), {k: p.grad.clone() for k, p in model.named_parameters()}

    counts = Launches(monkeypatch)
    got = go()
    n_scaled = kw["depth"] - (2 if bidirectional else 1) + 1        # every block with a residual, and the final norm
    assert counts.n["rmsnorm_drop_fwd"] == n_scaled and counts.n["rmsnorm_drop_bwd"] == n_scaled, counts.n
    real = M.rms_norm_fn
    monkeypatch.setattr(M, "rms_norm_fn", _reference_way(real))
    ref = go()
    assert counts.n["rmsnorm_drop_fwd"] == n_scaled, "the reference way runs the unscaled kernels"
    tol = 1e-2 if autocast else 1e-4
    e = rel_err(got[0].cpu().numpy(), ref[0].cpu().numpy())
    print(f"model bidirectional={bidirectional} autocast={autocast} logits: {e:.3e}")
    assert e < tol, e
    for k in got[1]:
        e = rel_err(got[1][k].float().cpu().numpy(), ref[1][k].float().cpu().numpy())
        print(f"  grad {k}: {e:.3e}")
        assert e < tol, (k, e)
    if autocast:
        # reported only: the distance to the reference's own rounding (factor and product in bf16), which is another bf16 run of the model
        monkeypatch.setattr(M, "rms_norm_fn", _reference_way(real, rounded=True))
        tim = go()
        worst = max((rel_err(got[1][k].float().cpu().numpy(), tim[1][k].float().cpu().numpy()), k) for k in got[1])
        print(f"  against the bf16-rounded DropPath: logits {rel_err(got[0].cpu().numpy(), tim[0].cpu().numpy()):.3e}, worst gradient "
              f"{worst[1]} {worst[0]:.3e}")
        assert bool(torch.isfinite(tim[0]).all())


def check_model_behaviour(dev, monkeypatch):
    """eval() at rate 0.2 and train() at rate 0 are the model built without the argument, bit for bit, on the unscaled kernels only"""
    import aum.model as M
    kw = dict(MODEL_KW, bimamba_type="v1")
    torch.manual_seed(12)
    plain = M.AudioMamba(**kw).to(dev)
    dropping, zero = M.AudioMamba(drop_path_rate=0.2, **kw).to(dev), M.AudioMamba(drop_path_rate=0.0, **kw).to(dev)
    assert sorted(dropping.state_dict()) == sorted(plain.state_dict())
    dropping.load_state_dict(plain.state_dict())
    zero.load_state_dict(plain.state_dict())
    assert [round(l.drop_path, 6) for l in dropping.layers] == [0.0, 0.0, 0.066667, 0.133333] and dropping.drop_path_rate == 0.2
    x = torch.randn(MODEL_BATCH, 128, 128, device=dev)

    def go(m):
        m.zero_grad()
        y = m(x)
        y.square().sum().backward()
        return y.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}

    counts = Launches(monkeypatch)
    monkeypatch.setattr(M, "drop_factors", lambda keep: pytest.fail("a factor was drawn"))
    for training, models in ((True, (zero,)), (False, (zero, dropping))):
        ref = go(plain.train(training))
        counts.n = {k: 0 for k in counts.n}
        again = go(plain)
        n_plain = dict(counts.n)
        assert counts.scaled() == 0 and counts.unscaled() > 0
        same_bits(again[0], ref[0], "logits")
        # gradients the plain model itself reproduces run to run (all of them on the host; on the device every one that no kernel adds up
        # with floating-point atomics) are held bit for bit; the add + norm weights are always among them
        repeatable = [k for k in ref[1] if torch.equal(bits(ref[1][k]), bits(again[1][k]))]
        assert all(k in repeatable for k in ref[1] if k.endswith("norm.weight") or k == "norm_f.weight"), repeatable
        for m in models:
            counts.n = {k: 0 for k in counts.n}
            got = go(m.train(training))
            assert counts.n == n_plain, counts.n
            same_bits(got[0], ref[0], "logits")
            for k in repeatable:
                same_bits(got[1][k], ref[1][k], k)
    with pytest.raises(ValueError):
        M.AudioMamba(drop_path_rate=1.0, **kw)
    with pytest.raises(NotImplementedError):
        M.AudioMamba(drop_rate=0.1, **kw)                           # token dropout stays outside


def check_model_draws(dev, monkeypatch):
    """a training forward at a rate draws drop_scales exactly once and runs; a block used on its own draws its own factors"""
    import aum.model as M
    torch.manual_seed(13)
    model = M.AudioMamba(drop_path_rate=0.5, **dict(MODEL_KW, bimamba_type="v1")).to(dev).train()
    calls = []
    real = model.drop_scales
    monkeypatch.setattr(model, "drop_scales", lambda batch, device: (calls.append(batch), real(batch, device))[1])
    x = torch.randn(MODEL_BATCH, 128, 128, device=dev)
    y = model(x)
    y.sum().backward()
    assert calls == [MODEL_BATCH] and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    counts = Launches(monkeypatch)
    blk = model.layers[3]
    h = torch.randn(MODEL_BATCH, 9, 64, device=dev)
    blk(h, torch.randn(MODEL_BATCH, 9, 64, device=dev))
    assert counts.n["rmsnorm_drop_fwd"] == 1
    blk(h, None)                                                     # no residual: no drop
    assert counts.n["rmsnorm_drop_fwd"] == 1 and counts.n["rmsnorm_fwd"] == 1
    # depth 1: the one block never drops, the add in front of norm_f drops at the rate itself
    one = M.AudioMamba(drop_path_rate=0.5, **dict(MODEL_KW, depth=1, bimamba_type="v1")).to(dev).train()
    counts.n = {k: 0 for k in counts.n}
    one(x).sum().backward()
    assert counts.n == {"rmsnorm_fwd": 1, "rmsnorm_bwd": 1, "rmsnorm_drop_fwd": 1, "rmsnorm_drop_bwd": 1}, counts.n


# ---- 10: the factors -------------------------------------------------------------------------------------------------------------
def check_drop_scales(dev, monkeypatch):
    import aum.model as M
    depth, rate, batch = 4, 0.2, 4096
    model = M.AudioMamba(drop_path_rate=rate, **dict(MODEL_KW, depth=depth, bimamba_type="none"))
    draws = []
    real = torch.bernoulli
    monkeypatch.setattr(torch, "bernoulli", lambda p, *a, **kw: (draws.append((tuple(p.shape), p.device.type)), real(p, *a, **kw))[1])
    torch.manual_seed(1234)
    s = model.drop_scales(batch, dev)
    assert draws == [((depth + 1, batch), torch.device(dev).type)], f"one Bernoulli launch on the device for the whole table: {draws}"
    assert s.shape == (depth + 1, batch) and s.dtype == torch.float32 and s.device.type == torch.device(dev).type
    torch.manual_seed(1234)
    assert torch.equal(model.drop_scales(batch, dev), s), "reproducible under torch.manual_seed"
    assert not torch.equal(model.drop_scales(batch, dev), s)
    s = s.cpu()
    assert bool((s[0] == 1).all())
    rates = [0.0] + [rate * (i - 1) / (depth - 1) for i in range(1, depth)] + [rate]
    for i in range(1, depth + 1):
        keep = 1.0 - rates[i]
        vals = s[i].unique().tolist()
        if keep == 1.0:
            assert vals == [1.0]
            continue
        assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] * keep - 1.0) < 4e-7, (i, vals)      # 1 / keep to fp32 rounding
        frac = float((s[i] != 0).float().mean())
        assert abs(frac - keep) <= 5 * (keep * (1 - keep) / batch) ** 0.5, (i, frac, keep)
    one = M.AudioMamba(drop_path_rate=rate, **dict(MODEL_KW, depth=1, bimamba_type="none"))
    # depth 1: the linspace is [0] (the one block never drops); the add in front of norm_f still uses the rate itself
    assert one._drop_rates == [0.0, rate]
    s1 = one.drop_scales(batch, dev).cpu()
    assert s1.shape == (2, batch) and bool((s1[0] == 1).all())
    vals = s1[1].unique().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] * (1.0 - rate) - 1.0) < 4e-7, vals
    frac = float((s1[1] != 0).float().mean())
    assert abs(frac - (1.0 - rate)) <= 5 * (rate * (1 - rate) / batch) ** 0.5, frac


# ---- 11: launcher ----------------------------------------------------------------------------------------------------------------
def check_scope():
    from aum import train as T
    parse = T.build_parser().parse_args
    T.check_scope(parse(["--aum_drop_path", "0.1"]))
    with pytest.raises(NotImplementedError, match="epic_sounds"):
        T.check_scope(parse(["--aum_drop_path", "0.1", "--dataset", "epic_sounds", "--epic_config", "/c.yaml"]))
    with pytest.raises(NotImplementedError):
        T.check_scope(parse(["--flexible_training", "True"]))
    with pytest.raises(ValueError):
        T.check_scope(parse(["--aum_drop_path", "1.0"]))
    args = parse(["--aum_drop_path", "0.1", "--depth", "4", "--model_type", "tiny", "--n_class", "4", "--audio_length", "64"])
    model = T.build_model(args)
    assert model.drop_path_rate == 0.1 and abs(model.layers[3].drop_path - 0.1 * 2 / 3) < 1e-7


def check_launcher_trains(tmp_path, monkeypatch):
    """aum.train --aum_drop_path 0.1 --depth 4 --max-steps 2 on the toy dataset of tools/make_toy_audioset.py (the reference's command
    line with the flag set): finite train and validation losses, the training steps on the scaled kernels and the validation not"""
    import os
    import subprocess
    import sys
    import aum.train as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = str(tmp_path / "toy")
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_toy_audioset.py"), data, "--clips", "8", "--val-clips", "2", "--seconds", "0.7",
                    "--classes", "4"], check=True)
    files = sorted(os.listdir(data))
    pick = lambda *keys: os.path.join(data, next(f for f in files if all(k in f for k in keys)))
    exp = str(tmp_path / "exp")
    counts = Launches(monkeypatch)
    T.main(["--model", "aum", "--model_type", "tiny", "--aum_type", "Fo-Bi", "--depth", "4", "--aum_drop_path", "0.1", "--n_class", "4",
            "--label-csv", pick(".csv"), "--data-train", pick("train", ".json"), "--data-val", pick("val", ".json"), "--audio_length", "64",
            "--num-workers", "0", "-b", "4", "--exp-dir", exp, "--n-epochs", "1", "--max-steps", "2", "--n-print-steps", "1000", "--lr", "1e-3",
            "--lrscheduler_start", "10", "--save_model", "False"])
    result = np.loadtxt(os.path.join(exp, "result.csv"), delimiter=",", ndmin=2)
    print(f"--aum_drop_path 0.1, two steps: train loss {result[0, 5]:.6f}, valid loss {result[0, 6]:.6f}; launches {counts.n}")
    assert result.shape == (1, 8) and np.isfinite(result[0, [5, 6]]).all(), result
    # two training steps x (blocks 1 .. 3 and the final norm), forward and backward; validation (eval mode) adds none
    assert counts.n["rmsnorm_drop_fwd"] == 8 and counts.n["rmsnorm_drop_bwd"] == 8, counts.n
    assert counts.n["rmsnorm_fwd"] > 2, counts.n
