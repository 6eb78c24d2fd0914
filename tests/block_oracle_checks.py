"""The fused Mamba block (selective_scan_interface: bimamba_inner_fn / mamba_inner_fn / mamba_inner_fn_no_out_proj x 2) under 16-bit
autocast at the widths its fast kernels take (cases.INNER_WIDE_CASES), against the fp64 oracle of the same block: shared bodies of
test_block_oracle.py (host: the references themselves and what the bars can see) and test_gpu_block_oracle.py (the product).

Three computations of one block from the operands the kernels see (xz, dout and the three projection weights rounded to the 16-bit type,
everything else fp32):
  oracle_reference   oracle.inner_fwd + inner_full_bwd (v1, none), inner_no_out_proj_fwd x 2 + inner_bwd x 2 composed as MS:214-246 (v2), fp64
  staged_reference   the same arithmetic stage by stage on the oracle's stage functions, a tensor rounded to the 16-bit type wherever the
                     product stores one (list in its docstring).  With no rounding it IS the oracle (1e-12, test_block_oracle.py); with
                     one term changed (`mutant`) it is the oracle with that mistake
  the product        check_block

Bars.  r = distance(staged_reference, oracle_reference) per (case, dtype, quantity, measure) is what the stored 16-bit tensors cost an
ideal implementation; the product's distance to the oracle has to stay below FACTOR x r = 2.2 r (two placements of the same roundings are
two draws of one spread: sqrt(2) x 1.5, as test_gpu_model._headline_lowp_vs_reference), floored at the fp32 figures of kernel_checks
(NORM_F32_BAR for the fp32 parameter sums, TOL_F32 for out and d xz).  r is computed when the test runs; nothing is taken from the kernels.
Measures: conftest.rel_err (`rel`), rms_err (`rms`), and for dA / dA_b rel_err_by state column (`state`); d xz also by halves (x | z),
d x_proj_w also by row block (dt | B | C).

The table of the worst product errors on the MI355X follows this docstring.
"""
# Worst product error / its bar on the MI355X over INNER_WIDE_CASES, every arm of test_gpu_block_oracle.py (measure `rel`; `state` for A):
#   quantity        bf16 error / bar      fp16 error / bar      (each pair: the figure with the largest error / bar)
#   out             4.58e-3 / 1.01e-2     4.16e-4 / 9.00e-4
#   d xz, x half    4.24e-3 / 9.08e-3     4.25e-4 / 9.34e-4
#   d xz, z half    5.58e-3 / 1.23e-2     4.86e-4 / 1.07e-3
#   d conv_w        4.22e-3 / 9.11e-3     4.32e-4 / 8.63e-4
#   d conv_b        2.12e-3 / 3.74e-3     4.07e-4 / 7.94e-4
#   d x_proj_w dt   5.56e-3 / 8.99e-3     5.97e-4 / 1.09e-3
#   d x_proj_w B    3.64e-3 / 7.73e-3     5.89e-4 / 1.22e-3
#   d x_proj_w C    5.76e-3 / 1.04e-2     4.46e-4 / 8.15e-4
#   d dt_proj_w     9.89e-3 / 1.90e-2     9.63e-4 / 1.36e-3
#   d dt_bias       2.70e-3 / 4.81e-3     7.21e-4 / 1.13e-3
#   d A, d A_b      1.17e-2 / 2.27e-2     9.97e-4 / 1.95e-3
#   d D             2.39e-3 / 5.26e-3     5.08e-4 / 1.12e-3
#   d out_proj_w    3.34e-3 / 7.35e-3     5.31e-4 / 1.17e-3
# (the _b parameter set folded into its row.)  Largest error / bar over every case, quantity and measure: bf16 token-major 0.62, channel-major
# 0.52, aum_gemm_tn forced 0.56, dt_bias and softplus inside the scans 0.57, x/dt backward on the library 0.56; fp16 token-major 0.60, channel-major
# 0.71 -- i.e. the product is within 1.6 r everywhere; in most figures its error equals r to three digits (it rounds where the staged
# reference rounds).
import numpy as np
import torch
import torch.nn.functional as F

import cases
import kernel_checks as KC
from conftest import rel_err, rel_err_by, rms_err
from oracle import oracle as O

FACTOR = 2.2
N_STATE = 16
WIDE = {c[0]: c for c in cases.INNER_WIDE_CASES}
# what a parameter set is made of; Bi-Bi's second set carries the suffix _b (its A is A_b)
_SET = ("conv_w", "conv_b", "x_proj_w", "dt_proj_w", "dt_bias", "D")
_ORACLE_KEYS = {"dconv_w": "conv_w", "dconv_b": "conv_b", "dx_proj_w": "x_proj_w", "ddt_proj_w": "dt_proj_w", "ddelta_bias": "dt_bias",
                "dA": "A", "dA_b": "A_b", "dD": "D", "dout_proj_w": "out_proj_w", "dxz": "xz"}
# (a) - (g): one term of the backward wrong each (staged_reference)
MUTANTS = {"a": "the reverse direction's part of d dt_bias dropped",
           "b": "the reverse direction's dz dropped",
           "c": "dB and dC rows swapped in dx_dbl",
           "d": "the dt block's part of d x_proj_w dropped",
           "e": "ddelta passed on without the softplus derivative",
           "f": "Bi-Bi's / 2 missing from the backward",
           "g": "one 64-token split left out of d out_proj_w"}


def mutants_of(mode):
    """(a), (b) need a reverse direction, (f) the Bi-Bi composition"""
    return [m for m in MUTANTS if not (mode == "none" and m in "abf") and not (mode == "v1" and m == "f")]


# ----------------------------------------------------------------------------------------------
# operands and the two references
# ----------------------------------------------------------------------------------------------
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def operands(case, dtype):
    """-> (p, q).  p: fp32 arrays for the product's leaves, xz and dout rounded to `dtype` (what in_proj delivers / what arrives from the
    next layer); q: the fp64 arrays the kernels see -- p with x_proj_w, dt_proj_w, out_proj_w (and the _b set's) rounded as autocast casts
    them (test_gpu_model.test_autocast_rules_bf16); conv weight and bias, A, A_b, D and dt_bias stay fp32."""
    def make():
        p = cases.inner_inputs(*case)
        p["xz"], p["dout"] = KC.rq(p["xz"], dtype), KC.rq(p["dout"], dtype)
        q = {k: np.asarray(KC.rq(v, dtype) if "_proj_w" in k else v, np.float64) for k, v in p.items()}
        return p, q
    return _cached(("operands", case[0], dtype), make)


def _pset(q, sfx):
    return {k: q[k + sfx] for k in _SET}


def _named(out, grads, sfx=""):
    res = {} if out is None else {"out": out}
    for k, v in grads.items():
        if v is not None and k in _ORACLE_KEYS:
            res[_ORACLE_KEYS[k] + sfx] = v
    return res


def oracle_reference(case, q):
    """the block in fp64 with nothing rounded: {"out", "xz" (= d xz), parameter name: its gradient}"""
    mode = case[1]
    dout = q["dout"]
    batch, L, Dm = dout.shape
    if mode != "v2":
        A_b = q["A_b"] if mode == "v1" else None
        a = (q["xz"], q["conv_w"], q["conv_b"], q["x_proj_w"], q["dt_proj_w"], q["out_proj_w"], None, q["A"], q["D"], q["dt_bias"])
        st = O.inner_fwd(*a, A_b=A_b, prec="f64")
        return _named(st["out"], O.inner_full_bwd(st, dout, *a, A_b=A_b, prec="f64"))
    # MS:214-246: two one-direction pipelines with their own parameters, the second on the flipped sequence, (of + ob) / 2, one out_proj
    sets = [(_pset(q, ""), q["A"], False), (_pset(q, "_b"), q["A_b"], True)]
    sts = [O.inner_no_out_proj_fwd(q["xz"], P["conv_w"], P["conv_b"], P["x_proj_w"], P["dt_proj_w"], A, P["D"], P["dt_bias"], rev, "f64")
           for P, A, rev in sets]
    y_t = _tok((sts[0]["out_z"] + sts[1]["out_z"]) / 2)
    dout2 = dout.reshape(batch * L, Dm)
    dy = _chan(dout2 @ q["out_proj_w"], batch) / 2
    gs = [O.inner_bwd(st, dy, q["xz"], P["conv_w"], P["conv_b"], P["x_proj_w"], P["dt_proj_w"], A, P["D"], P["dt_bias"], None, rev, "f64")
          for st, (P, A, rev) in zip(sts, sets)]
    res = _named((y_t @ q["out_proj_w"].T).reshape(batch, L, Dm), gs[0])
    second = _named(None, gs[1], "_b")
    res["A_b"] = second.pop("A_b")              # the second pipeline's A is A_b
    res["xz"] = res["xz"] + second.pop("xz_b")  # both pipelines read one xz: the z half carries BOTH directions' dz
    res.update(second)
    res["out_proj_w"] = dout2.T @ y_t
    return res


def _rounder(dtype):
    if dtype == torch.float32:          # the fp32 block stores no 16-bit tensor
        return lambda a: a
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()


def _tok(a):
    """(B, X, L) -> token rows (B L, X)"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, a.shape[1])


def _chan(a2, batch):
    """(B L, X) -> (B, X, L)"""
    return np.ascontiguousarray(a2.reshape(batch, -1, a2.shape[1]).transpose(0, 2, 1))


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _pipe_fwd(xz, P, A, A_b, reverse, rnd, activated):
    """conv -> x/dt -> scan(s) of one parameter set; rounded: conv_out, x_dbl, delta, (Fo-Bi) the first direction's y, out_pre, out_z"""
    batch, two_e, L = xz.shape
    E, R = two_e // 2, P["dt_proj_w"].shape[1]
    x, z = np.ascontiguousarray(xz[:, :E]), np.ascontiguousarray(xz[:, E:])
    xc = rnd(O.conv1d_fwd(x, P["conv_w"], P["conv_b"], True, reverse, "f64"))
    x_dbl = rnd(_tok(xc) @ P["x_proj_w"].T)
    raw = x_dbl[:, :R] @ P["dt_proj_w"].T                  # from the ROUNDED dt block (the x/dt kernel reads its own x_dbl tile)
    if activated:       # the fused x/dt kernel stores softplus(raw + dt_bias); the scans read it as it is (oracle's softplus, SSI:106-107)
        s = raw + P["dt_bias"]
        delta, bias, softplus = rnd(np.where(s > 20, s, np.log1p(np.exp(np.minimum(s, 20))))), None, False
    else:
        delta, bias, softplus = rnd(raw), P["dt_bias"], True
    delta = _chan(delta, batch)
    Bm, Cm = _chan(x_dbl[:, R:R + N_STATE], batch), _chan(x_dbl[:, R + N_STATE:], batch)
    st = dict(x=x, z=z, xc=xc, x_dbl=x_dbl, delta=delta, B=Bm, C=Cm, bias=bias, softplus=softplus, reverse=reverse)
    if A_b is None:
        r = O.scan_fwd(xc, delta, A, Bm, Cm, P["D"], z, bias, softplus, reverse, "f64")
        st["out_pre"], st["out_z"] = rnd(r["y_pre"]), rnd(r["out"])
    else:
        # Fo-Bi in one launch: each direction runs its half of the row first and leaves its y in `out` (16 bits); the other direction adds
        # its own, the 2 D u skip and the gate
        yf = O.scan_fwd(xc, delta, A, Bm, Cm, None, None, bias, softplus, False, "f64")["out"]
        yb = O.scan_fwd(xc, delta, A_b, Bm, Cm, None, None, bias, softplus, True, "f64")["out"]
        m = (L + 1) // 2
        yf[:, :, :m] = rnd(yf[:, :, :m])
        yb[:, :, m:] = rnd(yb[:, :, m:])
        tot = yf + yb + 2.0 * P["D"][None, :, None] * xc
        st["out_pre"], st["out_z"] = rnd(tot), rnd(tot * z * _sigmoid(z))
    return st


def _pipe_bwd(st, dout_z, P, A, A_b, rnd, activated, mutant):
    """adjoint of _pipe_fwd for d out_z (B, E, L); rounded: (Fo-Bi) the first direction's du / ddelta, du, ddelta, dz, dx_dbl (both blocks),
    du after x_proj's data gradient was added, the conv's dx.  Parameter sums stay fp64 (the product: fp32)."""
    xc, delta, Bm, Cm, z = st["xc"], st["delta"], st["B"], st["C"], st["z"]
    batch, E, L = xc.shape
    R = P["dt_proj_w"].shape[1]
    dirs = [(A, st["reverse"])] if A_b is None else [(A, False), (A_b, True)]
    gs = [O.scan_bwd(xc, delta, a, Bm, Cm, P["D"], z, st["bias"], dout_z, st["softplus"], rev, "f64") for a, rev in dirs]
    # delta arrived activated: the scan's ddelta is with respect to softplus's OUTPUT; the factor back to raw, from that output:
    # sigmoid(s) = 1 - exp(-softplus(s)) (1 where softplus is the identity)
    fac = np.where(delta > 20, 1.0, -np.expm1(-delta)) if activated else 1.0
    for g in gs:
        if activated:
            g["ddelta_bias"] = (g["ddelta"] * fac).sum((0, 2))
    g = gs[0]
    grads = {"A": g["dA"]}
    if len(gs) == 2:
        gb = gs[1]
        m = (L + 1) // 2      # the backward walks a direction from its end: the partial that is handed over covers the other half
        for k in ("du", "ddelta"):
            g[k][:, :, m:] = rnd(g[k][:, :, m:])
            gb[k][:, :, :m] = rnd(gb[k][:, :, :m])
        for k in ("du", "ddelta", "dB", "dC", "dD") + (() if mutant == "a" else ("ddelta_bias",)):
            g[k] = g[k] + gb[k]
        grads["A_b"] = gb["dA"]
    grads["D"], grads["dt_bias"] = g["dD"], g["ddelta_bias"]
    du = rnd(g["du"])
    ddelta = rnd(g["ddelta"] * (1.0 if mutant == "e" else fac))
    sg = _sigmoid(z)
    pre = gs[0]["dz"] if (mutant == "b" and len(gs) == 2) else dout_z * st["out_pre"] * sg * (1.0 + z * (1.0 - sg))     # SSI:150's adjoint on the STORED pre-gate sum
    dz = rnd(pre)
    # x/dt (SSI:570-590): dx_dbl = [ddelta W_dt | dB | dC] rounded as one row; both weight gradients and du from the rounded tensors
    dbc = [_tok(g["dB"]), _tok(g["dC"])]
    ddelta2 = _tok(ddelta)
    dx_dbl = rnd(np.concatenate([ddelta2 @ P["dt_proj_w"]] + (dbc[::-1] if mutant == "c" else dbc), axis=1))
    grads["dt_proj_w"] = ddelta2.T @ st["x_dbl"][:, :R]
    for_w = dx_dbl
    if mutant == "d":
        for_w = dx_dbl.copy()
        for_w[:, :R] = 0
    grads["x_proj_w"] = for_w.T @ _tok(xc)
    du2 = rnd(_tok(du) + dx_dbl @ P["x_proj_w"])
    cg = O.conv1d_bwd(st["x"], P["conv_w"], P["conv_b"], _chan(du2, batch), True, st["reverse"], "f64")
    grads["conv_w"], grads["conv_b"] = cg["dweight"], cg["dbias"]
    grads["xz"] = np.concatenate([rnd(cg["dx"]), dz], axis=1)
    return grads


def staged_reference(case, q, dtype, activated=True, lib16=(), mutant=None):
    """The block stage by stage in fp64, `.to(dtype).double()` applied where the product stores a 16-bit tensor (dtype float32: nowhere).
    Boundaries, from _inner_forward_tm / _inner_backward_tm and DESIGN.md 4:
      forward   conv_out | x_dbl (dt block, B, C) | delta -- softplus(raw + dt_bias) when `activated` (the fused x/dt kernel's hand-over to
                the scans), else raw | Fo-Bi: the y of the direction that reaches a token first (kept in `out` until the other adds its own)
                | out_pre (the pre-gate sum the backward's dz is formed from) | out_z | Bi-Bi: of + ob, then / 2 | out
      backward  dout_z (out_proj's data gradient; Bi-Bi: d y, then / 2) | Fo-Bi: the first direction's du and ddelta | du | ddelta (with
                the softplus derivative taken from the stored delta when activated) | dz | dx_dbl: dt block and the fp32 dB | dC rows | du
                after x_proj's data gradient was added in place | the conv's dx | Bi-Bi: the sum of the two pipelines' d xz
      lib16     the weight gradients this arm leaves to a library GEMM, whose 16-bit result is widened afterwards (out_proj_w outside
                aum_gemm_wgrad's widths and under F.linear; x_proj_w / dt_proj_w with the x/dt backward on the library)
    Not modelled (inside a kernel, not a stage boundary): the scan backward's 16-bit state checkpoints every 8th step.
    mutant: one of MUTANTS."""
    mode = case[1]
    rnd = _rounder(dtype)
    w16 = lambda k, a: rnd(a) if k.replace("_b", "") in lib16 or k in lib16 else a
    xz, dout, w_out = q["xz"], q["dout"], q["out_proj_w"]
    batch, L, Dm = dout.shape
    dout2 = dout.reshape(batch * L, Dm)
    dout2_w = dout2
    if mutant == "g":       # the last full 64-token chunk (of 130 tokens: 64 .. 127; of 27: the only, ragged one) never reaches the sum
        dout2_w = dout2.copy()
        lo = max(0, (batch * L // 64 - 1) * 64)
        dout2_w[lo:lo + 64] = 0
    if mode != "v2":
        A_b = q["A_b"] if mode == "v1" else None
        P = _pset(q, "")
        st = _pipe_fwd(xz, P, q["A"], A_b, False, rnd, activated)
        y_t = _tok(st["out_z"])
        res = _pipe_bwd(st, _chan(rnd(dout2 @ w_out), batch), P, q["A"], A_b, rnd, activated, mutant)
    else:
        sets = [(_pset(q, ""), q["A"], False), (_pset(q, "_b"), q["A_b"], True)]
        sts = [_pipe_fwd(xz, P, A, None, rev, rnd, activated) for P, A, rev in sets]
        y_t = _tok(rnd(rnd(sts[0]["out_z"] + sts[1]["out_z"]) / 2))
        dy = rnd(dout2 @ w_out)
        dy = _chan(dy if mutant == "f" else rnd(dy / 2), batch)
        res, second = [_pipe_bwd(st, dy, P, A, None, rnd, activated, mutant) for st, (P, A, rev) in zip(sts, sets)]
        dxz_b = second.pop("xz")
        if mutant == "a":       # (Bi-Bi's reverse direction is the second pipeline, with a dt_bias of its own)
            second["dt_bias"] = np.zeros_like(second["dt_bias"])
        if mutant == "b":
            dxz_b[:, dxz_b.shape[1] // 2:] = 0
        res["xz"] = rnd(res["xz"] + dxz_b)
        res["A_b"] = second.pop("A")
        res.update({k + "_b": v for k, v in second.items()})
    res["out"] = rnd(y_t @ w_out.T).reshape(batch, L, Dm)
    res["out_proj_w"] = dout2_w.T @ y_t
    return {k: w16(k, v) for k, v in res.items()}


# ----------------------------------------------------------------------------------------------
# distances and bars
# ----------------------------------------------------------------------------------------------
def distances(got, ref):
    """{(quantity, measure): error of got against ref} over every quantity of `ref`"""
    d = {}

    def note(k, a, b, state=False):
        d[k, "rel"], d[k, "rms"] = rel_err(a, b), rms_err(a, b)
        if state:
            d[k, "state"] = rel_err_by(a, b, 1)

    for k, b in ref.items():
        a = np.asarray(got[k], np.float64).reshape(b.shape)
        note(k, a, b, state=k in ("A", "A_b"))
        if k == "xz":
            E = b.shape[1] // 2
            note("xz.x", a[:, :E], b[:, :E])
            note("xz.z", a[:, E:], b[:, E:])
        if k.startswith("x_proj_w"):        # a misplaced dB | dC block is an O(1) error in 16 rows of 56 or 80
            R = b.shape[0] - 2 * N_STATE
            for blk, sl in (("dt", slice(0, R)), ("B", slice(R, R + N_STATE)), ("C", slice(R + N_STATE, None))):
                note(k + "." + blk, a[sl], b[sl])
    return d


def floor_of(quantity):
    """below the fp32 block's own error nothing is measured: the fp32 parameter sums at kernel_checks.NORM_F32_BAR, out and d xz at TOL_F32"""
    return KC.TOL_F32 if quantity == "out" or quantity.startswith("xz") else KC.NORM_F32_BAR


def bars(r):
    return {k: max(FACTOR * v, floor_of(k[0])) for k, v in r.items()}


def reference_and_bars(case, dtype, activated=True, lib16=()):
    """-> (q, oracle reference, r, bars) for one arm; cached, and nobody writes into them"""
    def make():
        p, q = operands(case, dtype)
        ref = _cached(("oracle", case[0], dtype), lambda: oracle_reference(case, q))
        r = distances(staged_reference(case, q, dtype, activated, lib16), ref)
        return q, ref, r, bars(r)
    return _cached(("bars", case[0], dtype, activated, tuple(sorted(lib16))), make)


# ----------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------
_TM_BASE = {"conv_tm_fwd", "conv_tm_bwd", "xdt_tm_fwd", "xdt_tm_bwd", "gemm_wgrad"}          # + the scan pair, named by direction count
_CM_BASE = {"conv_fwd", "conv_bwd", "proj_fwd", "proj_bwd_data", "proj_bwd_weight"}


def expected_launches(mode, layout, switches):
    """(names that must be among the run's aum_hip._launch names, names that must not): tests/golden/ssi_dispatch.json's vocabulary"""
    bi = "_bidir" if mode == "v1" else ""
    if layout == "channel_major":
        # (rows longer than one pass run Fo-Bi as two one-direction launches: either name)
        return set(_CM_BASE), {n for n in _TM_BASE if n != "gemm_wgrad"} | {"scan_tm_fwd", "scan_tm_bwd", "scan_tm_fwd_bidir", "scan_tm_bwd_bidir"}
    need = set(_TM_BASE) | {"scan_tm_fwd" + bi, "scan_tm_bwd" + bi}
    never = set(_CM_BASE) | {"scan_fwd", "scan_bwd", "scan_fwd_bidir", "scan_bwd_bidir", "scan_tm_seg_fwd", "scan_tm_seg_bwd",
                             "scan_tm_seg_fwd_bidir", "scan_tm_seg_bwd_bidir", "dtproj_tm_fwd"}
    if switches.get("_GEMM_MODE") == "hip":
        need.add("gemm_tn")
    if switches.get("_XDT_BWD_HIP") is False:
        # the five library calls instead; the skinny weight-gradient launches go with the kernel (a Bi-Bi pipeline then has no aum_gemm_wgrad)
        need -= {"xdt_tm_bwd", "gemm_wgrad"}
        never.add("xdt_tm_bwd")
    return need, never


def run_product(case, dtype, layout, switches, device, monkeypatch, shared_out_proj=False):
    """one forward + backward of the block as test_gpu_model.test_inner_fns_vs_reference calls it, under autocast(dtype) ->
    ({"out", "xz", parameter name: gradient} as fp64 arrays, launch names in order, the delta_activated flags the token-major scans got)"""
    import aum_hip
    import mamba_ssm.ops.selective_scan_interface as ssi
    name, mode, batch, d_model, L = case
    p, _ = operands(case, dtype)
    t = {k: torch.tensor(v, device=device).requires_grad_(True) for k, v in p.items() if k != "dout"}
    dout = torch.tensor(p["dout"], device=device)
    tm = layout == "token_major"
    xz = t["xz"].to(dtype)
    if tm:
        monkeypatch.setattr(ssi, "_TM_MIN_WAVES", 0)
        xz = xz.transpose(1, 2).contiguous().transpose(1, 2)
        assert ssi._is_tm(xz) and ssi.token_major_ok(2 * d_model, N_STATE, 4, t["dt_proj_w"].shape[1], dtype)
    else:
        xz = xz.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    for k, v in switches.items():
        monkeypatch.setattr(ssi, k, v)
    names, act_flags = [], []
    real_launch = aum_hip._launch

    def launch(fn, args, stream_tensor, lib, lname, meta=None):
        names.append(lname)
        return real_launch(fn, args, stream_tensor, lib, lname, meta)

    def flagged(real):
        def f(*a, **k):
            act_flags.append(bool(k.get("delta_activated", False)))
            return real(*a, **k)
        return f

    with monkeypatch.context() as mp:
        mp.setattr(aum_hip, "_launch", launch)
        mp.setattr(aum_hip, "scan_tm_fwd", flagged(aum_hip.scan_tm_fwd))
        mp.setattr(aum_hip, "scan_tm_bwd", flagged(aum_hip.scan_tm_bwd))
        with torch.autocast(device, dtype=dtype):
            if mode == "v1":
                o = ssi.bimamba_inner_fn(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], t["out_proj_w"], None,
                                         t["A"], t["A_b"], None, None, t["D"], delta_bias=t["dt_bias"], delta_softplus=True)
            elif mode == "none":
                o = ssi.mamba_inner_fn(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], t["out_proj_w"], None,
                                       t["A"], None, None, t["D"], delta_bias=t["dt_bias"], delta_softplus=True)
            else:
                of = ssi.mamba_inner_fn_no_out_proj(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], t["A"], None,
                                                    None, t["D"], delta_bias=t["dt_bias"], delta_softplus=True)
                ob = ssi.mamba_inner_fn_no_out_proj(xz, t["conv_w_b"], t["conv_b_b"], t["x_proj_w_b"], t["dt_proj_w_b"],
                                                    t["A_b"], None, None, t["D_b"], delta_bias=t["dt_bias_b"],
                                                    delta_softplus=True, reverse=True)
                y = (of + ob) / 2
                if shared_out_proj:     # Mamba.forward's own call: the one place a Bi-Bi block can reach aum_gemm_tn behind the scans
                    o = ssi.out_proj_shared(t["out_proj_w"], y, tm).reshape(batch, L, -1)
                else:
                    o = F.linear(y.transpose(1, 2), t["out_proj_w"], None)
        assert o.dtype == dtype and tuple(o.shape) == (batch, L, d_model)
        (o.float() * dout).sum().backward()
        if device != "cpu":
            torch.cuda.synchronize()
    got = {"out": o.detach().double().cpu().numpy()}
    for k, v in t.items():
        if k == "A_b" and mode == "none":
            continue
        assert v.grad is not None and v.grad.dtype == torch.float32 and bool(torch.isfinite(v.grad).all()), k
        got[k] = v.grad.double().cpu().numpy()
    return got, names, act_flags


def arm_roundings(case, layout, switches, shared_out_proj):
    """(activated, lib16) of staged_reference for one arm, read off the dispatch: delta is handed over activated by the fused x/dt kernel
    of the token-major block unless _DELTA_IN_XDT is off; d out_proj_w is aum_gemm_wgrad's fp32 sum only in the token-major block's own
    out_proj at d_model % 256 == 0, a library GEMM's 16-bit result elsewhere; d x_proj_w / d dt_proj_w are 16-bit library results when the
    x/dt backward is switched to the library"""
    mode, d_model = case[1], case[3]
    tm = layout == "token_major"
    lib16 = set()
    if not (tm and d_model % 256 == 0 and (mode != "v2" or shared_out_proj)):
        lib16.add("out_proj_w")
    if tm and switches.get("_XDT_BWD_HIP") is False:
        lib16 |= {"x_proj_w", "dt_proj_w"}
    return tm and switches.get("_DELTA_IN_XDT", True), lib16


def check_block(case, dtype, layout, switches, device, monkeypatch, shared_out_proj=False):
    """the product's block against the fp64 oracle: every quantity and measure below its bar, and the launches this arm is about were made.
    Prints `block-oracle <case> <dtype> <layout> <arm> <quantity> <measure> error bar r`, one line per figure.  Returns {key: (error, bar)}"""
    name, mode = case[0], case[1]
    activated, lib16 = arm_roundings(case, layout, switches, shared_out_proj)
    q, ref, r, bar = reference_and_bars(case, dtype, activated, lib16)
    got, names, act_flags = run_product(case, dtype, layout, switches, device, monkeypatch, shared_out_proj)
    need, never = expected_launches(mode, layout, switches)
    assert need <= set(names) and not (never & set(names)), (name, layout, switches, sorted(need - set(names)), sorted(never & set(names)), names)
    if layout == "token_major":
        assert act_flags and all(f == activated for f in act_flags), (name, switches, act_flags)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    e = distances(got, ref)
    arm = ",".join(f"{k}={v}" for k, v in sorted(switches.items())) or "base"
    tag = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]
    for k in sorted(e):
        print(f"block-oracle {name} {tag} {layout} {arm} {k[0]} {k[1]} {e[k]:.3e} {bar[k]:.3e} {r[k]:.3e}")
    over = {k: (e[k], bar[k]) for k in e if not e[k] < bar[k]}
    assert not over, (name, tag, layout, arm, over)
    return {k: (e[k], bar[k]) for k in e}
