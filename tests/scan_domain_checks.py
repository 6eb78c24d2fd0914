"""The VALUE DOMAIN of the scan kernels: every kernel family against the fp64 oracle on inputs off the one distribution the other scan checks
draw from (cases.scan_inputs: delta |A| in about [1e-3, 1.6], u, B, C, z ~ N(0, 1), D ~ 1, which carries `out`).  Shared by
tests/test_scan_domain.py (CPU, lane-array library; also the conditions on the inputs, on the oracle alone) and tests/test_gpu_scan_domain.py
(device library).

Regimes (REGIMES; each a generator seeded from its name and the shape's, returning a dict with the keys of cases.scan_inputs that the check
bodies of kernel_checks.py / timeline_train_checks.py take as inputs=).  All run without D so that the skip term cannot carry `out`;
gated and ungated; the operands are rounded to the activation dtype before the kernel and the oracle see them.
  fast_decay    delta + bias over [19.25, 30.75], A = -(1..16) jitter: every multiplier and every lane / chunk / segment product underflows
  threshold     delta + bias on {19.75, 19.875, 20, 20.125, 20.25} (exact in bf16 and fp16) walking along the row, A = -(1..16) / 100 so that
                `out` still depends on delta; the bias absent or 4.0 (delta + bias stays exact)
  long_memory   delta + bias in [-13, -8], a level per channel plus jitter (the quietest row has delta = 2.3e-6 .. 6e-6 in every step),
                A = -(1..16) / 20: a = 1 - 1e-6 .. 1e-4 over the whole row
  big_state     delta about 0.05, A = -(1..16) / 50, u and B each scaled by sqrt(s), s chosen so that the largest state of an fp64
                recurrence on the unrounded values is 2e4 in the busier direction; C / 1000
  mixed_rows    the trained-like delta and A of cases.scan_inputs, channel e's u times 10^((e mod 5) - 2); also run with D
Forms of delta (FORMS): "bias" raw delta + a bias vector, softplus in the kernel; "nobias" the same without a bias (threshold only);
"act" delta = softplus(raw) formed by the caller in fp64 and rounded (AUM_SCAN_DELTA_ACTIVATED; the families that have the flag, 16-bit and
gated where the token-major training kernels ask for that; threshold and long_memory), ddelta still with respect to raw.

Measures, for every quantity: `rel` conftest.rel_err, `rms` conftest.rms_err, `row` the worst (batch, channel) row against its own
largest element (rel_err_by(..., floor=0) on (rows, L)); dA / dB / dC also `state` (rel_err_by per state at its default floor).
Bars: bar = max(family bar, FACTOR x r), r = the same measure between the oracle at prec="f32" and at "f64" on the same rounded operands
(what fp32 arithmetic costs an honest implementation there), FACTOR = block_oracle_checks.FACTOR, the family bar the one the family's
existing check uses (family_bar).  r is computed when the test runs; nothing is taken from the kernels.

Mutants (host build, scratch copies, never committed) and what catches them are listed behind the table below.
"""
# Worst product error / its bar on the MI355X per regime and family (report(); the figure with the largest error / bar over every shape,
# direction, path, form, gate, quantity and measure; 495 cases of tests/test_gpu_scan_domain.py, 12.5 s).  Everywhere the worst figure of
# the 16-bit types is the one rounding of a stored output (bf16 2^-8 = 3.9e-3, fp16 2^-11 = 4.9e-4) in the `row` measure:
#   regime       family          bf16 error / bar      fp16 error / bar      fp32 error / bar
#   fast_decay   channel-major   3.55e-3 / 1.00e-2     4.36e-4 / 2.00e-3     5.19e-6 / 4.00e-4 (state:dA)
#   fast_decay   token-major     4.47e-3 / 1.00e-2     5.77e-4 / 2.00e-3     2.83e-6 / 4.00e-4 (state:dA)
#   fast_decay   segments        4.18e-3 / 1.00e-2     5.33e-4 / 2.00e-3     3.09e-6 / 4.00e-4 (state:dA)
#   fast_decay   peeks           3.75e-3 / 1.00e-2     4.41e-4 / 1.00e-2     2.54e-6 / 1.00e-4 (state:dA)
#   fast_decay   stream          3.66e-3 / 1.00e-2     4.78e-4 / 1.00e-2     2.70e-7 / 1.00e-4
#   fast_decay   state_update    3.62e-3 / 1.00e-2     4.51e-4 / 1.00e-2     4.79e-7 / 1.00e-4
#   threshold    channel-major   3.62e-3 / 1.00e-2     4.44e-4 / 2.00e-3     3.91e-7 / 1.00e-4
#   threshold    token-major     7.15e-3 / 1.00e-2     5.76e-4 / 2.00e-3     5.80e-7 / 1.00e-4
#   threshold    segments        5.17e-3 / 1.00e-2     4.87e-4 / 2.00e-3     3.85e-7 / 1.00e-4
#   threshold    peeks           3.80e-3 / 1.00e-2     4.47e-4 / 1.00e-2     4.45e-7 / 1.00e-4 (state:dA)
#   threshold    stream          3.63e-3 / 1.00e-2     4.54e-4 / 1.00e-2     3.69e-7 / 1.00e-4
#   threshold    state_update    3.66e-3 / 1.00e-2     4.59e-4 / 1.00e-2     3.71e-7 / 1.00e-4
#   long_memory  channel-major   3.80e-3 / 1.00e-2     4.68e-4 / 2.00e-3     6.43e-5 / 4.00e-4 (state:dA)
#   long_memory  token-major     5.30e-3 / 1.00e-2     7.21e-4 / 2.00e-3     4.63e-6 / 1.00e-4
#   long_memory  segments        5.01e-3 / 1.00e-2     7.64e-4 / 2.00e-3     2.57e-6 / 1.00e-4
#   long_memory  peeks           3.69e-3 / 1.00e-2     4.63e-4 / 1.00e-2     1.81e-6 / 1.00e-4
#   long_memory  stream          3.81e-3 / 1.00e-2     4.73e-4 / 1.00e-2     1.18e-6 / 1.00e-4
#   long_memory  state_update    3.69e-3 / 1.00e-2     4.41e-4 / 1.00e-2     1.05e-6 / 1.00e-4
#   big_state    channel-major   3.66e-3 / 1.00e-2     4.74e-4 / 2.00e-3     2.33e-6 / 1.00e-4 (rel:last_state)
#   big_state    token-major     5.62e-3 / 1.00e-2     5.85e-4 / 2.00e-3     1.78e-6 / 1.00e-4
#   big_state    segments        5.42e-3 / 1.00e-2     5.67e-4 / 2.00e-3     1.68e-6 / 1.00e-4
#   big_state    peeks           3.73e-3 / 1.00e-2     4.29e-4 / 1.00e-2     1.06e-6 / 1.00e-4 (state:dA)
#   big_state    stream          3.41e-3 / 1.00e-2     4.53e-4 / 1.00e-2     1.33e-6 / 1.00e-4
#   big_state    state_update    3.50e-3 / 1.00e-2     4.73e-4 / 1.00e-2     5.99e-7 / 1.00e-4
#   mixed_rows   channel-major   3.83e-3 / 1.00e-2     4.61e-4 / 2.00e-3     1.40e-5 / 4.00e-4 (state:dA)
#   mixed_rows   token-major     6.24e-3 / 1.00e-2     8.01e-4 / 2.00e-3     1.97e-6 / 1.00e-4
#   mixed_rows   segments        5.03e-3 / 1.00e-2     5.18e-4 / 2.00e-3     1.63e-6 / 1.00e-4
#   mixed_rows   peeks           3.64e-3 / 1.00e-2     4.63e-4 / 1.00e-2     1.66e-6 / 1.00e-4
#   mixed_rows   stream          3.77e-3 / 1.00e-2     4.71e-4 / 1.00e-2     9.84e-7 / 1.00e-4
#   mixed_rows   state_update    3.76e-3 / 1.00e-2     4.64e-4 / 1.00e-2     1.32e-6 / 1.00e-4
# In no figure did FACTOR x r pass the family bar: the bars that decided are the families' own.
#
# Finding (fixed with this file).  long_memory, token-major (plain and segments, every length and direction) and peeks: the backward passes
# that keep delta = softplus(raw) took sigmoid(raw) as 1 - exp(-delta), which cancels for small delta.  Before the fix, on the lane-array
# build: row:ddelta 5.1e-3 .. 8.8e-3 in fp32 (bar 4e-4; peeks 7.3e-3, bar 1e-4), 8.2e-3 .. 1.05e-2 in fp16 (bar 8e-3), and the peeks
# kernels' ddelta_bias 1.6e-4 .. 2.8e-4 in bf16 / fp16 (bar 1e-4); `rel` and `rms` of ddelta stayed below every bar.  Now
# wave.h: vsigmoid_of_softplus (the series below 2^-6).  k_scant_bwd keeps its register counts (239 .. 256 VGPRs per instantiation, no scratch).
# A limit it met on the way: with C x 256 and dout x 16 in long_memory the fp16 Fo-Bi backward returned inf in ddelta --
# the raw-space partial handed from the first direction to the second in the activations' type passed 65504; the regime carries C x 8, dout x 2.
#
# MUTANTS -- made on scratch copies of the host build, never committed; the assertion that catches each (all: judge(), bar of the named
# figure) and what the scan tests the suite had before (test_emu_kernels, test_emu_delta_activated, test_timeline_train, test_stream_chunk,
# test_block_oracle) say to it:
#   (a) vsoftplus / vsoftplus2 with a plain log(1 + e) in place of the accurate log1p
#         here: every long_memory case of every family fails (out, out_pre, du, ddelta, ... at `row` and `rel`: delta itself is off by up to
#         2^-24 / delta = 3 %); the other regimes pass.  The suite had: NOT blind to it -- two cases of test_emu_kernels.py::test_scan fail (the one
#         -12 element of cases.scan_inputs); every other scan case, the block, the streaming and the timeline tests pass.
#   (b) the softplus threshold compare at 19 instead of 20
#         here: passes, and so does the suite.  It cannot be otherwise in fp32: softplus(x) - x = log1p(exp(-x)) is 5.6e-9 at x = 19, 3e-9 of x,
#         twenty times below half an ulp (6e-8); both branches return the same float on [19, 20].  threshold still holds both branches
#         against the oracle in every lane and step, which a compare at 15 (3e-7 x 15) or a wrong branch body would not survive.
#   (c) k_scant_bwd: the fp32 entry state of a block (the checkpoint as read back) rounded to bf16
#         here: every fp32 token-major and segments case of every regime fails (ddelta, dA, dC at every measure; 16-bit cases pass, their
#         checkpoints are 16-bit anyway).  The suite had: NOT blind to it either -- test_emu_kernels' fp32 token-major cases fail at 1e-4.
#   (d) the segment carry's product of decays without the range's last step (k_scant_fwd PHASE 3 / 4: dsum)
#         here: 12 segments cases fail, in the regimes whose carries cross a range boundary at weight: long_memory (fp32, row:out_pre
#         1.1e-4 .. 1.4e-4 / 1e-4), big_state (row:out_pre 1.5e-3 .. 2.2e-3, fp32 and fp16), mixed_rows (2e-3 .. 2.9e-3, fp32 and fp16); in
#         fast_decay and threshold the product is 0 with or without the step.  bf16's bar (1e-2) hides it.  The suite had:
#         test_scan_tm_segments fails too.
# So of (a) - (c) only the claim for (a) holds in part (the existing tests see it through one element, these through a whole regime), (b) is
# not observable and (c) was already caught.
# ----------------------------------------------------------------------------------------------------------------------------------------
import numpy as np
import torch

import aum_hip
import cases
import kernel_checks as KC
import timeline_train_checks as TT
from block_oracle_checks import FACTOR
from conftest import rel_err, rel_err_by, rms_err
from mamba_ssm.ops import selective_scan_interface as ssi
from oracle import oracle as O
from stream_checks import CACHE_BAR, DT, OUT_BAR

N_STATE = 16
DTYPES = ("f32", "bf16", "f16")
REGIME_NAMES = ("fast_decay", "threshold", "long_memory", "big_state", "mixed_rows")
GRID = np.array([19.75, 19.875, 20.0, 20.125, 20.25])
ROW_QUANTITIES = ("out", "out_pre", "out_nopre", "du", "ddelta", "dz")
STATE_QUANTITIES = ("dA", "dA_b", "dB", "dC")
HALF_MAX = 65504.0

# channel-major shapes (name, batch, dim, len) and the paths each is run on
CM_SHAPES = {"l65": (2, 16, 65), "l513": (1, 8, 513), "l1025": (1, 5, 1025)}
CM_ARMS = [("l65", "workgroup"), ("l65", "generic"), ("l513", "default"), ("l513", "lane_ckpt"), ("l1025", "default"), ("l1025", "ckpt")]
CM_CASES = [(s, p, m) for s, p in CM_ARMS for m in (("fwd", "rev") if s == "l1025" else ("fwd", "rev", "bidir"))]
TM_CASES = [(L, 1) for L in (9, 75, 513)] + [(513, 3)]          # (len, segments); dim 64, batch 1
PEEK_P = 1              # pack_lengths(1) = (0, 1, 1, 2, 3, 4, 19): the smallest period, and 3 / 4 / 19 rows leave a partial 8-row checkpoint block
STREAM_CHUNKS = (1, 7, 64)
STREAM_LEN, STEP_LEN, STEP_DIM = 75, 20, 70


def softplus64(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def forms_of(regime, act_family=False, dt="bf16", gated=True):
    f = ["bias"] + (["nobias"] if regime == "threshold" else [])
    if act_family and regime in ("threshold", "long_memory") and gated and dt != "f32":
        f.append("act")
    return f


def d_variants(regime):
    return (False, True) if regime == "mixed_rows" else (False,)


def make_case(regime, tag, batch, dim, length, gated, with_D, form):
    """the case tuple of cases.SCAN_CASES for a regime's run: (name, batch, dim, len, dstate, has_z, has_D, has_bias, softplus)"""
    return (f"{regime}_{tag}", batch, dim, length, N_STATE, gated, with_D, form == "bias", form != "act")


# ---- the regimes ------------------------------------------------------------------------------------------------------------------------------
def _np_states(u, dt, A, Bm, reverse):
    """fp64 recurrence -> (largest |h|, the state path's y = sum_n C h is left to the caller) states (batch, dim, N, L)"""
    batch, dim, length = u.shape
    h = np.zeros((batch, dim, A.shape[1]))
    hs = np.zeros((batch, dim, A.shape[1], length))
    for t in (range(length - 1, -1, -1) if reverse else range(length)):
        h = np.exp(dt[:, :, t, None] * A[None]) * h + (dt[:, :, t] * u[:, :, t])[:, :, None] * Bm[:, None, :, t]
        hs[..., t] = h
    return hs


def second_A(A):
    """the second direction's A of a pair, as kernel_checks derives it"""
    return (A * np.exp(np.random.default_rng(7).normal(0, 0.1, A.shape))).astype(np.float32)


def inputs(regime, case, form="bias"):
    name, batch, dim, length, dstate, has_z, has_D, has_bias, softplus = case
    assert (form == "bias") == has_bias and (form != "act") == softplus and regime in REGIME_NAMES
    r = cases._rng("domain_" + name)
    f = np.float32
    n = lambda *s: r.normal(0, 1, s)
    u, Bm, Cm, dout = n(batch, dim, length), n(batch, dstate, length), n(batch, dstate, length), n(batch, dim, length)
    z = n(batch, dim, length)
    jitter = np.exp(r.normal(0, 0.1, (dim, dstate)))
    steps = np.arange(1, dstate + 1, dtype=np.float64)[None, :]
    bias = r.uniform(-1.0, 1.0, dim)
    e_idx = np.arange(dim)
    if regime == "fast_decay":
        pre, A = r.uniform(19.25, 30.75, (batch, dim, length)), -steps * jitter
    elif regime == "threshold":
        pre = GRID[(np.arange(length)[None, None, :] + e_idx[None, :, None] + np.arange(batch)[:, None, None]) % len(GRID)]
        A, bias = -steps * jitter * 0.01, np.full(dim, 4.0)
    elif regime == "long_memory":
        level = -13.0 + 4.0 * ((e_idx * 7) % dim) / max(dim - 1, 1)                 # a level per channel over [-13, -9]
        pre = np.clip(level[None, :, None] + r.uniform(0.0, 1.0, (batch, dim, length)), -13.0, -8.0)
        A = np.repeat(-steps * 0.05, dim, axis=0)
        # the states stay at delta u B (1e-6 .. 1e-3: fp16 subnormals in the packed checkpoints); C and dout carry powers of two so that the
        # kernels' 16-bit OUTPUTS (out, du, ddelta, dz) of the quietest row are normal fp16 numbers and the row measure sees the kernel, not the
        # output format's 2^-24 quantum.  (No more than that: at C x 256, dout x 16 the raw-space ddelta that the first direction of a pair
        # hands to the second in the activations' type passes 65504 and comes back as inf in fp16 -- DESIGN.md, "Value domain".)
        Cm, dout = Cm * 8.0, dout * 2.0
    elif regime == "big_state":
        pre = np.log(np.expm1(0.05 * np.exp(r.normal(0, 0.2, (batch, dim, length)))))
        A = np.repeat(-steps * 0.02, dim, axis=0)
        dt = softplus64(pre)
        top = max(np.abs(_np_states(u, dt, a, Bm, rev)).max() for a, rev in ((A, False), (A, True), (second_A(A.astype(f)).astype(np.float64), True)))
        s = np.sqrt(2.0e4 / top)
        u, Bm, Cm = u * s, Bm * s, Cm * 1e-3
    else:
        bias = cases.dt_bias_init(r, dim).astype(np.float64)
        pre, A = r.normal(0, 0.5, (batch, dim, length)) + bias[None, :, None], -steps * jitter
        u = u * (10.0 ** ((e_idx % 5) - 2))[None, :, None]
    if form == "act":
        delta, bias = softplus64(pre), None
    elif form == "bias":
        delta = pre - bias[None, :, None]
    else:
        delta, bias = pre, None
    d = dict(u=u.astype(f), delta=delta.astype(f), A=A.astype(f), B=Bm.astype(f), C=Cm.astype(f), dout=dout.astype(f),
             z=z.astype(f) if has_z else None, D=(1.0 + r.normal(0, 0.1, dim)).astype(f) if has_D else None,
             delta_bias=None if bias is None else bias.astype(f))
    d["softplus"], d["activated"] = softplus, form == "act"
    return d


# ---- the oracle at either precision ------------------------------------------------------------------------------------------------------------
_cache = {}


def reference(d, case, dt, reverse, bidir, prec):
    """the oracle's forward and gradients on the operands as rounded to the dtype `dt`, both directions summed for a pair -> {name: array},
    channel-major.  An activated delta is a plain delta to the oracle; ddelta is taken to raw space with sigmoid(raw) = 1 - exp(-delta)."""
    key = (case, dt, reverse, bidir, prec, bool(d["activated"]))
    if key in _cache:
        return _cache[key]
    name, batch, dim, length, dstate, has_z, has_D, has_bias, softplus = case
    q = {k: KC.rq(d[k], DT[dt]) for k in ("u", "delta", "z", "B", "C", "dout")}

    def one(A, rev):
        fw = O.scan_fwd(q["u"], q["delta"], A, q["B"], q["C"], d["D"], q["z"], d["delta_bias"], softplus, rev, prec)
        g = O.scan_bwd(q["u"], q["delta"], A, q["B"], q["C"], d["D"], q["z"], d["delta_bias"], q["dout"], softplus, rev, prec)
        return fw, g

    fw, g = one(d["A"], reverse)
    res = {"out": fw["out"], "out_pre": fw["y_pre"]}
    if bidir:
        fb, gb = one(second_A(d["A"]), True)
        res = {"out": fw["out"] + fb["out"], "out_pre": fw["y_pre"] + fb["y_pre"]}
        for k in ("du", "ddelta", "dB", "dC", "dD", "dz", "ddelta_bias"):
            if g[k] is not None:
                g[k] = g[k] + gb[k]
        g["dA_b"] = gb["dA"]
    else:
        res["last_state"] = fw["last_state"]
    if d["activated"]:
        g["ddelta"] = (g["ddelta"] * -np.expm1(-q["delta"].astype(np.float64))).astype(g["ddelta"].dtype)
    res.update({k: v for k, v in g.items() if v is not None})
    _cache[key] = res
    return res


# ---- measures and bars -------------------------------------------------------------------------------------------------------------------------
def measures(k, a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = {"rel": rel_err(a, b), "rms": rms_err(a, b)}
    if k in ROW_QUANTITIES:
        m["row"] = rel_err_by(a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), 0, floor=0)
    if k in STATE_QUANTITIES:
        m["state"] = rel_err_by(a, b, 1)
    return m


def family_bar(family, dt, k):
    """the bar the family's existing check holds quantity k to"""
    if family in ("channel-major", "token-major", "segments"):       # kernel_checks.check_scan / check_scan_tm; fp16: the tol= its callers pass
        return {"f32": KC.TOL_F32, "bf16": KC.TOL_BF16, "f16": 2e-3}[dt] * (4 if k.startswith("d") else 1)
    if family == "peeks":                                            # timeline_train_checks.check_gradients
        return TT.PARAM_BAR if k in TT.Scan.PARAM else OUT_BAR[dt]
    return CACHE_BAR if k == "last_state" else OUT_BAR[dt]           # stream_checks.check_vs_oracle


WORST = {}      # (regime, family, dt) -> (error / bar, error, bar, what): what report() prints


def judge(tag, regime, family, dt, got, ref64, ref32):
    """every quantity of `got` at every measure against bar = max(family bar, FACTOR r)"""
    assert set(got) <= set(ref64), (tag, set(got) - set(ref64))
    bad, worst = {}, (0.0, 0.0, 0.0, "")
    for k, a in got.items():
        assert a.shape == ref64[k].shape, (tag, k, a.shape, ref64[k].shape)
        assert np.isfinite(a).all(), (tag, k, "not finite")
        r = measures(k, ref32[k], ref64[k])
        for m, e in measures(k, a, ref64[k]).items():
            bar = max(family_bar(family, dt, k), FACTOR * r[m])
            worst = max(worst, (e / bar, e, bar, f"{m}:{k}"))
            if not e < bar:
                bad[f"{m}:{k}"] = (float(f"{e:.3e}"), float(f"{bar:.3e}"))
    key = (regime, family, dt)
    WORST[key] = max(WORST.get(key, worst), worst)
    print(f"{' '.join(map(str, tag))}: worst {worst[3]} {worst[1]:.3e} / bar {worst[2]:.3e}")
    return bad


def report():
    lines = ["regime        family          " + "".join(f"{dt + ' error / bar':<32}" for dt in ("bf16", "f16", "f32"))]
    for regime in REGIME_NAMES:
        for family in ("channel-major", "token-major", "segments", "peeks", "stream", "state_update"):
            cells = [WORST.get((regime, family, dt)) for dt in ("bf16", "f16", "f32")]
            if any(cells):
                lines.append(f"{regime:<13} {family:<15} " + "".join(f"{'-' if c is None else f'{c[1]:.2e} / {c[2]:.2e} {c[3]}':<32}" for c in cells))
    return "\n".join(lines)


def _variants(regime, act_family, dt):
    for gated in (True, False):
        for with_D in d_variants(regime):
            for form in forms_of(regime, act_family, dt, gated):
                yield gated, with_D, form


def _finish(bad):
    assert not bad, bad


# ---- channel-major ---------------------------------------------------------------------------------------------------------------------------
def check_cm(lib, dev, regime, shape, path, mode, dt):
    """aum_selective_scan_fwd / _bwd through kernel_checks.scan_pairs(inputs=)"""
    batch, dim, length = CM_SHAPES[shape]
    reverse, bidir = mode == "rev", mode == "bidir"
    kw = {"workgroup": {}, "default": {}, "generic": dict(generic=True), "lane_ckpt": dict(lane_ckpt=True), "ckpt": dict(ckpt=True)}[path]
    bad = {}
    for gated, with_D, form in _variants(regime, False, dt):
        case = make_case(regime, shape, batch, dim, length, gated, with_D, form)
        d = inputs(regime, case, form)
        pairs = KC.scan_pairs(lib, dev, case, DT[dt], reverse, bidir, inputs=d, **kw)
        ref64, ref32 = reference(d, case, dt, reverse, bidir, "f64"), reference(d, case, dt, reverse, bidir, "f32")
        assert np.array_equal(pairs["out"][1], ref64["out"]) and np.array_equal(pairs["ddelta"][1], ref64["ddelta"])
        tag = (regime, shape, path, mode, dt, "gated" if gated else "ungated", "D" if with_D else "noD", form)
        b = judge(tag, regime, "channel-major", dt, {k: v[0] for k, v in pairs.items()}, ref64, ref32)
        if b:
            bad[tag] = b
    _finish(bad)


# ---- token-major -----------------------------------------------------------------------------------------------------------------------------
def _tm_activated(lib, dev, case, dtype, reverse, bidir, segments, d):
    """the launches of kernel_checks.scan_tm_launch with delta_activated=True (delta_act_checks.check_scan_tm_activated's, without a bias)"""
    name, batch, dim, length, dstate = case[:5]
    tm = lambda a: None if a is None else KC.T(a, dev, dtype).transpose(1, 2).contiguous()
    xz = torch.cat([tm(d["u"]), tm(d["z"])], dim=2).contiguous()
    u, z = xz[:, :, :dim], xz[:, :, dim:]
    bcm = torch.cat([tm(d["B"]), tm(d["C"])], dim=2).contiguous()
    Bm, Cm = bcm[:, :, :dstate], bcm[:, :, dstate:]
    A, A_b, D = KC.T(d["A"], dev), KC.T(second_A(d["A"]), dev) if bidir else None, KC.T(d["D"], dev)
    ck = aum_hip.scan_tm_ckpt(batch, length, dim, dstate, bidir, dev, lib=lib, dtype=dtype)
    ck.fill_(float("nan"))
    kw = dict(lib=lib, segments=segments, delta_activated=True)
    out, out_pre = aum_hip.scan_tm_fwd(u, tm(d["delta"]), A, Bm, Cm, D, z, None, True, reverse, A_b, want_out_pre=True, ckpt=ck, **kw)
    out2, _ = aum_hip.scan_tm_fwd(u, tm(d["delta"]), A, Bm, Cm, D, z, None, True, reverse, A_b, **kw)
    g = aum_hip.scan_tm_bwd(u, tm(d["delta"]), A, Bm, Cm, D, z, None, tm(d["dout"]), out_pre, ck, True, reverse, A_b, **kw)
    return out, out_pre, out2, g


def check_tm(lib, dev, regime, length, segments, mode, dt):
    """aum_scan_tm_fwd / _bwd (segments > 1: aum_scan_tm_seg_fwd / _seg_bwd) through kernel_checks.scan_tm_launch(inputs=); the [x | z] row
    layout for bf16"""
    reverse, bidir = mode == "rev", mode == "bidir"
    family = "segments" if segments > 1 else "token-major"
    bad = {}
    for gated, with_D, form in _variants(regime, True, dt):
        case = make_case(regime, f"tm{length}", 1, 64, length, gated, with_D, form)
        d = inputs(regime, case, form)
        ref64, ref32 = reference(d, case, dt, reverse, bidir, "f64"), reference(d, case, dt, reverse, bidir, "f32")
        if form == "act":
            out, out_pre, out2, g = _tm_activated(lib, dev, case, DT[dt], reverse, bidir, segments, d)
        else:
            kref, out, out_pre, out2, g = KC.scan_tm_launch(lib, dev, case, DT[dt], reverse, bidir, dt == "bf16", True, segments, d)
            assert np.array_equal(kref["out"], ref64["out"]) and np.array_equal(kref["grads"]["ddelta"], ref64["ddelta"])
        mine = dict(out=ref64["out"], out_pre=ref64["out_pre"],
                    grads={k: ref64.get(k) for k in ("du", "ddelta", "dA", "dA_b", "dB", "dC", "dD", "dz", "ddelta_bias")})
        pairs = KC.scan_tm_pairs(case, mine, out, out_pre, out2, g)
        ref64n, ref32n = dict(ref64, out_nopre=ref64["out"]), dict(ref32, out_nopre=ref32["out"])
        tag = (regime, f"tm{length}", f"seg{segments}", mode, dt, "gated" if gated else "ungated", "D" if with_D else "noD", form)
        b = judge(tag, regime, family, dt, {k: v[0] for k, v in pairs.items()}, ref64n, ref32n)
        if b:
            bad[tag] = b
    _finish(bad)


# ---- timeline training -------------------------------------------------------------------------------------------------------------------------
def _peeks_oracle(o, dout, lens, P, dtype):
    """timeline_train_checks.Scan.oracle at either precision -> {name: array} channel-major ((1, dim, total), (1, 16, total), parameters)"""
    f = lambda t: None if t is None else t.detach().to(dtype).cpu().requires_grad_(True)
    u, dl, A, B, C, D, z, bias = f(o["u"]), f(o["delta"]), f(o["A"]), f(o["B"]), f(o["C"]), f(o["D"]), f(o["z"]), f(o["bias"])
    out = ssi.selective_scan_peeks_ref(u, dl, A, B, C, D, z, bias, o["sp"], P, aum_hip.seq_map(lens, device="cpu"))
    out.backward(dout.to(dtype).cpu())
    ddelta = dl.grad
    if o["act"]:
        ddelta = ddelta * -torch.expm1(-dl.detach().double()).to(dtype)
    g = {"out": out.detach(), "du": u.grad, "ddelta": ddelta, "dz": None if z is None else z.grad, "dB": B.grad, "dC": C.grad, "dA": A.grad,
         "dD": None if D is None else D.grad, "ddelta_bias": bias.grad if bias is not None else (ddelta.sum(0) if o["act"] else None)}
    return {k: _cmaj(k, v) for k, v in g.items() if v is not None}


def _cmaj(k, t):
    a = t.detach().double().cpu().numpy()
    return a.T[None] if k in ROW_QUANTITIES + ("dB", "dC") else a


def check_peeks(lib, dev, regime, dt):
    """aum_scan_tm_peeks_fwd_ckpt / _bwd on one pack of timeline_train_checks.layout(PEEK_P), operands through Scan.operands(inputs=)"""
    P, lens = PEEK_P, TT.layout(PEEK_P)
    total, dim = sum(lens), 64
    smap = aum_hip.seq_map(lens, device=dev)
    bad = {}
    for gated, with_D, form in _variants(regime, True, "bf16"):         # the activated form in every dtype: the peeks kernels take it
        case = make_case(regime, "peeks", 1, dim, total, gated, with_D, form)
        d = inputs(regime, case, form)
        o = TT.Scan.operands(dt, dim, total, dev, 0, 0, inputs=d)
        dout = torch.tensor(np.ascontiguousarray(d["dout"][0].T)).to(DT[dt]).to(dev)
        out, _ = TT.Scan.fwd(o, smap, P, lib)
        got = dict(TT.Scan.bwd(o, dout, smap, P, lib), out=out)
        ref64, ref32 = _peeks_oracle(o, dout, lens, P, torch.float64), _peeks_oracle(o, dout, lens, P, torch.float32)
        tag = (regime, "peeks", dt, "gated" if gated else "ungated", "D" if with_D else "noD", form)
        b = judge(tag, regime, "peeks", dt, {k: _cmaj(k, v) for k, v in got.items() if v is not None}, ref64, ref32)
        if b:
            bad[tag] = b
    _finish(bad)


# ---- streaming forward ---------------------------------------------------------------------------------------------------------------------------
def scan_chunks(lib, state, o, cuts):
    """aum_scan_tm_chunk: push the row `o` (token-major operands) into `state` in chunks of `cuts` steps"""
    outs, t = [], 0
    for n in cuts:
        sl = lambda a: None if a is None else a[:, t:t + n]
        outs.append(aum_hip.scan_tm_chunk(state, sl(o["u"]), sl(o["delta"]), o["A"], sl(o["B"]), sl(o["C"]), o["D"], sl(o["z"]), o["bias"],
                                          o["sp"], o["act"], lib=lib))
        t += n
    return torch.cat(outs, dim=1)


def state_updates(lib, state, o):
    """aum_selective_state_update: the row `o` one step per call"""
    z = o["z"]
    return torch.stack([aum_hip.state_update(state, o["u"][:, t], o["delta"][:, t], o["A"], o["B"][:, t], o["C"][:, t], o["D"],
                                             None if z is None else z[:, t], o["bias"], o["sp"], lib=lib) for t in range(o["u"].shape[1])], dim=1)


def _stream_operands(d, case, dt, dev):
    tm = lambda a: None if a is None else KC.T(a, dev, DT[dt]).transpose(1, 2).contiguous()
    return {"u": tm(d["u"]), "delta": tm(d["delta"]), "z": tm(d["z"]), "B": tm(d["B"]), "C": tm(d["C"]), "A": KC.T(d["A"], dev),
            "D": KC.T(d["D"], dev), "bias": KC.T(d["delta_bias"], dev), "sp": bool(d["softplus"]), "act": bool(d["activated"])}


def check_stream(lib, dev, regime, dt, chunk):
    """chunk > 0: aum_scan_tm_chunk, the regime's row of 75 steps pushed `chunk` steps at a time into a zeroed fp32 pool; chunk 0:
    aum_selective_state_update, 20 steps of 70 channels.  Forward only: out and the pool's last state against the oracle's forward."""
    family, dim, length = ("stream", 64, STREAM_LEN) if chunk else ("state_update", STEP_DIM, STEP_LEN)
    bad = {}
    for gated, with_D, form in _variants(regime, bool(chunk), "bf16"):
        case = make_case(regime, family, 1, dim, length, gated, with_D, form)
        d = inputs(regime, case, form)
        o = _stream_operands(d, case, dt, dev)
        state = torch.zeros(1, dim, N_STATE, device=dev)
        if chunk:
            out = scan_chunks(lib, state, o, [chunk] * (length // chunk) + ([length % chunk] if length % chunk else []))
        else:
            out = state_updates(lib, state, o)
        ref64, ref32 = reference(d, case, dt, False, False, "f64"), reference(d, case, dt, False, False, "f32")
        got = {"out": KC.N(out).transpose(0, 2, 1), "last_state": KC.N(state)}
        tag = (regime, family, f"chunk{chunk}", dt, "gated" if gated else "ungated", "D" if with_D else "noD", form)
        b = judge(tag, regime, family, dt, got, ref64, ref32)
        if b:
            bad[tag] = b
    _finish(bad)


# ---- the conditions on the inputs, on the oracle alone -------------------------------------------------------------------------------------------
def check_conditions(regime, tag, batch, dim, length, dt, bidir=False):
    for gated, with_D, form in _variants(regime, True, "bf16"):
        case = make_case(regime, tag, batch, dim, length, gated, with_D, form)
        d = inputs(regime, case, form)
        for mode in ("fwd", "rev") + (("bidir",) if bidir else ()):
            ref = reference(d, case, dt, mode == "rev", mode == "bidir", "f64")
            what = (regime, tag, dt, mode, gated, with_D, form)
            for k, v in ref.items():
                assert np.isfinite(v).all(), what + (k, "the reference is not finite")
            for k in ("out", "du", "ddelta"):
                assert (np.abs(ref[k]).max(axis=2) > 0).all(), what + (k, "a (batch, channel) row of the reference is all zeros")
        q = {k: np.asarray(KC.rq(d[k], DT[dt]), np.float64) for k in ("u", "delta", "B", "C")}
        pre = q["delta"] + (0.0 if d["delta_bias"] is None else d["delta_bias"].astype(np.float64)[None, :, None])
        step = softplus64(pre) if d["softplus"] else q["delta"]
        A = d["A"].astype(np.float64)
        if regime == "big_state":
            top = max(np.abs(_np_states(q["u"], step, a, q["B"], rev)).max() for a, rev in ((A, False), (A, True), (second_A(d["A"]).astype(np.float64), True)))
            out_top = max(np.abs(reference(d, case, dt, m == "rev", m == "bidir", "f64")["out_pre"]).max() for m in ("fwd", "rev", "bidir"))
            assert 1.0e4 <= top <= 3.0e4 and top < HALF_MAX / 2, (regime, tag, dt, form, "largest state", top)
            assert out_top < HALF_MAX / 4, (regime, tag, dt, form, "largest |out|", out_top)
        if regime == "long_memory":
            assert d["D"] is None
            y = (_np_states(q["u"], step, A, q["B"], False) * q["C"][:, None]).sum(axis=2)
            share = np.abs(y).max() / np.abs(reference(d, case, dt, False, False, "f64")["out_pre"]).max()
            assert abs(share - 1.0) < 1e-9, (regime, tag, dt, form, "the state path's share of out", share)
            assert step.max() < 4e-4 and step.min() > 1.5e-6, (regime, tag, dt, form, "delta", step.min(), step.max())
        if regime == "fast_decay":
            assert pre.min() >= 19.0 and pre.max() <= 31.0 and (pre > 20).any() and (pre < 20).any()
        if regime == "threshold" and form != "act":
            assert np.isin(pre, GRID).all() and all((pre == v).any() for v in GRID), (regime, tag, dt, form, "delta + bias left the grid")
