"""Checks of streaming PREFILL shared by tests/test_stream_prefill.py (lane-array library, host tensors) and
tests/test_gpu_stream_prefill.py (libaum_hip.so on the MI355X): aum_scan_tm_fwd_state (the token-major scan with state in / state out),
aum_hip.conv1d_tm_prefill, Mamba.prefill_chunk, Mamba.forward(inference_params) at offset 0 and AudioMamba.stream_prefill(_many).

Expected values never come from the kernel under test.  Outputs and exit states are oracle.scan_fwd in fp64 on the sequence FROM ITS
START (a non-zero entry state is the oracle's last_state behind a prefix), fed the inputs as rounded to the activations' dtype.
Bars:
  outputs   the bars tests/kernel_checks.py holds scan_tm_fwd to and tests/stream_checks.py holds scan_tm_chunk to: rel_err and rms_err
            below 1e-4 (fp32 rows) / 1e-2 (16-bit rows).
  states    STATE_BAR = 2 x the rel_err of the EXISTING aum_scan_tm_chunk's exit state against the same fp64 oracle at the same shapes
            on the lane-array build (chunk_state_error below measures it: 1.705e-07, the worst of the 24 + 3 cases of this file; STATE_BAR = 3.41e-07, recorded in
            profiles/r13_stream_prefill.txt) -- both kernels run the same fp32 recurrence from the same inputs, the factor two is
            for the re-association of the segmented carry pass.
Bitwise: a zero entry state gives scan_tm_fwd's bits (uncut and cut the same way), and the uncut form does not depend on how a stream is
cut into calls."""
import contextlib

import numpy as np
import torch

import aum_hip
import stream_checks as sc
from conftest import rel_err, rms_err
from oracle import oracle

DT = sc.DT
OUT_BAR = sc.OUT_BAR                         # = kernel_checks.TOL_F32 / TOL_BF16
CHUNK_STATE_ERR = 1.705e-07                   # measured: chunk_state_error(emu library, "cpu")
STATE_BAR = 2 * CHUNK_STATE_ERR
TS = (1, 3, 7, 8, 9, 64, 129, 513)
# (delta form, z, D, bias, x/z halves of one xz tensor, prefix length behind which the entry state is taken (0: zero))
KINDS = [("sp", True, True, True, True, 5), ("act", True, True, True, False, 11), ("raw", False, False, False, False, 0),
         ("sp", False, True, True, False, 3), ("act", True, False, True, True, 0), ("raw", True, True, True, True, 9)]


def _kernel_cases():
    """every T x every dtype; the option sets, batch in {1, 3} and dim in {64, 256} rotate through them (an activated delta is a 16-bit form)"""
    out = []
    for i, T in enumerate(TS):
        for j, dt in enumerate(("f32", "bf16", "f16")):
            n = 3 * i + j
            kind = KINDS[n % len(KINDS)]
            if dt == "f32" and kind[0] == "act":
                kind = ("sp",) + kind[1:]
            out.append(((T, dt, kind, n), (1, 3)[n % 2], (64, 256)[(n // 2) % 2], 1))
    return out


KERNEL_CASES = _kernel_cases()
# the segmented form: (case, batch, dim, forced segments) -- 1024 cut in 2 and in 8, 1025 in 4 (ragged last range)
SEG_CASES = [((1024, "bf16", KINDS[0], 101), 1, 64, 2), ((1024, "f32", KINDS[3], 102), 3, 64, 8), ((1025, "f16", KINDS[1], 103), 1, 256, 4)]


def kcase_id(c):
    case, batch, dim, seg = c
    return f"{sc.case_id(case)}-b{batch}-d{dim}-s{seg}"


def _np(t):
    return t.detach().float().cpu().numpy()


def run_state(s, lib, state_in, state_out, segments=1, lo=0, hi=None):
    """aum_hip.scan_tm_fwd_state on rows [lo, hi) of a scan_setup"""
    o = s["ops"]
    sl = lambda a: None if a is None else a[:, lo:hi]
    return aum_hip.scan_tm_fwd_state(sl(o["u"]), sl(o["delta"]), o["A"], sl(o["B"]), sl(o["C"]), o["D"], sl(o["z"]), o["bias"], o["sp"], o["act"],
                                     state_in=state_in, state_out=state_out, segments=segments, lib=lib)


def chunk_state_error(lib, device):
    """the yardstick of STATE_BAR: rel_err of the exit state of the existing aum_scan_tm_chunk against the fp64 oracle, worst case of this file"""
    worst = 0.0
    for case, batch, dim, _ in KERNEL_CASES + SEG_CASES:
        s = sc.scan_setup(case, device, batch=batch, dim=dim)
        _, state = sc.scan_run(s, [s["T"]], lib)
        e = rel_err(_np(state), s["ref_state"])
        print(f"scan_tm_chunk state vs oracle {kcase_id((case, batch, dim, 1))}: {e:.3e}")
        worst = max(worst, e)
    return worst


# ---- 1. state hand-off at the kernel ---------------------------------------------------------------
def check_kernel_handoff(c, lib, device):
    case, batch, dim, seg = c
    s = sc.scan_setup(case, device, batch=batch, dim=dim)
    o, dt = s["ops"], s["dt"]
    # a zero entry state: the bits of scan_tm_fwd, cut the same way; None and a tensor of zeros are the same thing
    ref_tm, _ = aum_hip.scan_tm_fwd(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"], lib=lib, segments=seg,
                                    delta_activated=o["act"])
    out0 = run_state(s, lib, None, None, seg)
    z0 = torch.zeros_like(s["entry"])
    z1 = torch.full_like(s["entry"], float("nan"))
    out1 = run_state(s, lib, z0, z1, seg)
    assert torch.equal(out0, ref_tm), "state_in=None differs from scan_tm_fwd"
    assert torch.equal(out1, ref_tm) and not z0.any(), "a zero state_in differs from scan_tm_fwd (or state_in was written)"
    # the carried entry state: out and state_out against the fp64 oracle on the sequence from its start
    exit_ = torch.full_like(s["entry"], float("nan"))
    entry = s["entry"].clone()
    out = run_state(s, lib, entry, exit_, seg)
    e_out, r_out, e_st = rel_err(_np(out), s["ref_out"]), rms_err(_np(out), s["ref_out"]), rel_err(_np(exit_), s["ref_state"])
    print(f"scan_tm_fwd_state {kcase_id(c)}: out {e_out:.3e} rms {r_out:.3e} (bar {OUT_BAR[dt]:.0e}), state_out {e_st:.3e} (bar {STATE_BAR:.1e})")
    assert out.dtype == DT[dt] and torch.equal(entry, s["entry"]), "state_in was written"
    assert e_out < OUT_BAR[dt] and r_out < OUT_BAR[dt]
    assert e_st < STATE_BAR
    if not s["entry"].any():
        assert torch.equal(out, ref_tm)
    # state_out may be state_in
    st = s["entry"].clone()
    out2 = run_state(s, lib, st, st, seg)
    assert torch.equal(out2, out) and torch.equal(st, exit_), "advancing in place differs from state_in -> state_out"


def check_refusals(lib, device):
    import pytest
    s = sc.scan_setup((9, "bf16", KINDS[0], 7), device, batch=1, dim=64)
    o = s["ops"]
    ok = lambda **kw: aum_hip.scan_tm_fwd_state_supported(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], True, False, **kw)
    st = s["entry"]
    assert ok() and ok(state_in=st, state_out=st) and ok(segments=8)
    assert not ok(state_in=st.double()) and not ok(state_out=st[:, :, :8]) and not ok(state_in=st.transpose(1, 2).contiguous().transpose(1, 2))
    assert not ok(state_in=torch.zeros(2, 64, 16, device=device)) and not ok(segments=0) and not ok(segments=aum_hip.SCAN_TM_MAX_SEGMENTS + 1)
    pad = torch.zeros(64 * 16 + 1, device=device)[1:].view(1, 64, 16)                  # 4-byte aligned only
    assert not ok(state_out=pad)
    keep = st.clone()
    with pytest.raises(RuntimeError, match="scan_tm_fwd_state"):
        run_state(s, lib, st, st.double())
    assert torch.equal(st, keep)
    # the C entry point refuses what it has no kernels for: checkpoints, the pre-gate copy, a second direction, reverse time
    sa = aum_hip.ScanTmFwdStateArgs()
    a = sa.base
    out = torch.empty(o["u"].shape, dtype=o["u"].dtype, device=device)
    u, d, z = o["u"].contiguous(), o["delta"].contiguous(), o["z"].contiguous()
    Bm, Cm = o["B"].contiguous(), o["C"].contiguous()
    a.u, a.delta, a.z, a.B, a.C, a.A, a.out = (t.data_ptr() for t in (u, d, z, Bm, Cm, o["A"], out))
    for n in ("u", "delta", "z", "out"):
        setattr(a, n + "_bs", 9 * 64), setattr(a, n + "_ts", 64)
    a.B_bs = a.C_bs = 9 * 16
    a.B_ts = a.C_ts = 16
    a.batch, a.dim, a.len, a.dstate, a.dtype, sa.segments = 1, 64, 9, 16, aum_hip.AUM_BF16, 1
    call = lambda: lib.c.aum_scan_tm_fwd_state(aum_hip.C_byref(sa), lib.stream(u))
    assert call() == 0
    scratch = torch.zeros(4096, device=device)
    for field, flag in (("ckpt", 0), ("out_pre", 0), ("A_b", 0), (None, aum_hip.SCAN_REVERSE)):
        if field:
            setattr(a, field, scratch.data_ptr())
        a.flags = flag
        assert call() == -4, field or "reverse"
        if field:
            setattr(a, field, None)
    a.flags = 0
    sa.segments = 2                             # segments without scratch
    assert call() == -1
    if device != "cpu":
        torch.cuda.synchronize()


# ---- 2. partition ----------------------------------------------------------------------------------
def check_partition_uncut(T, dt, kind, lib, device, batch=1, dim=64):
    """every two-way cut of T: out and state_out bit for bit those of one call (the state crosses as exact fp32, a step is the same
    instruction sequence wherever it falls in a call or in an 8-step block)"""
    s = sc.scan_setup((T, dt, kind, 40 + T), device, batch=batch, dim=dim)
    whole_state = s["entry"].clone()
    whole = run_state(s, lib, whole_state, whole_state)
    for t1 in range(1, T):
        st = s["entry"].clone()
        a = run_state(s, lib, st, st, 1, 0, t1)
        b = run_state(s, lib, st, st, 1, t1, T)
        assert torch.equal(torch.cat((a, b), dim=1), whole), f"outputs differ for the cut {t1} + {T - t1}"
        assert torch.equal(st, whole_state), f"states differ for the cut {t1} + {T - t1}"


def check_partition_segmented(dt, kind, cut, seg, lib, device):
    """L = 1024 in two calls, each cut into `seg` time ranges: the carry pass re-associates the recurrence, so the yardstick is the oracle"""
    s = sc.scan_setup((1024, dt, kind, 77), device, batch=1, dim=64)
    st = s["entry"].clone()
    a = run_state(s, lib, st, st, seg, 0, cut)
    b = run_state(s, lib, st, st, seg, cut, 1024)
    out = torch.cat((a, b), dim=1)
    e_out, r_out, e_st = rel_err(_np(out), s["ref_out"]), rms_err(_np(out), s["ref_out"]), rel_err(_np(st), s["ref_state"])
    print(f"segmented partition {cut} + {1024 - cut}, {seg} ranges, {dt}: out {e_out:.3e} rms {r_out:.3e} (bar {OUT_BAR[dt]:.0e}), state {e_st:.3e} "
          f"(bar {STATE_BAR:.1e})")
    assert e_out < OUT_BAR[dt] and r_out < OUT_BAR[dt]
    assert e_st < STATE_BAR


# ---- 3. hand-over to the live kernels ------------------------------------------------------------------
CONV_CASES = [(T, dt, k, i) for i, (T, dt, k) in enumerate(
    (T, ("f32", "bf16", "f16")[n % 3], sc.CONV_KINDS[n % len(sc.CONV_KINDS)]) for n, T in enumerate(TS + (2, 4)))]


def check_conv_prefill(case, lib, device):
    """conv1d_tm_prefill against conv1d_stream on the same window: the window bit for bit (it holds the inputs themselves), the outputs to
    the bar, both to the fp64 oracle; a zero window = the plain causal conv"""
    s = sc.conv_setup(case, device, batch=2, dim=72)
    dt = s["dt"]
    c_live, c_pre = s["entry"].clone(), s["entry"].clone()
    y_live = aum_hip.conv1d_stream(s["x"], c_live, s["w"], s["bias"], s["silu"], lib=lib)
    y_pre = aum_hip.conv1d_tm_prefill(s["x"], c_pre, s["w"], s["bias"], s["silu"], lib=lib)
    e_live, e_ref = rel_err(_np(y_pre), _np(y_live)), rel_err(_np(y_pre), s["ref_out"])
    print(f"conv1d_tm_prefill {sc.case_id(case)}: vs conv1d_stream {e_live:.3e}, vs oracle {e_ref:.3e} (bar {OUT_BAR[dt]:.0e})")
    assert y_pre.shape == s["x"].shape and y_pre.dtype == DT[dt]
    assert torch.equal(c_pre, c_live), "conv_state differs from conv1d_stream's"
    assert rel_err(_np(c_pre), s["ref_state"]) == 0.0
    assert e_live < OUT_BAR[dt] and e_ref < OUT_BAR[dt]
    zero = torch.zeros_like(s["entry"])
    y0 = aum_hip.conv1d_tm_prefill(s["x"], zero, s["w"], s["bias"], s["silu"], lib=lib)
    assert torch.equal(y0, aum_hip.conv1d_tm_fwd(s["x"], s["w"], s["bias"], s["silu"], lib=lib)), "a zero window differs from the plain causal conv"


@contextlib.contextmanager
def product_lib(lib):
    """the modules call aum_hip.get(): the library under test in its place"""
    old, aum_hip._product = aum_hip._product, lib
    try:
        yield
    finally:
        aum_hip._product = old


@contextlib.contextmanager
def counting(obj, name):
    """calls of obj.name counted while the block runs -> a one-element list: a check that means to cover a path asserts it was taken,
    so a dispatch that quietly falls back to the old path fails the test"""
    real, n = getattr(obj, name), [0]

    def wrapper(*a, **kw):
        n[0] += 1
        return real(*a, **kw)

    setattr(obj, name, wrapper)
    try:
        yield n
    finally:
        setattr(obj, name, real)


def _block_oracle(m, x):
    """the causal block in fp64 on the module's own in_proj rows (as rounded to the working dtype) -> (out (batch, L, d_model), last state)"""
    f = lambda t: t.detach().double().cpu().numpy()
    B, L, _ = x.shape
    with torch.no_grad():
        xz = m.in_proj(x.reshape(B * L, -1)).view(B, L, -1)
    A = -np.exp(f(m.A_log))
    st = oracle.inner_fwd(np.ascontiguousarray(f(xz).transpose(0, 2, 1)), f(m.conv1d.weight).reshape(m.d_inner, -1), f(m.conv1d.bias), f(m.x_proj.weight),
                          f(m.dt_proj.weight), f(m.out_proj.weight), None, A, f(m.D), f(m.dt_proj.bias), prec="f64")
    last = oracle.scan_fwd(st["xc"], st["delta"], A, st["B"], st["C"], f(m.D), st["z"], f(m.dt_proj.bias), True, prec="f64")["last_state"]
    return st["out"], last


def make_mamba(d_model, dt_rank, dt, device):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(5)
    return Mamba(d_model, dt_rank=dt_rank, layer_idx=0, bimamba_type="none").eval().to(device).to(DT[dt])


def check_mamba_handover(d_model, dt_rank, dt, T, batch, lib, device, prefix=5):
    """caches made non-zero by `prefix` tokens of step_chunk; then prefill_chunk of T tokens and step_chunk of 8 more, against step_chunk
    over all T + 8 and against the fp64 oracle over the whole sequence.  d_model 32 (dt_rank 2): d_inner 64, the library x/dt products;
    d_model 128 with dt_rank 24: d_inner 256, the smallest width aum_xdt_tm_fwd takes (on the device, 16-bit).  prefill_chunk must run
    its own path -- exactly one aum_hip.scan_tm_fwd_state call, no step_chunk inside it -- and on the device aum_xdt_tm_fwd exactly where
    the widths are its own.  The fp32 state against step_chunk's: STATE_BAR (the same
    recurrence on the same conv outputs); against the oracle, which keeps fp64 where the block rounds xc, x_dbl and delta to the working
    dtype: the outputs' bar."""
    m = make_mamba(d_model, dt_rank, dt, device)
    torch.manual_seed(T)
    L = prefix + T + 8
    x = torch.randn(batch, L, d_model, device=device).to(DT[dt])
    with torch.no_grad(), product_lib(lib):
        c0, s0 = (t.float() for t in m.allocate_inference_cache(batch, 0))
        m.step_chunk(x[:, :prefix], c0, s0)
        assert c0.any() and s0.any()
        ca, sa, cb, sb = c0.clone(), s0.clone(), c0.clone(), s0.clone()
        with counting(aum_hip, "scan_tm_fwd_state") as n_state, counting(m, "step_chunk") as n_live, counting(aum_hip, "xdt_tm_fwd") as n_xdt:
            o1, _, _ = m.prefill_chunk(x[:, prefix:prefix + T], ca, sa)
        assert n_state[0] == 1 and n_live[0] == 0, f"prefill_chunk fell back to step_chunk ({n_state[0]} scan_tm_fwd_state, {n_live[0]} step_chunk calls)"
        assert n_xdt[0] == int(device != "cpu" and d_model == 128 and dt != "f32"), f"{n_xdt[0]} aum_xdt_tm_fwd calls"
        o2, _, _ = m.step_chunk(x[:, prefix + T:], ca, sa)
        got = torch.cat((o1, o2), dim=1)
        live, _, _ = m.step_chunk(x[:, prefix:], cb, sb)
    ref_out, ref_state = _block_oracle(m, x)
    e = {"out vs step_chunk": rel_err(_np(got), _np(live)), "state vs step_chunk": rel_err(_np(sa), _np(sb)),
         "out vs oracle": rel_err(_np(got), ref_out[:, prefix:]), "state vs oracle": rel_err(_np(sa), ref_state)}
    print(f"Mamba({d_model}, dt_rank={dt_rank}) {dt} batch {batch} T {T}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert got.shape == (batch, T + 8, d_model) and got.dtype == DT[dt]
    assert torch.equal(ca, cb), "conv_state differs from step_chunk's"
    assert e["out vs step_chunk"] < OUT_BAR[dt] and e["out vs oracle"] < OUT_BAR[dt] and e["state vs oracle"] < OUT_BAR[dt]
    assert e["state vs step_chunk"] < STATE_BAR


# ---- 4. model --------------------------------------------------------------------------------------
def _autocast(device):
    return torch.autocast(device_type=torch.device(device).type, dtype=torch.bfloat16)


def check_model_prefill(lib, device):
    """causal AuM (depth 2, embed_dim 128: d_inner 256, dt_rank 8) on a (128, 256) spectrogram in bf16 autocast: 10 columns by
    stream_prefill, 6 by stream_push one by one, stream_read -- against model(spec) and against 16 single-column pushes (the bar of
    stream_checks.check_model_stream under autocast)"""
    model = sc.make_causal_aum(128, device, depth=2)
    torch.manual_seed(12)
    spec = torch.randn(2, 256, 128, device=device)
    bar = 2e-2
    with torch.no_grad(), _autocast(device), product_lib(lib):
        full = model(spec, return_features=True)          # the features in front of the head: 2 x 128 values, not 2 x 7 logits
        cache = model.allocate_inference_cache(2)
        with counting(aum_hip, "scan_tm_fwd_state") as n_state:
            assert model.stream_prefill(spec[:, :160], cache) == 10
        assert n_state[0] == len(model.layers), f"stream_prefill ran {n_state[0]} scan_tm_fwd_state launches for {len(model.layers)} blocks"
        for c in range(10, 16):
            assert model.stream_push(spec[:, 16 * c:16 * (c + 1)], cache) == c + 1
        got = model.stream_read(cache, return_features=True)
        live = model.allocate_inference_cache(2)
        for c in range(16):
            model.stream_push(spec[:, 16 * c:16 * (c + 1)], live)
        ref = model.stream_read(live, return_features=True)
        # read=True is stream_read behind the push
        c2 = model.allocate_inference_cache(2)
        n, logits = model.stream_prefill(spec, c2, read=True, return_features=True)
        assert n == 16 and torch.equal(logits, model.stream_read(c2, return_features=True))
    e_full, e_live, e_all = rel_err(_np(got), _np(full)), rel_err(_np(got), _np(ref)), rel_err(_np(logits), _np(full))
    print(f"model prefill: read vs model(spec) {e_full:.3e}, vs 16 pushes {e_live:.3e}, all 16 columns prefilled vs model(spec) {e_all:.3e} (bar {bar:.0e})")
    for (ca, sa), (cb, sb) in zip(cache["layers"].values(), live["layers"].values()):
        assert torch.equal(ca, cb), "a conv window differs from the pushed session's"
    assert e_full < bar and e_live < bar and e_all < bar


def check_model_prefill_many(lib, device):
    """stream_prefill_many on shuffled rows of a pool = stream_prefill of each session alone; the other rows keep their sentinel"""
    model = sc.make_causal_aum(128, device, depth=2)
    torch.manual_seed(13)
    spec = torch.randn(3, 256, 128, device=device)
    rows, ks = [4, 1, 3], [10, 3, 16]
    with torch.no_grad(), _autocast(device), product_lib(lib):
        pool = model.allocate_stream_pool(6)
        for c, s in pool["layers"].values():
            c.fill_(7.0)
            s.fill_(-3.0)
        model.stream_reset(pool, rows)
        assert model.stream_prefill_many([spec[i, :16 * k] for i, k in enumerate(ks)], pool, rows) == ks
        assert pool["columns"] == [0, 3, 0, 16, 10, 0]
        for i, (r, k) in enumerate(zip(rows, ks)):
            solo = model.allocate_inference_cache(1)
            model.stream_prefill(spec[i:i + 1, :16 * k], solo)
            for (c, s), (cs, ss) in zip(pool["layers"].values(), solo["layers"].values()):
                assert torch.equal(c[r], cs[0]) and torch.equal(s[r], ss[0]), f"session {r} differs from a stream_prefill of its own"
        for c, s in pool["layers"].values():
            for r in (0, 2, 5):
                assert bool((c[r] == 7.0).all()) and bool((s[r] == -3.0).all()), f"row {r} was touched"
        # the sessions go on live from there
        assert model.stream_push_many([spec[1, 48:64]], pool, [1]) == [4]


def check_model_refusals(lib, device):
    import pytest
    model = sc.make_causal_aum(128, device, depth=2)
    spec = torch.randn(2, 256, 128, device=device)

    def snapshot(c):
        return [t.clone() for pair in c["layers"].values() for t in pair], (list(c["columns"]) if isinstance(c["columns"], list) else c["columns"])

    def same(c, snap):
        return all(torch.equal(a, b) for a, b in zip(snapshot(c)[0], snap[0])) and snapshot(c)[1] == snap[1]

    with torch.no_grad(), _autocast(device), product_lib(lib):
        cache = model.allocate_inference_cache(2)
        model.stream_prefill(spec[:, :112], cache)
        snap = snapshot(cache)
        for bad in (spec[:, :160], spec[:1, :16], spec[:, :24], spec[:, :16, :64], spec[0, :16]):      # too many columns, wrong shapes
            with pytest.raises(ValueError):
                model.stream_prefill(bad, cache)
            assert same(cache, snap)
        pool = model.allocate_stream_pool(3)
        with pytest.raises(ValueError):
            model.stream_prefill(spec[:, :16], pool)
        model.stream_prefill_many([spec[0, :224]], pool, [2])
        psnap = snapshot(pool)
        for specs, rows in (([spec[0, :16], spec[1, :48]], [0, 2]), ([spec[0, :16]], [3]), ([spec[0, :16], spec[1, :16]], [1, 1]),
                            ([spec[0, :24]], [0]), ([spec[0, :16]], [0, 1])):
            with pytest.raises(ValueError):
                model.stream_prefill_many(specs, pool, rows)
            assert same(pool, psnap)
        with pytest.raises(ValueError):
            model.stream_prefill_many([spec[0, :16]], cache, [0])


# ---- 5. the reference's prefill contract ---------------------------------------------------------------
def check_forward_offset0(d_model, lib, device, L=37, steps=6):
    """Mamba.forward(x, inference_params) at seqlen_offset == 0 leaves caches from which step() continues: all outputs against the fp64
    oracle over the whole sequence, the state behind the prompt against the oracle's (fp32 module: the 1e-4 bar).  The new path
    (prefill_chunk) is taken exactly where the module says it is -- on a device with widths for which ssi.token_major_ok holds (d_model
    128: dt_rank 8) -- and the un-fused branch elsewhere (the host; d_model 32: dt_rank 2); the caller says which it means to cover."""
    from types import SimpleNamespace
    import mamba_ssm.ops.selective_scan_interface as ssi
    m = make_mamba(d_model, "auto", "f32", device)
    new_path = device != "cpu" and ssi.token_major_ok(m.d_inner, m.d_state, m.d_conv, m.dt_rank, torch.float32)
    torch.manual_seed(9)
    x = torch.randn(2, L + steps, d_model, device=device)
    params = SimpleNamespace(key_value_memory_dict={}, seqlen_offset=0)
    with torch.no_grad(), product_lib(lib):
        with counting(m, "prefill_chunk") as n_pre, counting(aum_hip, "scan_tm_fwd_state") as n_state:
            outs = [m(x[:, :L], inference_params=params)]
        assert n_pre[0] == n_state[0] == int(new_path), f"forward at offset 0: {n_pre[0]} prefill_chunk / {n_state[0]} scan_tm_fwd_state calls"
        conv_c, ssm_c = params.key_value_memory_dict[0]
        _, state_L = _block_oracle(m, x[:, :L])
        e_state = rel_err(_np(ssm_c), state_L)
        for t in range(L, L + steps):
            params.seqlen_offset = t
            outs.append(m(x[:, t:t + 1], inference_params=params))
    ref_out, _ = _block_oracle(m, x)
    e_out = rel_err(_np(torch.cat(outs, dim=1)), ref_out)
    print(f"Mamba({d_model}).forward at offset 0 ({'prefill_chunk' if new_path else 'un-fused branch'}), then {steps} steps: out vs oracle {e_out:.3e}, "
          f"state behind the prompt {e_state:.3e} (bar 1e-4)")
    assert e_out < OUT_BAR["f32"] and e_state < OUT_BAR["f32"]
    return new_path
