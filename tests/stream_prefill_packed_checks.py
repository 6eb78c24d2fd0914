"""Checks of PACKED streaming prefill shared by tests/test_stream_prefill_packed.py (lane-array library, host tensors) and
tests/test_gpu_stream_prefill_packed.py (libaum_hip.so on the MI355X): aum_conv1d_tm_prefill_var, aum_scan_tm_fwd_state_var,
Mamba.prefill_chunk(seq_map=) and AudioMamba.stream_prefill_many(packed=True).

Expected values never come from the kernels under test.  They are the fp64 oracle as tests/stream_prefill_checks.py uses it
(sc.scan_setup / sc.conv_setup: oracle.scan_fwd / oracle.conv1d_fwd on the sequence from its start) with that file's bars (OUT_BAR,
STATE_BAR: imported), or the existing fixed-batch kernels that file already holds to the oracle -- aum_hip.conv1d_tm_prefill and
aum_hip.scan_tm_fwd_state at batch 1 on a session alone -- to which the packed kernels must be BIT-EQUAL: the conv is not recurrent, and
the scan runs the same steps over the same ranges.

A pack is built from one setup of batch = number of sessions: session i takes the first lens[i] rows of batch entry i, so every session
has an oracle of its own (the oracle is causal: a prefix of the sequence is the sequence).  Pools have 6 rows, the sessions own the
shuffled rows ROWS and every other row holds a sentinel."""
import numpy as np
import torch

import aum_hip
import stream_checks as sc
import stream_prefill_checks as pc
from conftest import rel_err, rms_err
from oracle import oracle

DT = sc.DT
OUT_BAR, STATE_BAR = pc.OUT_BAR, pc.STATE_BAR
NROWS = 6
ROWS = (4, 1, 3, 0, 5, 2, 6)            # pool rows of sessions 0, 1, ...: (the last one only for packs of seven, on a pool of 7)
SENT = 7.0
CONV_LENS = (1, 2, 3, 4, 0, 9, 130)     # T < width, T == width, an empty session, more than one 64-step chunk
SCAN_LENS = (9, 1, 0, 40, 3, 64)
CUT_LENS = (40, 24, 9, 1, 0)            # range_len 8: every own cut has ranges of 8 steps too
_np = pc._np


def _pack(parts):
    return torch.cat(parts, dim=0)


def _pool(rows_of, entry, nrows, device):
    """a pool of sentinel rows with session i's entry in row rows_of[i]"""
    pool = torch.full((nrows,) + tuple(entry.shape[1:]), SENT, dtype=torch.float32, device=device)
    for i, r in enumerate(rows_of):
        pool[r] = entry[i]
    return pool


def _foreign_untouched(pool, used, what):
    for r in range(pool.shape[0]):
        if r not in used:
            assert bool((pool[r] == SENT).all()), f"{what}: foreign row {r} was touched"


# ---- conv ------------------------------------------------------------------------------------------
def conv_pack(dt, kind, dim, device, lens=CONV_LENS, seed=0, zero_window=False):
    n = len(lens)
    s = sc.conv_setup((max(lens), dt, kind, 60 + seed), device, batch=n, dim=dim)
    width = kind[0]
    entry = torch.zeros_like(s["entry"]) if zero_window else s["entry"]         # the entry window holds inputs as rounded to dt: exact in dt
    halves = kind[3]
    if halves:                           # packed x rows as the first half of wider rows
        d = s["x"].shape[2]
        wide = torch.zeros(sum(lens), 2 * d, dtype=DT[dt], device=device)
        wide[:, :d] = _pack([s["x"][i, :L] for i, L in enumerate(lens)])
        x = wide[:, :d]
    else:
        x = _pack([s["x"][i, :L] for i, L in enumerate(lens)])
    rows = ROWS[:n]
    return {"s": s, "x": x, "lens": lens, "rows": rows, "entry": entry, "width": width, "nrows": max(NROWS, n), "zero": zero_window}


def check_conv(dt, kind, dim, lib, device, zero_window=False):
    """per session: y and the new window bit-equal to conv1d_tm_prefill at batch 1 on the session alone, inside the bars against
    conv1d_stream (the bars of stream_prefill_checks.check_conv_prefill), against the oracle; foreign and empty rows untouched"""
    p = conv_pack(dt, kind, dim, device, zero_window=zero_window)
    s, lens, rows = p["s"], p["lens"], p["rows"]
    pool = _pool(rows, p["entry"], p["nrows"], device)
    keep = pool.clone()
    m = aum_hip.seq_map(lens, rows, device=device)
    y = aum_hip.conv1d_tm_prefill_var(p["x"], pool, s["w"], s["bias"], s["silu"], seq_map=m, lib=lib)
    assert y.shape == p["x"].shape and y.dtype == DT[dt] and y.is_contiguous()
    o = 0
    for i, (L, r) in enumerate(zip(lens, rows)):
        if L == 0:
            assert torch.equal(pool[r], keep[r]), "the empty session's window was touched"
            continue
        xi = s["x"][i:i + 1, :L]
        w_solo, w_live = p["entry"][i:i + 1].clone(), p["entry"][i:i + 1].clone()
        y_solo = aum_hip.conv1d_tm_prefill(xi, w_solo, s["w"], s["bias"], s["silu"], lib=lib)
        y_live = aum_hip.conv1d_stream(xi, w_live, s["w"], s["bias"], s["silu"], lib=lib)
        got = y[o:o + L].unsqueeze(0)
        assert torch.equal(got, y_solo), f"session {i} (len {L}): y differs from conv1d_tm_prefill on the session alone"
        assert torch.equal(pool[r:r + 1], w_solo), f"session {i} (len {L}): the window differs from conv1d_tm_prefill's"
        assert torch.equal(pool[r:r + 1], w_live), f"session {i} (len {L}): the window differs from conv1d_stream's"
        e_live = rel_err(_np(got), _np(y_live))
        assert e_live < OUT_BAR[dt], f"session {i}: vs conv1d_stream {e_live:.3e}"
        if not zero_window:              # the setup's oracle starts from the setup's window
            e_ref = rel_err(_np(got), s["ref_out"][i:i + 1, :L])
            print(f"conv1d_tm_prefill_var {dt} dim {dim} session {i} len {L}: vs conv1d_stream {e_live:.3e}, vs oracle {e_ref:.3e} (bar {OUT_BAR[dt]:.0e})")
            assert e_ref < OUT_BAR[dt]
        o += L
    _foreign_untouched(pool, rows, "conv")


# ---- scan ------------------------------------------------------------------------------------------
def scan_pack(dt, kind, dim, device, lens, seed=0):
    n = len(lens)
    s = sc.scan_setup((max(lens), dt, kind, 80 + seed), device, batch=n, dim=dim)
    o = s["ops"]
    cut = lambda a: None if a is None else _pack([a[i, :L] for i, L in enumerate(lens)])
    halves = kind[4] and o["z"] is not None
    if halves:                           # packed u / z rows as the two halves of one (total, 2 dim) tensor
        xz = torch.cat((cut(o["u"]), cut(o["z"])), dim=1)
        u, z = xz[:, :dim], xz[:, dim:]
    else:
        u, z = cut(o["u"]), cut(o["z"])
    bc = torch.cat((cut(o["B"]), cut(o["C"])), dim=1)                           # B, C as column blocks of one packed row
    packed = {"u": u, "delta": cut(o["delta"]), "z": z, "B": bc[:, :16], "C": bc[:, 16:]}
    # per-session oracle: the setup's sequence cut at lens[i] rows (entry state behind the setup's prefix)
    return {"s": s, "ops": packed, "lens": tuple(lens), "rows": ROWS[:n], "nrows": max(NROWS, n)}


def run_var(p, lib, pool, range_len=0, ops=None, lens=None, rows=None):
    o, k = p["s"]["ops"], (ops or p["ops"])
    m = aum_hip.seq_map(lens or p["lens"], rows or p["rows"], device=pool.device)
    return aum_hip.scan_tm_fwd_state_var(pool, k["u"], k["delta"], o["A"], k["B"], k["C"], o["D"], k["z"], o["bias"], o["sp"], o["act"], seq_map=m,
                                         range_len=range_len, lib=lib)


def _solo(p, i, L, lib, segments):
    """scan_tm_fwd_state at batch 1 on session i alone, from the same entry state -> (out (1, L, dim), exit state (1, dim, 16))"""
    o = p["s"]["ops"]
    sl = lambda a: None if a is None else a[i:i + 1, :L]
    st = p["s"]["entry"][i:i + 1].clone()
    out = aum_hip.scan_tm_fwd_state(sl(o["u"]), sl(o["delta"]), o["A"], sl(o["B"]), sl(o["C"]), o["D"], sl(o["z"]), o["bias"], o["sp"], o["act"],
                                    state_in=st, state_out=st, segments=segments, lib=lib)
    return out, st


def check_scan(dt, kind, dim, lib, device, lens, range_len=0, bitwise=True, state_oracle=None, seed=0):
    """per session: out and the exit state bit-equal to scan_tm_fwd_state on the session alone (bitwise=True: uncut, or a cut whose ranges
    coincide), out within OUT_BAR of the oracle; in place; foreign and empty rows untouched.  state_oracle: {session: fp64 state}"""
    p = scan_pack(dt, kind, dim, device, lens, seed)
    s, rows = p["s"], p["rows"]
    pool = _pool(rows, s["entry"], p["nrows"], device)
    keep = pool.clone()
    out = run_var(p, lib, pool, range_len)
    assert out.dtype == DT[dt] and out.shape == p["ops"]["u"].shape and out.is_contiguous()
    o = 0
    for i, (L, r) in enumerate(zip(lens, rows)):
        if L == 0:
            assert torch.equal(pool[r], keep[r]), "the empty session's state was touched"
            continue
        got = out[o:o + L].unsqueeze(0)
        ref = s["ref_out"][i:i + 1, :L]
        e_out, r_out = rel_err(_np(got), ref), rms_err(_np(got), ref)
        msg = f"scan_tm_fwd_state_var {dt} dim {dim} range {range_len} session {i} len {L}: out {e_out:.3e} rms {r_out:.3e} (bar {OUT_BAR[dt]:.0e})"
        if bitwise:
            seg = 1 if range_len == 0 else -(-L // range_len)
            o_solo, st_solo = _solo(p, i, L, lib, seg)
            assert torch.equal(got, o_solo), f"session {i} (len {L}): out differs from scan_tm_fwd_state(segments={seg}) on the session alone"
            assert torch.equal(pool[r:r + 1], st_solo), f"session {i} (len {L}): the state differs from scan_tm_fwd_state(segments={seg})'s"
        if L == max(lens) or state_oracle is not None:
            ref_st = s["ref_state"][i] if L == max(lens) else state_oracle.get(i)
            if ref_st is not None:
                e_st = rel_err(_np(pool[r]), ref_st)
                msg += f", state {e_st:.3e} (bar {STATE_BAR:.1e})"
                assert e_st < STATE_BAR, msg
        print(msg)
        assert e_out < OUT_BAR[dt] and r_out < OUT_BAR[dt], msg
        o += L
    _foreign_untouched(pool, rows, "scan")
    return p, out, pool


def session_state_oracle(dt, kind, dim, device, lens, seed=0):
    """fp64 exit states of the sessions shorter than the longest: the setup rebuilt (same seed: same operands) and the oracle run on each
    session's own rows.  scan_setup draws every operand for max(lens) + prefix rows; a setup of another T draws other numbers, so the
    oracle is run here on slices of the same draw."""
    T, t0 = max(lens), kind[5]
    n = len(lens)
    rng = np.random.default_rng(100 + 80 + seed)
    Lall, N = t0 + T, 16
    form, has_z, has_D, has_bias = kind[0], kind[1], kind[2], kind[3]
    u_t, u = sc._round(rng.standard_normal((n, Lall, dim)), dt)
    z_t, z = sc._round(rng.standard_normal((n, Lall, dim)), dt)
    B_t, Bm = sc._round(rng.standard_normal((n, Lall, N)), dt)
    C_t, Cm = sc._round(rng.standard_normal((n, Lall, N)), dt)
    A = -np.exp(rng.standard_normal((dim, N)) * 0.5).astype(np.float32)
    D = rng.standard_normal(dim).astype(np.float32) if has_D else None
    bias = (rng.standard_normal(dim) * 0.5).astype(np.float32) if has_bias else None
    if form == "raw" and bias is not None:
        bias = np.abs(bias)
    raw = rng.standard_normal((n, Lall, dim)) * 0.7 - (0.5 if form != "raw" else 0.0)
    if form == "raw":
        raw = np.abs(raw) * 0.3
    if form == "act":
        d_t, d = sc._round(sc._softplus64(raw + (bias[None, None, :] if bias is not None else 0.0)), dt)
        o_bias, o_sp = None, False
    else:
        d_t, d = sc._round(raw, dt)
        o_bias, o_sp = bias, form == "sp"
    tr = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    out = {}
    for i, L in enumerate(lens):
        if 0 < L < T:
            e = t0 + L
            out[i] = oracle.scan_fwd(tr(u[i:i + 1, :e]), tr(d[i:i + 1, :e]), A, tr(Bm[i:i + 1, :e]), tr(Cm[i:i + 1, :e]), D,
                                     tr(z[i:i + 1, :e]) if has_z else None, o_bias, o_sp, prec="f64")["last_state"][0]
    return out


# ---- packing invariance ----------------------------------------------------------------------------
def check_packing_invariance(dt, kind, dim, lib, device, range_len=0):
    """a session's out, state and window do not change by a bit when the other sessions of the call, its place in the pack and its pool
    row change, nor when the neighbours' rows of every operand are NaN (the staging never reads a neighbour's row into a result)"""
    lens = (9, 40, 3, 17)
    p = scan_pack(dt, kind, dim, device, lens, seed=3)
    s = p["s"]
    pool = _pool(p["rows"], s["entry"], p["nrows"], device)
    out = run_var(p, lib, pool, range_len)
    cu = np.cumsum((0,) + lens)
    for i, L in enumerate(lens):
        # (a) session i alone, at another pool row
        ops1 = {k: (None if v is None else v[cu[i]:cu[i + 1]]) for k, v in p["ops"].items()}
        pool1 = _pool((2,), s["entry"][i:i + 1], NROWS, device)
        out1 = run_var(p, lib, pool1, range_len, ops=ops1, lens=(L,), rows=(2,))
        assert torch.equal(out1, out[cu[i]:cu[i + 1]]), f"session {i}: out depends on the other sessions / its place / its row"
        assert torch.equal(pool1[2], pool[p["rows"][i]]), f"session {i}: state depends on the other sessions / its place / its row"
        # (b) the whole pack again with every OTHER session's rows poisoned
        ops2 = {}
        for k, v in p["ops"].items():
            if v is None:
                ops2[k] = None
                continue
            w = v.clone()
            w[:cu[i]] = float("nan")
            w[cu[i + 1]:] = float("nan")
            ops2[k] = w
        pool2 = _pool(p["rows"], s["entry"], p["nrows"], device)
        out2 = run_var(p, lib, pool2, range_len, ops=ops2)
        assert torch.equal(out2[cu[i]:cu[i + 1]], out[cu[i]:cu[i + 1]]), f"session {i}: out changes when the neighbours' rows are NaN"
        assert torch.equal(pool2[p["rows"][i]], pool[p["rows"][i]]), f"session {i}: state changes when the neighbours' rows are NaN"


def check_conv_packing_invariance(dt, dim, lib, device):
    kind = sc.CONV_KINDS[0]
    lens = (3, 70, 1, 9)
    p = conv_pack(dt, kind, dim, device, lens=lens, seed=5)
    s = p["s"]
    pool = _pool(p["rows"], p["entry"], p["nrows"], device)
    m = aum_hip.seq_map(lens, p["rows"], device=device)
    y = aum_hip.conv1d_tm_prefill_var(p["x"], pool, s["w"], s["bias"], s["silu"], seq_map=m, lib=lib)
    cu = np.cumsum((0,) + lens)
    for i, L in enumerate(lens):
        x2 = p["x"].clone()
        x2[:cu[i]] = float("nan")
        x2[cu[i + 1]:] = float("nan")
        pool2 = _pool(p["rows"], p["entry"], p["nrows"], device)
        y2 = aum_hip.conv1d_tm_prefill_var(x2, pool2, s["w"], s["bias"], s["silu"], seq_map=m, lib=lib)
        assert torch.equal(y2[cu[i]:cu[i + 1]], y[cu[i]:cu[i + 1]]), f"session {i}: y changes when the neighbours' rows are NaN"
        assert torch.equal(pool2[p["rows"][i]], pool[p["rows"][i]]), f"session {i}: the window changes when the neighbours' rows are NaN"
        pool1 = _pool((5,), p["entry"][i:i + 1], NROWS, device)
        m1 = aum_hip.seq_map((L,), (5,), device=device)
        y1 = aum_hip.conv1d_tm_prefill_var(p["x"][cu[i]:cu[i + 1]], pool1, s["w"], s["bias"], s["silu"], seq_map=m1, lib=lib)
        assert torch.equal(y1, y[cu[i]:cu[i + 1]]) and torch.equal(pool1[5], pool[p["rows"][i]]), f"session {i}: depends on the pack"


# ---- refusals --------------------------------------------------------------------------------------
def check_refusals(lib, device):
    import pytest
    lens = (9, 5)
    p = scan_pack("bf16", pc.KINDS[0], 64, device, lens)
    s = p["s"]
    pool = _pool(p["rows"], s["entry"], NROWS, device)
    keep = pool.clone()
    o, k = s["ops"], p["ops"]
    m = aum_hip.seq_map(lens, p["rows"], device=device)
    call = lambda st=pool, mm=m, rl=0, act=False, **kw: aum_hip.scan_tm_fwd_state_var(
        st, kw.get("u", k["u"]), kw.get("delta", k["delta"]), o["A"], k["B"], k["C"], o["D"], kw.get("z", k["z"]), o["bias"], o["sp"] and not act, act,
        seq_map=mm, range_len=rl, lib=lib)
    call()                                                                      # the operands as they are: taken
    pool.copy_(keep)
    pad = torch.zeros(NROWS * 64 * 16 + 1, device=device)[1:].view(NROWS, 64, 16)                  # 4-byte aligned only
    for bad in (dict(st=pool.double()), dict(st=pad), dict(rl=12), dict(rl=-8), dict(delta=k["delta"].float())):
        with pytest.raises(RuntimeError, match="scan_tm_fwd_state_var"):
            call(**bad)
    long = aum_hip.seq_map((9 + 5,), (0,), device=device)                       # 14 steps in ranges of 8: fine; 33 ranges: refused
    call(mm=long, rl=8)
    p2 = scan_pack("bf16", pc.KINDS[0], 64, device, (8 * 33,))
    pool2 = _pool((0,), p2["s"]["entry"], NROWS, device)
    with pytest.raises(RuntimeError, match="scan_tm_fwd_state_var"):
        run_var(p2, lib, pool2, range_len=8)
    run_var(p2, lib, pool2, range_len=16)
    pool.copy_(keep)
    with pytest.raises(ValueError):                                             # a map of another total
        call(mm=aum_hip.seq_map((9, 4), p["rows"], device=device))
    with pytest.raises(ValueError):                                             # a row outside the pool
        call(mm=aum_hip.seq_map(lens, (1, NROWS), device=device))
    with pytest.raises(TypeError):
        call(mm=None)
    if device != "cpu":                                                         # a map on another device
        with pytest.raises(RuntimeError):
            call(mm=aum_hip.seq_map(lens, p["rows"], device="cpu"))
    # an activated delta with fp32 rows
    pf = scan_pack("f32", pc.KINDS[0], 64, device, lens)
    kf, of = pf["ops"], pf["s"]["ops"]
    with pytest.raises(RuntimeError, match="scan_tm_fwd_state_var"):
        aum_hip.scan_tm_fwd_state_var(pool, kf["u"], kf["delta"], of["A"], kf["B"], kf["C"], of["D"], kf["z"], None, False, True, seq_map=m, lib=lib)
    assert torch.equal(pool, keep), "a refused call wrote to the pool"
    # conv
    c = conv_pack("bf16", sc.CONV_KINDS[0], 64, device, lens=lens)
    cs = c["s"]
    cpool = _pool(c["rows"], c["entry"], NROWS, device)
    ckeep = cpool.clone()
    ccall = lambda x=c["x"], st=cpool, mm=m: aum_hip.conv1d_tm_prefill_var(x, st, cs["w"], cs["bias"], True, seq_map=mm, lib=lib)
    ccall()
    cpool.copy_(ckeep)
    odd = torch.zeros(sum(lens) * 64 + 1, dtype=DT["bf16"], device=device)[1:].view(sum(lens), 64)      # 2-byte aligned rows
    for bad in (dict(st=cpool.double()), dict(x=c["x"].double()), dict(x=odd), dict(st=cpool.transpose(1, 2).contiguous().transpose(1, 2))):
        with pytest.raises(RuntimeError, match="conv1d_tm_prefill_var"):
            ccall(**bad)
    with pytest.raises(ValueError):
        ccall(mm=aum_hip.seq_map((9, 4), c["rows"], device=device))
    with pytest.raises(ValueError):
        ccall(mm=aum_hip.seq_map(lens, (1, NROWS), device=device))
    assert torch.equal(cpool, ckeep), "a refused call wrote to the pool"
    # the C entry points: what the binding cannot send
    a = aum_hip.ScanTmFwdStateVarArgs()
    outt = torch.empty_like(k["u"].contiguous())
    u, d, z, bc = k["u"].contiguous(), k["delta"].contiguous(), k["z"].contiguous(), torch.cat((k["B"], k["C"]), dim=1).contiguous()
    a.u, a.delta, a.z, a.B, a.C, a.A, a.out, a.state = u.data_ptr(), d.data_ptr(), z.data_ptr(), bc.data_ptr(), bc.data_ptr() + 32, o["A"].data_ptr(), outt.data_ptr(), pool.data_ptr()
    a.cu_seqlens, a.state_indices = m.cu.data_ptr(), m.idx.data_ptr()
    a.u_ts = a.delta_ts = a.z_ts = a.out_ts = 64
    a.B_ts = a.C_ts = 32
    a.total, a.nseq, a.nrows, a.dim, a.dstate, a.dtype, a.max_len = sum(lens), 2, NROWS, 64, 16, aum_hip.AUM_BF16, 9
    go = lambda: lib.c.aum_scan_tm_fwd_state_var(aum_hip.C_byref(a), lib.stream(u))
    assert go() == 0
    a.range_len = 4
    assert go() == -4
    a.range_len = 8                             # ranges without scratch
    assert go() == -1
    a.range_len, a.max_len = 0, sum(lens) + 1   # a longest session the pack cannot hold
    assert go() == -4
    a.max_len, a.flags = 9, aum_hip.SCAN_REVERSE
    assert go() == -4
    assert lib.c.aum_scan_tm_fwd_state_var_carry_bytes(2, 64, 16, 33) == 0 and lib.c.aum_scan_tm_fwd_state_var_carry_bytes(2, 64, 16, 5) == 2 * 5 * 2 * 16 * 64 * 4
    if device != "cpu":
        torch.cuda.synchronize()


# ---- block -----------------------------------------------------------------------------------------
def check_block(d_model, dt_rank, dt, lib, device, lens=(9, 3, 70)):
    """prefill_chunk(seq_map=) on three ragged sessions over pools against prefill_chunk per session (rel_err within OUT_BAR[dt]: the GEMMs
    see another M); step_chunk(seq_map=) continues from the caches it leaves; the two new launches ran once each, conv1d_tm_fwd and
    scan_tm_fwd_state did not"""
    m = pc.make_mamba(d_model, dt_rank, dt, device)
    torch.manual_seed(21)
    n, prefix, more = len(lens), 5, 4
    xs = [torch.randn(1, prefix + L + more, d_model, device=device).to(DT[dt]) for L in lens]
    rows = ROWS[:n]
    with torch.no_grad(), pc.product_lib(lib):
        cp, sp = (t.float() for t in m.allocate_inference_cache(NROWS, 0))
        cp.fill_(SENT), sp.fill_(SENT)
        solo = []
        for x, r in zip(xs, rows):           # non-zero caches: a prefix through step_chunk
            c0, s0 = (t.float() for t in m.allocate_inference_cache(1, 0))
            m.step_chunk(x[:, :prefix], c0, s0)
            cp[r], sp[r] = c0[0], s0[0]
            solo.append((c0, s0))
        smap = aum_hip.seq_map(lens, rows, device=device)
        packed = torch.cat([x[:, prefix:prefix + L] for x, L in zip(xs, lens)], dim=1)
        with pc.counting(aum_hip, "_conv1d_tm_prefill_var") as n_conv, pc.counting(aum_hip, "_scan_tm_fwd_state_var") as n_scan, \
                pc.counting(aum_hip, "conv1d_tm_fwd") as n_oldc, pc.counting(aum_hip, "scan_tm_fwd_state") as n_olds, \
                pc.counting(m, "step_chunk") as n_live, pc.counting(aum_hip, "xdt_tm_fwd") as n_xdt:
            out, _, _ = m.prefill_chunk(packed, cp, sp, seq_map=smap)
        assert (n_conv[0], n_scan[0], n_oldc[0], n_olds[0], n_live[0]) == (1, 1, 0, 0, 0), \
            f"packed prefill_chunk: {n_conv[0]} conv1d_tm_prefill_var, {n_scan[0]} scan_tm_fwd_state_var, {n_oldc[0]} conv1d_tm_fwd, {n_olds[0]} scan_tm_fwd_state, {n_live[0]} step_chunk"
        assert n_xdt[0] == int(device != "cpu" and d_model == 128 and dt != "f32"), f"{n_xdt[0]} aum_xdt_tm_fwd calls"
        assert out.shape == (1, sum(lens), d_model) and out.dtype == DT[dt]
        o = 0
        for x, L, r, (c0, s0) in zip(xs, lens, rows, solo):
            ref, _, _ = m.prefill_chunk(x[:, prefix:prefix + L], c0, s0)
            e_out, e_st = rel_err(_np(out[:, o:o + L]), _np(ref)), rel_err(_np(sp[r]), _np(s0[0]))
            print(f"Mamba({d_model}, dt_rank={dt_rank}) {dt} packed session len {L}: out vs solo prefill_chunk {e_out:.3e}, state {e_st:.3e} (bar {OUT_BAR[dt]:.0e})")
            assert e_out < OUT_BAR[dt] and e_st < OUT_BAR[dt]
            assert rel_err(_np(cp[r]), _np(c0[0])) < OUT_BAR[dt], "a conv window differs from the solo prefill's"      # in_proj rows of another M
            o += L
        _foreign_untouched(cp, rows, "block conv pool")
        _foreign_untouched(sp, rows, "block state pool")
        # live from there: step_chunk(seq_map=) on the pools against step_chunk on the solo caches
        smap2 = aum_hip.seq_map((more,) * n, rows, device=device)
        nxt = torch.cat([x[:, prefix + L:] for x, L in zip(xs, lens)], dim=1)
        o2, _, _ = m.step_chunk(nxt, cp, sp, seq_map=smap2)
        for i, (x, L, (c0, s0)) in enumerate(zip(xs, lens, solo)):
            ref, _, _ = m.step_chunk(x[:, prefix + L:], c0, s0)
            e = rel_err(_np(o2[:, i * more:(i + 1) * more]), _np(ref))
            assert e < OUT_BAR[dt], f"step_chunk behind the packed prefill, session {i}: {e:.3e}"


# ---- model -----------------------------------------------------------------------------------------
def check_model(lib, device):
    """stream_prefill_many(packed=True) on rows [4, 1, 3] of a pool of 6, columns [10, 3, 16]: stream_read against a solo stream_prefill +
    stream_read and, for the full clip, against model(spec) -- the 2e-2 bar of check_model_prefill; counts, sentinels, one packed pass"""
    model = sc.make_causal_aum(128, device, depth=2)
    torch.manual_seed(13)
    spec = torch.randn(3, 256, 128, device=device)
    rows, ks = [4, 1, 3], [10, 3, 16]
    bar = 2e-2
    with torch.no_grad(), pc._autocast(device), pc.product_lib(lib):
        pool = model.allocate_stream_pool(6)
        for c, s in pool["layers"].values():
            c.fill_(SENT)
            s.fill_(-3.0)
        model.stream_reset(pool, rows)
        with pc.counting(aum_hip, "_conv1d_tm_prefill_var") as n_conv, pc.counting(aum_hip, "_scan_tm_fwd_state_var") as n_scan, \
                pc.counting(aum_hip, "scan_tm_fwd_state") as n_old:
            assert model.stream_prefill_many([spec[i, :16 * k] for i, k in enumerate(ks)], pool, rows, packed=True) == ks
        assert n_conv[0] == n_scan[0] == len(model.layers) and n_old[0] == 0, \
            f"{n_conv[0]} / {n_scan[0]} packed launches for {len(model.layers)} blocks, {n_old[0]} scan_tm_fwd_state calls"
        assert pool["columns"] == [0, 3, 0, 16, 10, 0]
        got = model.stream_read(pool, return_features=True, sessions=rows)
        for i, (r, k) in enumerate(zip(rows, ks)):
            solo = model.allocate_inference_cache(1)
            model.stream_prefill(spec[i:i + 1, :16 * k], solo)
            ref = model.stream_read(solo, return_features=True)
            e = rel_err(_np(got[i:i + 1]), _np(ref))
            print(f"packed prefill, session {r} ({k} columns): stream_read vs a solo stream_prefill {e:.3e} (bar {bar:.0e})")
            assert e < bar
            for (c, s), (cs, ss) in zip(pool["layers"].values(), solo["layers"].values()):
                assert rel_err(_np(s[r]), _np(ss[0])) < bar
        full = model(spec[2:3], return_features=True)
        e_full = rel_err(_np(got[2:3]), _np(full))
        print(f"packed prefill, the full clip: stream_read vs model(spec) {e_full:.3e} (bar {bar:.0e})")
        assert e_full < bar
        for c, s in pool["layers"].values():
            for r in (0, 2, 5):
                assert bool((c[r] == SENT).all()) and bool((s[r] == -3.0).all()), f"row {r} was touched"
        assert model.stream_push_many([spec[1, 48:64]], pool, [1]) == [4]        # the sessions go on live from there
        live = model.allocate_inference_cache(1)
        model.stream_prefill(spec[1:2, :64], live)
        e_live = rel_err(_np(model.stream_read(pool, return_features=True, sessions=[1])), _np(model.stream_read(live, return_features=True)))
        assert e_live < bar, f"a push behind the packed prefill: {e_live:.3e}"


def check_model_refusals(lib, device):
    """the refusal cases of stream_prefill_checks.check_model_refusals with packed=True: pool and counts unchanged"""
    import pytest
    model = sc.make_causal_aum(128, device, depth=2)
    spec = torch.randn(2, 256, 128, device=device)

    def snapshot(c):
        return [t.clone() for pair in c["layers"].values() for t in pair], list(c["columns"])

    def same(c, snap):
        return all(torch.equal(a, b) for a, b in zip(snapshot(c)[0], snap[0])) and snapshot(c)[1] == snap[1]

    with torch.no_grad(), pc._autocast(device), pc.product_lib(lib):
        pool = model.allocate_stream_pool(3)
        model.stream_prefill_many([spec[0, :224]], pool, [2], packed=True)
        assert pool["columns"] == [0, 0, 14]
        psnap = snapshot(pool)
        for specs, rows in (([spec[0, :16], spec[1, :48]], [0, 2]), ([spec[0, :16]], [3]), ([spec[0, :16], spec[1, :16]], [1, 1]),
                            ([spec[0, :24]], [0]), ([spec[0, :16]], [0, 1])):
            with pytest.raises(ValueError):
                model.stream_prefill_many(specs, pool, rows, packed=True)
            assert same(pool, psnap)
        cache = model.allocate_inference_cache(2)
        with pytest.raises(ValueError):
            model.stream_prefill_many([spec[0, :16]], cache, [0], packed=True)
