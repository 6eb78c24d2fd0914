"""Checks of PEEK ROWS EVERY P ROWS of streaming inference (aum_conv1d_tm_chunk_peeks / aum_scan_tm_chunk_peeks, aum_hip.conv1d_tm_chunk_peeks
/ scan_tm_chunk_peeks, conv1d_stream / scan_stream(peek_every=), Mamba.step_chunk(peek_every=), AudioMamba.stream_timeline /
stream_timeline_many), shared by tests/test_stream_timeline.py (CPU, lane-array library) and tests/test_gpu_stream_timeline.py (device
library).

The defining property is BIT EQUALITY with calls the library had before: per session, the rows cut into groups of P + 1, aum_*_tm_chunk_var
with the PEEK_LAST flag on one full group after the other and once more, without the flag, on the trailing partial group (chain()).  y and
the cache pool are compared with torch.equal; pool rows no session names stay at the sentinel.
The arithmetic is held to an fp64 recurrence written here (committed rows update, peek rows do not) under the bars of stream_checks
(OUT_BAR per dtype, CACHE_BAR).  Module and model: the bars of stream_checks.check_model_stream / stream_peek_checks (1e-4 without
autocast, 2e-2 under it) -- the GEMMs see another row count than in the per-column form."""
import contextlib

import numpy as np
import pytest
import torch

import aum_hip
import stream_block_checks as bc
from conftest import rel_err
from stream_checks import CACHE_BAR, DT, OUT_BAR, make_causal_aum

SENTINEL = 7.25
PERIODS = (1, 3, 7, 8, 15)      # STREAM_UB = 8: the peek row at every position of a fetch block (8 walks through all phases), always on a
                                # block's last row (7), always on the double block's last row (15)
DIMS = (128, 384)


def pack_lengths(P):
    return (0, 1, P, P + 1, P + 2, 2 * (P + 1), 8 * (P + 1) + 3)


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _np(t):
    return t.detach().float().cpu().numpy()


def _is_peek(j, P):
    return (j + 1) % (P + 1) == 0


# ---- the two operators behind one interface: operands of `total` packed rows and a pool of `nrows` cache rows -------------------------------
class ConvOp:
    name = "conv"
    KINDS = ((True, True), (False, False), (True, False))        # (silu, bias), rotating over the cases

    @staticmethod
    def operands(dt, dim, total, nrows, live, device, kind=0, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        silu, has_bias = ConvOp.KINDS[kind % len(ConvOp.KINDS)]
        xz = torch.randn(max(total, 1), 2 * dim, generator=g).to(DT[dt]).to(device)[:total]      # x as the first half of xz rows
        pool = torch.full((nrows, dim, 4), SENTINEL)
        for r in live:
            pool[r] = torch.randn(dim, 4, generator=g)
        return {"dt": dt, "dim": dim, "x": xz[:, :dim], "w": (torch.randn(dim, 4, generator=g) * 0.5).to(device),
                "b": torch.randn(dim, generator=g).to(device) if has_bias else None, "silu": silu, "pool": pool.to(device)}

    @staticmethod
    def var(o, idx, pool, smap, lib, peek):
        x = o["x"] if idx is None else o["x"].index_select(0, idx)
        return aum_hip.conv1d_tm_chunk_var(x, pool, o["w"], o["b"], o["silu"], seq_map=smap, lib=lib, peek=peek)

    @staticmethod
    def peeks(o, pool, smap, lib, P, out=None):
        return aum_hip.conv1d_tm_chunk_peeks(o["x"], pool, o["w"], o["b"], o["silu"], seq_map=smap, out=out, lib=lib, peek_every=P)

    @staticmethod
    def raw(o, pool, smap, y, lib):
        """the C struct of a call on all rows, and what must stay alive until the call returns"""
        pa = aum_hip.ConvTmChunkPeeksArgs()
        a = pa.base
        _, held = aum_hip._conv_chunk_operands(a, "test", lib, o["x"], pool, o["w"], o["b"], o["silu"], y)
        aum_hip._fill_map(a, smap, pool.shape[0])
        return pa, lib.c.aum_conv1d_tm_chunk_peeks, aum_hip.CONV_PEEK_LAST, held

    @staticmethod
    def fp64(o, lens, rows, P):
        """y (total, dim) and the pool in fp64: committed rows move the window, peek rows do not"""
        x, w = _np(o["x"]).astype(np.float64), _np(o["w"]).astype(np.float64)
        b = np.zeros(o["dim"]) if o["b"] is None else _np(o["b"]).astype(np.float64)
        pool = _np(o["pool"]).astype(np.float64)
        y, at = np.zeros_like(x), 0
        for n, r in zip(lens, rows):
            win = pool[r].copy()                                  # (dim, 4): the last four committed inputs
            for j in range(n):
                full = np.concatenate((win[:, 1:], x[at + j][:, None]), axis=1)
                acc = b + (full * w).sum(axis=1)
                y[at + j] = acc / (1.0 + np.exp(-acc)) if o["silu"] else acc
                if not _is_peek(j, P):
                    win = full
            pool[r] = win
            at += n
        return y, pool


class ScanOp:
    name = "scan"
    KINDS = (("sp", True, True), ("act", True, True), ("raw", False, False), ("sp", False, True))      # (delta form, z, D)

    @staticmethod
    def operands(dt, dim, total, nrows, live, device, kind=0, seed=0):
        g = torch.Generator().manual_seed(2000 + seed)
        form, has_z, has_D = ScanOp.KINDS[kind % len(ScanOp.KINDS)]
        n = max(total, 1)
        xz = torch.randn(n, 2 * dim, generator=g).to(DT[dt]).to(device)[:total]          # u, z as the halves of one xz row
        bcm = torch.randn(n, 32, generator=g).to(DT[dt]).to(device)[:total]              # B, C as column blocks of one row
        raw = torch.randn(n, dim, generator=g) * 0.7 - 0.5
        bias = torch.randn(dim, generator=g) * 0.5
        if form == "act":
            delta, o_bias = torch.nn.functional.softplus(raw.double() + bias.double()).float(), None
        elif form == "raw":
            delta, o_bias = raw.abs() * 0.3, bias.abs()
        else:
            delta, o_bias = raw, bias
        pool = torch.full((nrows, dim, 16), SENTINEL)
        for r in live:
            pool[r] = torch.randn(dim, 16, generator=g) * 0.3
        return {"dt": dt, "dim": dim, "u": xz[:, :dim], "z": xz[:, dim:] if has_z else None, "delta": delta.to(DT[dt]).to(device)[:total],
                "B": bcm[:, :16], "C": bcm[:, 16:], "A": (-torch.exp(torch.randn(dim, 16, generator=g) * 0.5)).to(device),
                "D": torch.randn(dim, generator=g).to(device) if has_D else None, "bias": None if o_bias is None else o_bias.to(device),
                "sp": form == "sp", "act": form == "act", "pool": pool.to(device)}

    @staticmethod
    def var(o, idx, pool, smap, lib, peek):
        t = (lambda a: a) if idx is None else (lambda a: None if a is None else a.index_select(0, idx))
        return aum_hip.scan_tm_chunk_var(pool, t(o["u"]), t(o["delta"]), o["A"], t(o["B"]), t(o["C"]), o["D"], t(o["z"]), o["bias"], o["sp"],
                                         o["act"], seq_map=smap, lib=lib, peek=peek)

    @staticmethod
    def peeks(o, pool, smap, lib, P, out=None):
        return aum_hip.scan_tm_chunk_peeks(pool, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"], o["act"],
                                           seq_map=smap, out=out, lib=lib, peek_every=P)

    @staticmethod
    def raw(o, pool, smap, y, lib):
        pa = aum_hip.ScanTmChunkPeeksArgs()
        a = pa.base
        _, held = aum_hip._scan_chunk_operands(a, "test", lib, pool, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"],
                                               o["sp"], o["act"], y)
        aum_hip._fill_map(a, smap, pool.shape[0])
        return pa, lib.c.aum_scan_tm_chunk_peeks, aum_hip.SCAN_PEEK_LAST, held

    @staticmethod
    def fp64(o, lens, rows, P):
        """y (total, dim) and the pool in fp64: committed rows update the state, peek rows step from it and leave it"""
        f = lambda t: _np(t).astype(np.float64)
        u, dl, Bm, Cm, A = f(o["u"]), f(o["delta"]), f(o["B"]), f(o["C"]), f(o["A"])
        if o["bias"] is not None:
            dl = dl + f(o["bias"])[None, :]
        if o["sp"]:
            dl = np.where(dl > 20, dl, np.log1p(np.exp(np.minimum(dl, 20))))
        pool = f(o["pool"])
        y, at = np.zeros_like(u), 0
        for n, r in zip(lens, rows):
            h = pool[r].copy()                                    # (dim, 16)
            for j in range(n):
                t = at + j
                hn = np.exp(dl[t][:, None] * A) * h + (dl[t] * u[t])[:, None] * Bm[t][None, :]
                v = hn @ Cm[t]
                if o["D"] is not None:
                    v = v + f(o["D"]) * u[t]
                if o["z"] is not None:
                    z = f(o["z"])[t]
                    v = v * z / (1.0 + np.exp(-z))
                y[t] = v
                if not _is_peek(j, P):
                    h = hn
            pool[r] = h
            at += n
        return y, pool


OPS = {"conv": ConvOp, "scan": ScanOp}


def chain(op, o, lens, rows, P, lib, device):
    """The defining procedure with the entry points the library had before, all sessions in lockstep: call g takes group g (P + 1 rows) of
    every session that has a full one with the PEEK_LAST flag, and the sessions whose group g is the trailing partial one without it.
    -> (y (total, dim), the pool)"""
    pool = o["pool"].clone()
    total = sum(lens)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    y = torch.zeros(total, o["dim"], dtype=DT[o["dt"]], device=device)
    for g in range(max(-(-n // (P + 1)) for n in lens) if total else 0):
        for flagged in (True, False):
            sel, idx = [], []
            for n, at in zip(lens, starts):
                a, b = g * (P + 1), min((g + 1) * (P + 1), n)
                take = b > a and (b - a == P + 1) == flagged
                sel.append(b - a if take else 0)
                if take:
                    idx += list(range(at + a, at + b))
            if idx:
                ix = torch.tensor(idx, dtype=torch.int64, device=device)
                y[ix] = op.var(o, ix, pool, aum_hip.seq_map(sel, rows, device=device), lib, flagged)
    return y, pool


def _layouts(P, nseq):
    """(lengths in pack order, cache rows or None, pool rows): a shuffled pack on shuffled rows of a pool with spare rows, and the same
    lengths with state_indices = NULL"""
    rng = np.random.default_rng(17 + P)
    lens = [pack_lengths(P)[i] for i in rng.permutation(nseq)]
    return ((lens, [int(r) for r in rng.permutation(nseq + 2)[:nseq]], nseq + 2), (lens, None, nseq + 2))


def check_peeks_equal_chain(opname, dt, dim, P, lib, device, kind=0):
    op = OPS[opname]
    for lens, rows, nrows in _layouts(P, len(pack_lengths(P))):
        live = list(range(len(lens))) if rows is None else rows
        o = op.operands(dt, dim, sum(lens), nrows, live, device, kind=kind, seed=P)
        smap = aum_hip.seq_map(lens, rows, device=device)
        y_ref, pool_ref = chain(op, o, lens, live, P, lib, device)
        pool = o["pool"].clone()
        y = op.peeks(o, pool, smap, lib, P)
        _sync(device)
        assert y.dtype == DT[dt] and y.shape == (sum(lens), dim)
        assert torch.equal(y, y_ref), f"{opname} {dt} dim {dim} P {P}: outputs differ from the chain of PEEK_LAST calls"
        assert torch.equal(pool, pool_ref), f"{opname} {dt} dim {dim} P {P}: the cache pool differs from the chain of PEEK_LAST calls"
        for r in set(range(nrows)) - set(live):
            assert torch.equal(pool[r], torch.full_like(pool[r], SENTINEL)), f"{opname}: spare cache row {r} was written"
        for n, r in zip(lens, live):
            if n == 0:
                assert torch.equal(pool[r], o["pool"][r])
            else:
                assert not torch.equal(pool[r], o["pool"][r])


def check_no_peek_row_is_plain_var(opname, dt, dim, P, lib, device):
    """sessions shorter than P + 1 have no peek row: the call is the plain *_chunk_var call, bit for bit"""
    op = OPS[opname]
    lens, rows = (P, 0, 1, max(P - 1, 1)), (2, 0, 3, 1)
    o = op.operands(dt, dim, sum(lens), 5, rows, device, kind=1, seed=40 + P)
    smap = aum_hip.seq_map(lens, rows, device=device)
    pool_a, pool_b = o["pool"].clone(), o["pool"].clone()
    y_a, y_b = op.peeks(o, pool_a, smap, lib, P), op.var(o, None, pool_b, smap, lib, False)
    _sync(device)
    assert torch.equal(y_a, y_b) and torch.equal(pool_a, pool_b)
    assert torch.equal(pool_a[4], torch.full_like(pool_a[4], SENTINEL))


def check_vs_fp64(opname, dt, lib, device, dim=128, P=3):
    op = OPS[opname]
    lens, rows = (11, 4, 3, 18), (2, 0, 3, 1)
    o = op.operands(dt, dim, sum(lens), 5, rows, device, kind=0, seed=77)
    pool = o["pool"].clone()
    y = op.peeks(o, pool, aum_hip.seq_map(lens, rows, device=device), lib, P)
    _sync(device)
    y_ref, pool_ref = op.fp64(o, lens, rows, P)
    live = list(rows)
    e_out, e_pool = rel_err(_np(y), y_ref), rel_err(_np(pool[live]), pool_ref[live])
    print(f"{opname} peeks {dt} vs fp64 recurrence: out {e_out:.3e} (bar {OUT_BAR[dt]:.0e}), cache {e_pool:.3e} (bar {CACHE_BAR:.0e})")
    assert e_out < OUT_BAR[dt]
    assert e_pool < CACHE_BAR
    # the peek rows did not advance anything: dropping them from the input gives the same caches through the plain call
    keep = [at + j for at, n in zip(np.cumsum((0,) + lens[:-1]), lens) for j in range(n) if not _is_peek(j, P)]
    ix = torch.tensor(keep, dtype=torch.int64, device=device)
    pool2 = o["pool"].clone()
    y2 = op.var(o, ix, pool2, aum_hip.seq_map([n - n // (P + 1) for n in lens], rows, device=device), lib, False)
    _sync(device)
    assert torch.equal(pool2, pool) and torch.equal(y2, y.index_select(0, ix))


def check_refusals(opname, lib, device):
    """peek_every = 0 and a PEEK_LAST bit in base.flags: a non-zero code each, every buffer untouched; the same struct is taken without them"""
    op = OPS[opname]
    lens, rows = (5, 3), (1, 0)
    o = op.operands("bf16", 128, sum(lens), 2, rows, device, kind=0, seed=5)
    smap = aum_hip.seq_map(lens, rows, device=device)
    pool = o["pool"].clone()
    y = torch.full((sum(lens), 128), 3.0, dtype=DT["bf16"], device=device)
    pa, fn, peek_last, held = op.raw(o, pool, smap, y, lib)
    call = lambda: fn(aum_hip.C_byref(pa), lib.stream(y))
    flags = pa.base.flags
    for pe, fl in ((0, flags), (-1, flags), (2, flags | peek_last)):
        pa.peek_every, pa.base.flags = pe, fl
        assert call() != 0, (pe, fl)
        _sync(device)
        assert torch.equal(pool, o["pool"]) and bool((y == 3.0).all())
    pa.peek_every, pa.base.flags = 2, flags
    assert call() == 0
    _sync(device)
    y_ref, pool_ref = chain(op, o, lens, rows, 2, lib, device)
    assert torch.equal(y, y_ref) and torch.equal(pool, pool_ref)
    with pytest.raises(ValueError, match="peek_every"):
        op.peeks(o, pool, smap, lib, 0)
    with pytest.raises(ValueError, match="peek_every"):
        op.peeks(o, pool, smap, lib, None)


def check_host_loop(lib):
    """shapes the packed kernels refuse (a scan of 96 channels, a conv window of 5): the ladder loops over the groups on the host through
    the existing peek path -- against the same calls written out"""
    torch.manual_seed(23)
    P, lens, rows = 2, (7, 2, 0, 3), (2, 0, 1, 3)
    total, smap = sum(lens), aum_hip.seq_map(lens, rows, device="cpu")

    def written_out(call, st0):
        ref, want, at = st0.clone(), [], 0
        for n, r in zip(lens, rows):
            for j in range(n):          # row by row: committed rows on the cache row, peek rows on a copy
                row = ref[r:r + 1].clone() if _is_peek(j, P) else ref[r:r + 1]
                want.append(call(row, at + j, at + j + 1))
            at += n
        return torch.cat(want, dim=1), ref

    dim = 96
    u, dl, z = torch.randn(1, total, dim), torch.rand(1, total, dim) * 0.3, torch.randn(1, total, dim)
    B, C, A, D = torch.randn(1, total, 16), torch.randn(1, total, 16), -torch.exp(torch.randn(dim, 16) * 0.5), torch.randn(dim)
    st0 = torch.randn(4, dim, 16) * 0.3
    assert not aum_hip.scan_tm_chunk_var_supported(st0, u[0])
    st = st0.clone()
    y = aum_hip.scan_stream(st, u, dl, A, B, C, D, z, None, False, False, smap, lib=lib, peek_every=P)
    want, ref = written_out(lambda row, a, b: aum_hip.scan_stream(row, u[:, a:b], dl[:, a:b], A, B[:, a:b], C[:, a:b], D, z[:, a:b], None, False,
                                                                  False, None, lib=lib), st0)
    assert torch.equal(y, want) and torch.equal(st, ref) and torch.equal(st[1], st0[1])
    x, w, b5 = torch.randn(1, total, 64), torch.randn(64, 5) * 0.5, torch.randn(64)
    cs0 = torch.randn(4, 64, 5)
    assert not aum_hip.conv1d_tm_chunk_var_supported(x[0], cs0)
    cs = cs0.clone()
    y = aum_hip.conv1d_stream(x, cs, w, b5, True, smap, lib=lib, peek_every=P)
    want, ref = written_out(lambda row, a, b: aum_hip.conv1d_stream(x[:, a:b], row, w, b5, True, None, lib=lib), cs0)
    assert torch.equal(y, want) and torch.equal(cs, ref) and torch.equal(cs[1], cs0[1])
    with pytest.raises(ValueError, match="exclude"):
        aum_hip.conv1d_stream(x, cs, w, b5, True, smap, lib=lib, peek=True, peek_every=P)


# ---- module ------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def row_wise_linear():
    """torch.nn.functional.linear as K element-wise multiply-adds in fp32, rounded to the input's dtype: a row's result then depends on
    that row alone.  A library GEMM's bits may depend on its row count (measured on the host: one Mamba(64) block, the ssm caches of the
    one call and of the chain of group calls differed by 3e-8 relative at (batch 2, P 4, T 17) and were equal at (2, 8, 9)), and the one
    call and the group calls hand the projections different row counts.  With this in place of the GEMMs in BOTH forms, the block's
    caches are a function of the conv and scan kernels and the ladder alone, and bit equality is theirs to keep."""
    import torch.nn.functional as F
    orig = F.linear

    def linear(x, w, b=None):
        x2 = x.reshape(-1, x.shape[-1]).float()
        acc = torch.zeros(x2.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
        wt = w.float().t().contiguous()
        for k in range(x2.shape[1]):
            acc.addcmul_(x2[:, k:k + 1], wt[k])
        if b is not None:
            acc += b.float()
        return acc.to(x.dtype).reshape(*x.shape[:-1], w.shape[0])

    F.linear = linear
    try:
        yield
    finally:
        F.linear = orig


def check_mamba_peek_every(m, h, P, device, bar, seq_map=None, pool_rows=None):
    """step_chunk(h, peek_every=P) against the chain of step_chunk(peek=True) calls on the groups of P + 1 rows (the trailing partial group
    without peek), on the ladder (aum_hip.debug.stream_fused off for the reference).  The caches bit for bit, the outputs within bar.
    Both forms run under row_wise_linear()."""
    nrows = h.shape[0] if pool_rows is None else pool_rows
    launches = []
    orig = aum_hip._launch
    aum_hip._launch = lambda fn, args, t, lib, name, meta=None: (launches.append(name), orig(fn, args, t, lib, name, meta))[1]
    with torch.no_grad(), row_wise_linear():
        c, s = m.allocate_inference_cache(nrows, 0, dtype=torch.float32)
        torch.manual_seed(5)
        c.copy_(torch.randn(c.shape)), s.copy_(torch.randn(s.shape) * 0.3)
        c0, s0 = c.clone(), s.clone()
        try:
            out, _, _ = m.step_chunk(h, c, s, seq_map=seq_map, peek_every=P)
        finally:
            aum_hip._launch = orig
        ca, sa = c0.clone(), s0.clone()
        ref = torch.zeros_like(out)
        with bc._fused(False):
            if seq_map is None:
                T = h.shape[1]
                for a in range(0, T, P + 1):
                    b = min(a + P + 1, T)
                    ref[:, a:b] = m.step_chunk(h[:, a:b], ca, sa, peek=(b - a == P + 1))[0]
            else:
                lens = seq_map.lens
                starts = [sum(lens[:i]) for i in range(len(lens))]
                for g in range(max(-(-n // (P + 1)) for n in lens)):
                    for flagged in (True, False):
                        sel, idx = [], []
                        for n, at in zip(lens, starts):
                            a, b = g * (P + 1), min((g + 1) * (P + 1), n)
                            take = b > a and (b - a == P + 1) == flagged
                            sel.append(b - a if take else 0)
                            idx += list(range(at + a, at + b)) if take else []
                        if idx:
                            ref[0, idx] = m.step_chunk(h[:, idx], ca, sa, seq_map=aum_hip.seq_map(sel, seq_map.rows, device=device), peek=flagged)[0][0]
    _sync(device)
    assert "conv1d_tm_chunk_peeks" in launches and "scan_tm_chunk_peeks" in launches and "stream_block" not in launches, launches
    e_out = rel_err(_np(out), _np(ref))
    e_c, e_s = rel_err(_np(c), _np(ca)), rel_err(_np(s), _np(sa))
    print(f"step_chunk(peek_every={P}) vs the chain of peek=True calls: out {e_out:.3e} (bar {bar:.0e}), conv cache {e_c:.3e}, ssm cache {e_s:.3e}, "
          f"caches bit-equal: {torch.equal(c, ca) and torch.equal(s, sa)}")
    assert e_out < bar
    assert torch.equal(c, ca) and torch.equal(s, sa)
    assert not torch.equal(s, s0)


def check_mamba_exclusive_arguments(m, device):
    h = torch.randn(2, 6, m.d_model, device=device).to(m.in_proj.weight.dtype)
    c, s = m.allocate_inference_cache(2, 0, dtype=torch.float32)
    c0, s0 = c.clone(), s.clone()
    with torch.no_grad():
        with pytest.raises(ValueError, match="peek_every"):
            m.step_chunk(h, c, s, peek=True, peek_every=2)
        with pytest.raises(ValueError, match="peek_every"):
            m.step_chunk(h, c, s, commit=False, peek_every=2)
        with pytest.raises(ValueError, match="peek_every"):
            m.step_chunk(h, c, s, peek_every=0)
    assert torch.equal(c, c0) and torch.equal(s, s0)


# ---- model -------------------------------------------------------------------------------------------------------------------------
def _ctx(device, autocast_dtype):
    if autocast_dtype is None:
        return contextlib.nullcontext
    return lambda: torch.autocast(device_type=torch.device(device).type, dtype=autocast_dtype)


def _cache_err(a, b):
    return max(max(rel_err(_np(c1), _np(c2)), rel_err(_np(s1), _np(s2))) for (c1, s1), (c2, s2) in zip(a["layers"].values(), b["layers"].values()))


def check_model_timeline(embed_dim, device, autocast_dtype=None):
    """stream_timeline of the whole clip: every column against the per-column stream_push(read=True) loop on a twin cache, the last column
    against model(spec), caches and counts against the twin; 5 columns then 11 against the 16 in one call, and stream_read behind it"""
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(11)
    spec = torch.randn(2, 256, 128, device=device)
    bar = 1e-4 if autocast_dtype is None else 2e-2
    with torch.no_grad(), _ctx(device, autocast_dtype)():
        full = model(spec)
        cache, twin, split = model.allocate_inference_cache(2), model.allocate_inference_cache(2), model.allocate_inference_cache(2)
        cols, logits = model.stream_timeline(spec, cache)
        assert cols == 16 == cache["columns"] and logits.shape == (2, 16, 7)
        for j in range(16):
            n, want = model.stream_push(spec[:, 16 * j:16 * (j + 1)], twin, read=True)
            e = rel_err(_np(logits[:, j]), _np(want))
            print(f"timeline column {j}: vs stream_push(read=True) {e:.3e} (bar {bar:.0e})")
            assert n == j + 1 and e < bar
        e_full, e_cache = rel_err(_np(logits[:, -1]), _np(full)), _cache_err(cache, twin)
        print(f"timeline last column vs model(spec) {e_full:.3e}, caches vs the per-column loop {e_cache:.3e} (bar {bar:.0e})")
        assert e_full < bar and e_cache < bar
        n5, l5 = model.stream_timeline(spec[:, :80], split)
        n16, l11 = model.stream_timeline(spec[:, 80:], split)
        assert (n5, n16) == (5, 16) and l5.shape == (2, 5, 7) and l11.shape == (2, 11, 7)
        e_split = rel_err(_np(torch.cat((l5, l11), dim=1)), _np(logits))
        e_read = rel_err(_np(model.stream_read(split)), _np(model.stream_read(cache)))
        print(f"timeline 5 + 11 columns vs 16: logits {e_split:.3e}, stream_read behind them {e_read:.3e}, caches {_cache_err(split, cache):.3e} (bar {bar:.0e})")
        assert e_split < bar and e_read < bar and _cache_err(split, cache) < bar
        feats = model.stream_timeline(spec, model.allocate_inference_cache(2), return_features=True)[1]
        assert feats.shape == (2, 16, embed_dim) and rel_err(_np(model.head(feats)), _np(logits)) < bar


def check_model_timeline_many(embed_dim, device, autocast_dtype=None):
    """two sessions at different offsets with different k in a pool of 4, against the sessions served alone"""
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(12)
    spec = torch.randn(2, 256, 128, device=device)
    bar = 1e-4 if autocast_dtype is None else 2e-2
    with torch.no_grad(), _ctx(device, autocast_dtype)():
        pool = model.allocate_stream_pool(4)
        alone = [model.allocate_inference_cache(1), model.allocate_inference_cache(1)]
        sessions = [2, 0]                                       # clip 0 on row 2, clip 1 on row 0
        assert model.stream_push_many([spec[1, :48]], pool, [0]) == [3]        # clip 1 is three columns ahead
        model.stream_push(spec[1:2, :48], alone[1])
        at = [0, 3]
        for ka, kb in ((5, 2), (3, 7), (8, 4)):
            pieces = [spec[0, 16 * at[0]:16 * (at[0] + ka)], spec[1, 16 * at[1]:16 * (at[1] + kb)]]
            cols, logits = model.stream_timeline_many(pieces, pool, sessions)
            at = [at[0] + ka, at[1] + kb]
            assert cols == at and [pool["columns"][r] for r in sessions] == at
            assert [tuple(t.shape) for t in logits] == [(ka, 7), (kb, 7)]
            for i, piece in enumerate(pieces):
                n, want = model.stream_timeline(piece.unsqueeze(0), alone[i])
                e = rel_err(_np(logits[i]), _np(want[0]))
                print(f"timeline_many session {sessions[i]} at column {at[i]}: vs served alone {e:.3e} (bar {bar:.0e})")
                assert n == at[i] and e < bar
        assert at == [16, 16]
        e = rel_err(_np(torch.stack((logits[0][-1], logits[1][-1]))), _np(model(spec)))
        print(f"timeline_many last columns vs model(spec) {e:.3e} (bar {bar:.0e})")
        assert e < bar
        for i, r in enumerate(sessions):
            for (pc, ps), (ac, as_) in zip(pool["layers"].values(), alone[i]["layers"].values()):
                assert rel_err(_np(pc[r]), _np(ac[0])) < bar and rel_err(_np(ps[r]), _np(as_[0])) < bar
        for pc, ps in pool["layers"].values():                  # rows no session owns
            assert not pc[1].any() and not pc[3].any() and not ps[1].any() and not ps[3].any()


def check_model_timeline_refusals(device):
    """_check_push stands in front of the new calls: a refused call leaves caches and column counts as they were"""
    model = make_causal_aum(64, device, depth=2)
    torch.manual_seed(13)
    spec = torch.randn(1, 256, 128, device=device)
    with torch.no_grad():
        cache, pool = model.allocate_inference_cache(1), model.allocate_stream_pool(3)
        model.stream_timeline(spec[:, :32], cache)
        model.stream_timeline_many([spec[0, :32]], pool, [1])
        snap = lambda cch: [(c.clone(), s.clone()) for c, s in cch["layers"].values()]
        same = lambda cch, sn: all(torch.equal(c, c1) and torch.equal(s, s1) for (c, s), (c1, s1) in zip(cch["layers"].values(), sn))
        s_cache, s_pool = snap(cache), snap(pool)
        for bad in (spec[:, :24], spec[:, :0], spec[:, :32, :64], spec[0, :32], spec.expand(2, -1, -1)[:, :32], spec[:, :240]):
            with pytest.raises(ValueError):
                model.stream_timeline(bad, cache)
        with pytest.raises(ValueError, match="stream_timeline_many"):
            model.stream_timeline(spec[:, :32], pool)
        for args in (([spec[0, :24]], [1]), ([spec[0, :32], spec[0, :32]], [1, 1]), ([spec[0, :32]], [3]), ([spec[0, :32]], [1, 2]),
                     ([spec[0, :240]], [1]), ([], [])):
            with pytest.raises(ValueError):
                model.stream_timeline_many(args[0], pool, args[1])
        with pytest.raises(ValueError, match="pool"):
            model.stream_timeline_many([spec[0, :32]], cache, [0])
        assert cache["columns"] == 2 and pool["columns"] == [0, 2, 0]
        assert same(cache, s_cache) and same(pool, s_pool)
