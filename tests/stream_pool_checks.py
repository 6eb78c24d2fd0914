"""Checks of streaming MANY sessions at different positions in one call, shared by tests/test_stream_pool.py (lane-array library, host
tensors) and tests/test_gpu_stream_pool.py (libaum_hip.so on the MI355X): aum_conv1d_tm_chunk_var / aum_scan_tm_chunk_var,
Mamba.step_chunk(seq_map=) and AudioMamba.allocate_stream_pool / stream_push_many / stream_read(sessions=) / stream_reset.

Expected values never come from the kernels under test.  The bitwise checks compare every session of a packed call with the EXISTING
fixed-batch kernels (scan_tm_chunk / conv1d_tm_chunk at batch 1, pinned to the oracle by tests/stream_checks.py) on a clone of that
session's entry cache; the accuracy checks compare with the fp64 oracle on the whole sequence (stream_checks.scan_setup / conv_setup:
ref_out, ref_state) under the existing bars: OUT_BAR per dtype, CACHE_BAR = 1e-4.  Module and model: 1e-4 fp32, 2e-2 bf16 autocast, the
bars of check_mamba_chunks / check_model_stream."""
import contextlib

import numpy as np
import pytest
import torch

import aum_hip
from conftest import rel_err
from stream_checks import CACHE_BAR, DT, OUT_BAR, conv_setup, make_causal_aum, scan_setup

SENTINEL = 7.25       # what the pool rows that no session owns hold: they must come back unchanged
S = 4


def _np(t):
    return t.detach().float().cpu().numpy()


# ---- the two operators behind one interface ----------------------------------------------------------
class ScanOp:
    """pieces: [(session, first token, tokens)] in pack order"""
    name = "scan"

    @staticmethod
    def setup(case, device, batch, dim=None):
        return scan_setup(case, device, batch=batch, **({} if dim is None else {"dim": dim}))

    @staticmethod
    def pack(s, pieces):
        o = s["ops"]
        cat = lambda a: torch.cat([a[b, t:t + n] for b, t, n in pieces], dim=0)
        u, d, Bm, Cm = cat(o["u"]), cat(o["delta"]), cat(o["B"]), cat(o["C"])
        dim, N = u.shape[1], Bm.shape[1]
        bc = torch.cat((Bm, Cm), dim=1)                      # B, C as column blocks of one packed row, read in place
        if o["z"] is not None:                               # u, z as the halves of one packed xz row (row stride 2 dim)
            xz = torch.cat((u, cat(o["z"])), dim=1)
            u, z = xz[:, :dim], xz[:, dim:]
        else:
            z = None
        return {"u": u, "delta": d, "z": z, "B": bc[:, :N], "C": bc[:, N:]}

    @staticmethod
    def var(s, pool, p, smap, lib, out=None):
        o = s["ops"]
        return aum_hip.scan_tm_chunk_var(pool, p["u"], p["delta"], o["A"], p["B"], p["C"], o["D"], p["z"], o["bias"], o["sp"], o["act"],
                                         seq_map=smap, out=out, lib=lib)

    @staticmethod
    def solo(s, state1, b, t, n, lib):
        o = s["ops"]
        sl = lambda a: None if a is None else a[b:b + 1, t:t + n]
        return aum_hip.scan_tm_chunk(state1, sl(o["u"]), sl(o["delta"]), o["A"], sl(o["B"]), sl(o["C"]), o["D"], sl(o["z"]), o["bias"], o["sp"],
                                     o["act"], lib=lib)[0]


class ConvOp:
    name = "conv"

    @staticmethod
    def setup(case, device, batch, dim=None):
        return conv_setup(case, device, batch=batch, **({} if dim is None else {"dim": dim}))

    @staticmethod
    def pack(s, pieces):
        x = torch.cat([s["x"][b, t:t + n] for b, t, n in pieces], dim=0)
        if s["x"].stride(1) != s["x"].shape[2]:              # the case reads x as the first half of xz rows: so does the pack
            x = torch.cat((x, torch.zeros_like(x)), dim=1)[:, :x.shape[1]]
        return {"x": x}

    @staticmethod
    def var(s, pool, p, smap, lib, out=None):
        return aum_hip.conv1d_tm_chunk_var(p["x"], pool, s["w"], s["bias"], s["silu"], seq_map=smap, out=out, lib=lib)

    @staticmethod
    def solo(s, state1, b, t, n, lib):
        return aum_hip.conv1d_tm_chunk(s["x"][b:b + 1, t:t + n], state1, s["w"], s["bias"], s["silu"], lib=lib)[0]


def _pool(s, rows, spare=2):
    """a pool of len(rows) + spare cache rows: session i's entry cache in row rows[i], the sentinel everywhere else"""
    entry = s["entry"]
    pool = torch.full((entry.shape[0] + spare,) + tuple(entry.shape[1:]), SENTINEL, dtype=torch.float32, device=entry.device)
    for i, r in enumerate(rows):
        pool[r] = entry[i]
    return pool


def _lens(rng, T, n):
    """per-session lengths in [0, T], at least one 0 and one T"""
    lens = [int(v) for v in rng.integers(0, T + 1, size=n)]
    a, b = (int(v) for v in rng.permutation(n)[:2])
    lens[a], lens[b] = 0, T
    return lens


def _seed(s, salt):
    return 7919 * salt + 31 * s["T"] + len(s["dt"])


def _check_exact(s, op, lib, pieces, rows_of, out, pool, skip=()):
    """every packed session = the fixed-batch kernel at batch 1 on a clone of its entry cache, bitwise"""
    at = 0
    for b, t, n in pieces:
        if b not in skip:
            st1 = s["entry"][b:b + 1].clone()
            if n:
                o1 = op.solo(s, st1, b, t, n, lib)
                assert torch.equal(out[at:at + n], o1), f"{op.name}: outputs of session {b} ({n} rows at pack row {at}) differ from the batch-1 call"
            assert torch.equal(pool[rows_of[b]], st1[0]), f"{op.name}: cache row {rows_of[b]} of session {b} differs from the batch-1 call"
        at += n


def check_packing_bitwise(op, case, lib, device, sessions=S, dim=None):
    s = op.setup(case, device, sessions, dim)
    T = s["T"]
    rng = np.random.default_rng(_seed(s, 1))
    lens = _lens(rng, T, sessions)
    rows = [int(r) for r in rng.permutation(sessions + 2)[:sessions]]          # shuffled rows of a pool of S + 2
    order = [int(b) for b in rng.permutation(sessions)]                        # and a shuffled place in the pack
    pool = _pool(s, rows)
    pieces = [(b, 0, lens[b]) for b in order]
    smap = aum_hip.seq_map([n for _, _, n in pieces], [rows[b] for b in order], device=device)
    out = op.var(s, pool, op.pack(s, pieces), smap, lib)
    assert out.dtype == DT[s["dt"]] and out.shape[0] == sum(lens)
    _check_exact(s, op, lib, pieces, rows, out, pool)
    for r in set(range(sessions + 2)) - set(rows):
        assert torch.equal(pool[r], torch.full_like(pool[r], SENTINEL)), f"{op.name}: spare cache row {r} was written"


def check_null_indices(op, case, lib, device, sessions=S, dim=None):
    s = op.setup(case, device, sessions, dim)
    lens = _lens(np.random.default_rng(_seed(s, 2)), s["T"], sessions)
    pieces = [(b, 0, lens[b]) for b in range(sessions)]
    p = op.pack(s, pieces)
    pool_a, pool_b = s["entry"].clone(), s["entry"].clone()
    m_null = aum_hip.seq_map(lens, None, device=device)
    m_id = aum_hip.seq_map(lens, range(sessions), device=device)
    assert m_null.idx is None and m_id.idx is not None and m_null.rows == m_id.rows
    out_a, out_b = op.var(s, pool_a, p, m_null, lib), op.var(s, pool_b, p, m_id, lib)
    assert torch.equal(out_a, out_b) and torch.equal(pool_a, pool_b)
    _check_exact(s, op, lib, pieces, list(range(sessions)), out_a, pool_a)


def check_var_vs_oracle(op, case, lib, device, sessions=S, dim=None):
    """all sessions advanced to T over several packed calls, each by its own cut schedule; sessions absent from calls and calls that
    carry an explicitly empty sequence"""
    s = op.setup(case, device, sessions, dim)
    T = s["T"]
    rng = np.random.default_rng(_seed(s, 3))
    rows = [int(r) for r in rng.permutation(sessions + 2)[:sessions]]
    pool = _pool(s, rows)
    cuts = []
    for b in range(sessions):            # session b: a few cut points of its own
        pts = sorted(set(int(v) for v in rng.integers(1, T, size=int(rng.integers(0, 4))))) if T > 1 else []
        cuts.append([q - p for p, q in zip([0] + pts, pts + [T])])
    done, got = [0] * sessions, [[] for _ in range(sessions)]
    n_absent = n_empty = call = 0
    while any(cuts):
        pieces = []
        for b in (int(v) for v in rng.permutation(sessions)):
            how = "absent" if (call == 0 and b == 0) else "empty" if (call == 0 and b == 1) else \
                rng.choice(["absent", "empty", "go"], p=[0.2, 0.15, 0.65])
            if how == "absent":
                n_absent += 1
            elif how == "empty" or not cuts[b]:
                n_empty += 1
                pieces.append((b, done[b], 0))
            else:
                pieces.append((b, done[b], cuts[b].pop(0)))
        call += 1
        if not pieces:
            continue
        smap = aum_hip.seq_map([n for _, _, n in pieces], [rows[b] for b, _, _ in pieces], device=device)
        if smap.total == 0:
            continue
        out = op.var(s, pool, op.pack(s, pieces), smap, lib)
        at = 0
        for b, _, n in pieces:
            got[b].append(out[at:at + n])
            done[b] += n
            at += n
    assert done == [T] * sessions and n_absent and n_empty
    out = torch.stack([torch.cat(g, dim=0) for g in got], dim=0)
    state = torch.stack([pool[r] for r in rows], dim=0)
    e_out, e_state = rel_err(_np(out), s["ref_out"]), rel_err(_np(state), s["ref_state"])
    print(f"{op.name} packed, {call} calls vs oracle: out {e_out:.3e} (bar {OUT_BAR[s['dt']]:.0e}), cache {e_state:.3e} (bar {CACHE_BAR:.0e})")
    assert e_out < OUT_BAR[s["dt"]]
    assert e_state < CACHE_BAR
    for r in set(range(sessions + 2)) - set(rows):
        assert torch.equal(pool[r], torch.full_like(pool[r], SENTINEL))


def check_out_of_range_index(op, case, lib, sessions=S):
    """host build only: a sequence whose cache row is outside the pool is a no-op -- its output rows and every cache row it could have
    meant keep their values, the other sequences are exact"""
    s = op.setup(case, "cpu", sessions)
    T = s["T"]
    lens = [T, max(T // 2, 1), T, max(T - 1, 1)][:sessions]
    pieces = [(b, 0, lens[b]) for b in range(sessions)]
    p = op.pack(s, pieces)
    for bad_value in (sessions + 2, -1, 1 << 30):
        rows = list(range(sessions))
        pool = _pool(s, rows)
        before = pool.clone()
        smap = aum_hip.seq_map(lens, rows, device="cpu")
        idx = smap.idx.clone()
        idx[1] = bad_value
        out = torch.full((sum(lens), p[list(p)[0]].shape[1]), SENTINEL, dtype=DT[s["dt"]])
        op.var(s, pool, p, smap._replace(idx=idx), lib, out=out)
        assert torch.equal(out[lens[0]:lens[0] + lens[1]], torch.full_like(out[lens[0]:lens[0] + lens[1]], SENTINEL)), "the refused sequence wrote outputs"
        assert torch.equal(pool[1], before[1]) and torch.equal(pool[sessions:], before[sessions:]), "a cache row changed that no valid sequence owns"
        _check_exact(s, op, lib, pieces, rows, out, pool, skip=(1,))


# ---- binding ------------------------------------------------------------------------------------------
def check_seq_map_validates(device):
    m = aum_hip.seq_map([3, 0, 5], [4, 1, 0], device=device)
    assert m.lens == (3, 0, 5) and m.rows == (4, 1, 0) and m.total == 8
    assert m.cu.dtype == torch.int32 and m.cu.cpu().tolist() == [0, 3, 3, 8] and m.idx.cpu().tolist() == [4, 1, 0]
    assert torch.device(m.cu.device).type == torch.device(device).type
    with pytest.raises(AttributeError):
        m.total = 9
    for lens, rows in (([1, -1], None), ([1, 2], [0, 0]), ([1, 2], [0, -1]), ([1, 2], [0]), ([], None)):
        with pytest.raises(ValueError):
            aum_hip.seq_map(lens, rows, device=device)
    # the range check happens where the cache is known
    dim = 64
    st = torch.zeros(2, dim, 16, device=device)
    u = torch.zeros(3, dim, device=device)
    bc = torch.zeros(3, 16, device=device)
    with pytest.raises(ValueError, match="pool has 2 rows"):
        aum_hip.scan_tm_chunk_var(st, u, u, torch.zeros(dim, 16, device=device), bc, bc, seq_map=aum_hip.seq_map([1, 2], [0, 2], device=device),
                                  lib=None if torch.device(device).type == "cuda" else aum_hip._product)
    with pytest.raises(ValueError, match="describes 4 rows"):
        aum_hip.conv1d_tm_chunk_var(u, torch.zeros(2, dim, 4, device=device), torch.zeros(dim, 4, device=device),
                                    seq_map=aum_hip.seq_map([1, 3], None, device=device),
                                    lib=None if torch.device(device).type == "cuda" else aum_hip._product)


# ---- module -------------------------------------------------------------------------------------------
def check_mamba_pool(d_model, device):
    """3 sessions prefilled to different lengths through the existing path, then ragged packed step_chunk(seq_map=) calls vs every
    session run alone through step_chunk (not bitwise: the projection GEMMs see different row counts)"""
    from types import SimpleNamespace
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(5)
    m = Mamba(d_model, layer_idx=0, bimamba_type="none").eval().to(device)
    prefill = (5, 9, 17)
    calls = [(3, 0, 2), (1, 4, 8), (0, 5, 1), (7, 1, 0), (2, 2, 9)]           # new tokens per session per call
    rows = (2, 0, 3)
    L = [p + sum(c[i] for c in calls) for i, p in enumerate(prefill)]
    xs = [torch.randn(1, n, d_model, device=device) for n in L]
    with torch.no_grad():
        solo = []
        for i, p in enumerate(prefill):
            params = SimpleNamespace(key_value_memory_dict={}, seqlen_offset=0)
            m(xs[i][:, :p], inference_params=params)
            solo.append(params.key_value_memory_dict[0])
        conv_pool = torch.full((4,) + tuple(solo[0][0].shape[1:]), SENTINEL, device=device)
        ssm_pool = torch.full((4,) + tuple(solo[0][1].shape[1:]), SENTINEL, device=device)
        for i, r in enumerate(rows):
            conv_pool[r], ssm_pool[r] = solo[i][0][0], solo[i][1][0]
        at = list(prefill)
        worst = 0.0
        for c in calls:
            smap = aum_hip.seq_map(c, rows, device=device)
            packed = torch.cat([xs[i][:, at[i]:at[i] + n] for i, n in enumerate(c)], dim=1)
            out, _, _ = m.step_chunk(packed, conv_pool, ssm_pool, seq_map=smap)
            assert out.shape == packed.shape
            o = 0
            for i, n in enumerate(c):
                if n:
                    ref, _, _ = m.step_chunk(xs[i][:, at[i]:at[i] + n], solo[i][0], solo[i][1])
                    worst = max(worst, rel_err(_np(out[:, o:o + n]), _np(ref)))
                worst = max(worst, rel_err(_np(conv_pool[rows[i]]), _np(solo[i][0][0])), rel_err(_np(ssm_pool[rows[i]]), _np(solo[i][1][0])))
                at[i] += n
                o += n
        print(f"Mamba({d_model}) packed sessions vs each alone: worst of outputs and caches {worst:.3e} (bar 1e-4)")
        assert torch.equal(conv_pool[1], torch.full_like(conv_pool[1], SENTINEL)) and torch.equal(ssm_pool[1], torch.full_like(ssm_pool[1], SENTINEL))
        assert worst < 1e-4
        with pytest.raises(ValueError):
            m.step_chunk(packed, conv_pool, ssm_pool, seq_map=aum_hip.seq_map(calls[-1], (0, 1, 4), device=device))


# ---- model --------------------------------------------------------------------------------------------
def _snapshot(pool):
    return {i: (c.clone(), s.clone()) for i, (c, s) in pool["layers"].items()}, list(pool["columns"])


def _unchanged(pool, snap):
    layers, cols = snap
    return pool["columns"] == cols and all(torch.equal(pool["layers"][i][0], c) and torch.equal(pool["layers"][i][1], s) for i, (c, s) in layers.items())


def check_model_pool(embed_dim, device, autocast_dtype=None):
    """three clips in a pool of 4 on staggered schedules with ragged hops (clip 1 starts two calls late); the slot of clip 2 is reset
    mid-way and reused for a fourth clip.  Final reads vs model(spec), a mid-clip read vs a solo session at the same column under the
    single-session API, reads do not advance, refused calls change nothing."""
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(13)
    spec = torch.randn(4, 256, 128, device=device)
    ctx = (lambda: torch.autocast(device_type=torch.device(device).type, dtype=autocast_dtype)) if autocast_dtype is not None else contextlib.nullcontext
    bar = 1e-4 if autocast_dtype is None else 2e-2
    # (clip, pool row, first call, hops in columns); clip 2 is cut off after its 6 columns
    plan = [(0, 2, 0, [1, 2, 1, 4, 3, 5]), (1, 0, 2, [4, 1, 2, 1, 8]), (2, 3, 0, [2, 1, 3]), (3, 3, 3, [1, 4, 2, 1, 8])]
    with torch.no_grad(), ctx():
        full = model(spec)
        pool = model.allocate_stream_pool(4)
        assert pool["columns"] == [0, 0, 0, 0] and pool["batch"] == 4
        with pytest.raises(ValueError, match="stream_push_many"):
            model.stream_push(spec[:, :16], pool)
        pushed = {}
        errs = {}
        for call in range(8):
            specs, rows, clips = [], [], []
            for clip, row, first, hops in plan:
                j = call - first
                if 0 <= j < len(hops):
                    c0 = sum(hops[:j])
                    specs.append(spec[clip, 16 * c0:16 * (c0 + hops[j])])
                    rows.append(row)
                    clips.append((clip, c0 + hops[j]))
            if call == 6:       # refused calls, each checked against a snapshot: clip 0 (row 2) is complete here
                assert pool["columns"][2] == 16
                snap = _snapshot(pool)
                for bad_specs, bad_rows in ((specs + specs[:1], rows + rows[:1]),                        # a duplicate session
                                            ([spec[0, :16]], [2]),                                     # a column overflow
                                            (specs[:-1] + [spec[1, :24]], rows),                       # a wrong frame count
                                            (specs, rows[:-1] + [4]),                                  # a session outside the pool
                                            (specs[:-1] + [spec[1, :16, :64]], rows)):                 # wrong mel bins
                    with pytest.raises(ValueError):
                        model.stream_push_many(bad_specs, pool, bad_rows)
                    assert _unchanged(pool, snap), "a refused stream_push_many changed the pool"
                with pytest.raises(ValueError):
                    model.stream_reset(pool, [4])
                with pytest.raises(ValueError):
                    model.stream_read(pool, sessions=[4])
                assert _unchanged(pool, snap)
            got = model.stream_push_many(specs, pool, rows)
            assert got == [c for _, c in clips]
            for (clip, cols), row in zip(clips, rows):
                pushed[clip] = cols
                if cols == 16:
                    a = model.stream_read(pool, sessions=[row])
                    b = model.stream_read(pool, sessions=[row])
                    assert a.shape == full[clip:clip + 1].shape and torch.equal(a, b), "stream_read advanced the caches"
                    errs[f"clip {clip} final"] = rel_err(_np(a), _np(full[clip:clip + 1]))
            if call == 2:       # clip 2 at column 6: the read vs a solo session at the same column, then its slot is freed
                assert pushed[2] == 6
                mid = model.stream_read(pool, sessions=[3])
                solo = model.allocate_inference_cache(1)
                model.stream_push(spec[2:3, :16 * 6], solo)
                errs["clip 2 mid-clip"] = rel_err(_np(mid), _np(model.stream_read(solo)))
                both = model.stream_read(pool, sessions=[3, 2])
                assert both.shape[0] == 2
                errs["gathered pair vs single"] = rel_err(_np(both[:1]), _np(mid))
                model.stream_reset(pool, [3])
                assert pool["columns"][3] == 0 and all(not c[3].any() and not s[3].any() for c, s in pool["layers"].values())
        assert sorted(k for k in errs if "final" in k) == ["clip 0 final", "clip 1 final", "clip 3 final"]
        everything = model.stream_read(pool)
        assert everything.shape[0] == 4
    print(f"model pool ({embed_dim}, {autocast_dtype}): " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bar {bar:.0e})")
    assert max(errs.values()) < bar
