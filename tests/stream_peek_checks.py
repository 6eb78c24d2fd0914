"""Checks of the PEEK ROW of streaming inference (AUM_STREAM_PEEK_LAST / AUM_CONV_PEEK_LAST / AUM_SCAN_PEEK_LAST, aum_hip.stream_block /
conv1d_stream / scan_stream(peek=), Mamba.step_chunk(peek=), AudioMamba.stream_push / stream_push_many(read=)), shared by
tests/test_stream_peek.py (CPU, lane-array library) and tests/test_gpu_stream_peek.py (device library).

The defining property is BIT EQUALITY with two calls the library had before the flag: per session, a committed call on its first len - 1
rows, then an AUM_STREAM_NO_COMMIT call on its last row alone (reference()).  y, conv_state and state are compared with torch.equal;
pool rows no session names stay at the sentinel and the row of a length-1 session stays at its entry values.
Module and model are held to the bars of stream_checks.check_model_stream (1e-4 without autocast, 2e-2 under it): there the in_proj GEMM
sees one more row than in the two-call form, and a library GEMM's bits may depend on its row count."""
import contextlib

import pytest
import torch

import aum_hip
import stream_block_checks as bc
from conftest import rel_err
from stream_checks import CACHE_BAR, make_causal_aum

SENTINEL = bc.SENTINEL
MAX_T = bc.MAX_T
# (lengths, cache rows or None: session i on row i, pool rows).  1: peek only; 2: one committed row; 8 / 9: a fetch block of STREAM_UB = 8
# ends at / just before the peek row; 16, 17, 18: the double block of 16; 0: a no-op.
CASES = {"ragged": ((1, 9, 0, 17), (2, 0, 1, 3), 4), "blocks": ((2, 8, 16, 18), (3, 1, 0, 2), 4), "null_idx": ((9, 1, 17), None, 4)}


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _np(t):
    return t.detach().float().cpu().numpy()


def setup(shape, dt, lens, rows, nrows, device, seed=0):
    o = bc.operands(shape, dt, sum(lens), nrows, device, seed=seed)
    live = list(range(len(lens))) if rows is None else list(rows)
    bc.seed_rows(o, live)
    return o, live, aum_hip.seq_map(lens, rows, device=device)


def reference(o, lens, rows, lib, device):
    """what the library gave before the flag: a committed call on every session's first len - 1 rows, then an uncommitted call on its last
    row alone -- on copies of the pools; returns (y (total, dim), conv, state)"""
    conv, state = o["conv"].clone(), o["state"].clone()
    body, last, at = [], [], 0
    for n in lens:
        body += list(range(at, at + n - 1))
        if n:
            last.append(at + n - 1)
        at += n
    y = torch.zeros(at, o["dim"], dtype=o["x"].dtype, device=device)
    take = lambda t, ix: t.index_select(0, torch.tensor(ix, dtype=torch.int64, device=device))
    if body:
        m = aum_hip.seq_map([max(n - 1, 0) for n in lens], rows, device=device)
        y[body] = aum_hip.stream_block(take(o["x"], body), take(o["z"], body), conv, state, o["plan"], seq_map=m, lib=lib)
    if last:
        m = aum_hip.seq_map([min(n, 1) for n in lens], rows, device=device)
        snap = (conv.clone(), state.clone())
        y[last] = aum_hip.stream_block(take(o["x"], last), take(o["z"], last), conv, state, o["plan"], seq_map=m, commit=False, lib=lib)
        assert torch.equal(conv, snap[0]) and torch.equal(state, snap[1])
    return y, conv, state


def ladder(o, smap, lib, conv, state, peek):
    """conv1d_stream -> xdt_tm_fwd -> scan_stream on the packed rows, as Mamba.step_chunk's ladder calls them (on the host library the
    projection loop has no activation, so bias and softplus are the scan's: stream_block_checks.three_launches)"""
    p, R = o["plan"], o["rank"]
    xc = aum_hip.conv1d_stream(o["x"].unsqueeze(0), conv, p.conv_w, p.conv_b, True, smap, lib=lib, peek=peek)[0]
    if lib.host:
        proj, delta = aum_hip.xdt_tm_fwd(xc, p.w_x, p.w_dt, lib=lib)
        bias, sp, act = p.dt_bias, True, False
    else:
        proj, delta = aum_hip.xdt_tm_fwd(xc, p.w_x, p.w_dt, lib=lib, delta_bias=p.dt_bias, delta_softplus=True)
        bias, sp, act = None, False, True
    u = lambda t: t.unsqueeze(0)
    return aum_hip.scan_stream(state, u(xc), u(delta), p.A, u(proj[:, R:R + 16]), u(proj[:, R + 16:R + 32]), p.D, u(o["z"]), bias, sp, act, smap,
                               lib=lib, peek=peek)[0]


def _assert_pools(o, conv, state, ref_conv, ref_state, lens, live, nrows):
    assert torch.equal(conv, ref_conv) and torch.equal(state, ref_state)
    for r in set(range(nrows)) - set(live):                     # rows no session names
        assert torch.equal(conv[r], torch.full_like(conv[r], SENTINEL)) and torch.equal(state[r], torch.full_like(state[r], SENTINEL))
    for r, n in zip(live, lens):
        if n <= 1:                                              # a no-op, or the peek row alone: the cache row is as it was
            assert torch.equal(conv[r], o["entry"][0][r]) and torch.equal(state[r], o["entry"][1][r])
        else:
            assert not torch.equal(state[r], o["entry"][1][r])


def check_peek_equals_two_calls(shape, dt, lens, rows, nrows, lib, device, block=True, steps=True):
    """property 1 for the one launch (block) and for the ladder of three launches with the two flags (steps), and property 3: the two
    agree with each other"""
    o, live, smap = setup(shape, dt, lens, rows, nrows, device)
    y_ref, c_ref, s_ref = reference(o, lens, rows, lib, device)
    got = {}
    if block:
        c, s = o["conv"].clone(), o["state"].clone()
        got["block"] = (aum_hip.stream_block(o["x"], o["z"], c, s, o["plan"], seq_map=smap, lib=lib, peek=True), c, s)
    if steps:
        c, s = o["conv"].clone(), o["state"].clone()
        got["steps"] = (ladder(o, smap, lib, c, s, True), c, s)
    _sync(device)
    for name, (y, c, s) in got.items():
        assert torch.equal(y, y_ref), name
        _assert_pools(o, c, s, c_ref, s_ref, lens, live, nrows)
    if block and steps:
        for a, b in zip(got["block"], got["steps"]):
            assert torch.equal(a, b)
    # with AUM_STREAM_NO_COMMIT nothing is written, and the rows are the same rows
    if block:
        c, s = o["conv"].clone(), o["state"].clone()
        y = aum_hip.stream_block(o["x"], o["z"], c, s, o["plan"], seq_map=smap, lib=lib, peek=True, commit=False)
        _sync(device)
        assert torch.equal(y, y_ref) and torch.equal(c, o["conv"]) and torch.equal(s, o["state"])


def check_flag_off_unchanged(shape, dt, lib, device):
    """peek=False: the one launch against the three launches on the same ragged case, as before the flag"""
    lens, rows, nrows = CASES["ragged"]
    o, live, smap = setup(shape, dt, lens, rows, nrows, device)
    c3, s3 = o["conv"].clone(), o["state"].clone()
    y3 = bc.three_launches(o, smap, lib, conv=c3, state=s3)
    c, s = o["conv"].clone(), o["state"].clone()
    y = aum_hip.stream_block(o["x"], o["z"], c, s, o["plan"], seq_map=smap, lib=lib, peek=False)
    cl, sl = o["conv"].clone(), o["state"].clone()
    yl = ladder(o, smap, lib, cl, sl, False)
    _sync(device)
    for yy, cc, ss in ((y, c, s), (yl, cl, sl)):
        assert torch.equal(yy, y3) and torch.equal(cc, c3) and torch.equal(ss, s3)
    assert not torch.equal(s[2], o["entry"][1][2])              # the length-1 session did advance its row: this is not the peek


def check_limits(lib, device):
    """MAX_T + 1 rows with the flag: the code of the unflagged call, nothing touched; MAX_T rows with the flag: taken"""
    o, live, smap = setup("small", "bf16", (MAX_T + 1,), (0,), 2, device)
    total = MAX_T + 1
    y = torch.full((total, o["dim"]), 3.0, dtype=o["x"].dtype, device=device)
    scratch = torch.zeros(int(lib.c.aum_stream_block_scratch_bytes(total, o["dim"], o["plan"].w_x.shape[0])), dtype=torch.uint8, device=device)
    snap = (o["conv"].clone(), o["state"].clone())
    a = bc.raw_args(o, smap, y, scratch, lib)
    plain = bc.call_raw(a, y, lib)
    a.flags = aum_hip.STREAM_PEEK_LAST
    assert bc.call_raw(a, y, lib) == plain == -4
    a.flags = aum_hip.STREAM_PEEK_LAST | aum_hip.STREAM_NO_COMMIT
    assert bc.call_raw(a, y, lib) == -4
    a.flags = 4                                                 # a bit nobody owns is still refused
    a.max_len = 8
    assert bc.call_raw(a, y, lib) == -4
    _sync(device)
    assert torch.equal(o["conv"], snap[0]) and torch.equal(o["state"], snap[1]) and bool((y == 3.0).all())
    assert not aum_hip.stream_block_supported(o["x"], o["z"], o["conv"], o["state"], o["plan"], MAX_T + 1)
    assert aum_hip.stream_block_supported(o["x"][:MAX_T], o["z"][:MAX_T], o["conv"], o["state"], o["plan"], MAX_T)
    with pytest.raises(RuntimeError, match="longest session"):
        aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], seq_map=smap, lib=lib, peek=True)
    assert torch.equal(o["conv"], snap[0]) and torch.equal(o["state"], snap[1])


def check_fixed_batch_goes_packed(shape, dt, lib, device):
    """seq_map=None with peek=True: (batch, T, dim) rows through the packed kernels with the fixed map, session b on cache row b"""
    batch, T = 2, 9
    o, live, smap = setup(shape, dt, (T,) * batch, None, batch, device, seed=4)
    y_ref, c_ref, s_ref = reference(o, (T,) * batch, None, lib, device)
    p, R, dim = o["plan"], o["rank"], o["dim"]
    c, s = o["conv"].clone(), o["state"].clone()
    x3, z3 = o["xz"].view(batch, T, 2 * dim)[..., :dim], o["xz"].view(batch, T, 2 * dim)[..., dim:]
    xc = aum_hip.conv1d_stream(x3, c, p.conv_w, p.conv_b, True, None, lib=lib, peek=True)
    assert xc.shape == (batch, T, dim)
    xc2 = xc.reshape(batch * T, dim)
    if lib.host:
        proj, delta = aum_hip.xdt_tm_fwd(xc2, p.w_x, p.w_dt, lib=lib)
        bias, sp, act = p.dt_bias, True, False
    else:
        proj, delta = aum_hip.xdt_tm_fwd(xc2, p.w_x, p.w_dt, lib=lib, delta_bias=p.dt_bias, delta_softplus=True)
        bias, sp, act = None, False, True
    proj = proj.view(batch, T, -1)
    y = aum_hip.scan_stream(s, xc, delta.view(batch, T, dim), p.A, proj[..., R:R + 16], proj[..., R + 16:R + 32], p.D, z3, bias, sp, act, None,
                            lib=lib, peek=True)
    yb = aum_hip.stream_block(x3, z3, o["conv"].clone(), o["state"].clone(), p, lib=lib, peek=True)
    _sync(device)
    assert torch.equal(y.reshape(batch * T, dim), y_ref) and torch.equal(yb.reshape(batch * T, dim), y_ref)
    assert torch.equal(c, c_ref) and torch.equal(s, s_ref)


def check_host_loop(lib):
    """shapes the packed kernels refuse (a scan of 96 channels, a conv window of 5): the ladder's loop over the sessions advances the
    last row of each on a copy of its cache row -- against the same calls written out"""
    torch.manual_seed(21)
    lens, rows = (3, 1, 0, 4), (2, 0, 1, 3)
    total, smap = sum(lens), aum_hip.seq_map(lens, rows, device="cpu")
    # scan, dim 96
    dim = 96
    u, dl, z = torch.randn(1, total, dim), torch.rand(1, total, dim) * 0.3, torch.randn(1, total, dim)
    B, C, A, D = torch.randn(1, total, 16), torch.randn(1, total, 16), -torch.exp(torch.randn(dim, 16) * 0.5), torch.randn(dim)
    st0 = torch.randn(4, dim, 16) * 0.3
    assert not aum_hip.scan_tm_chunk_var_supported(st0, u[0])
    st = st0.clone()
    y = aum_hip.scan_stream(st, u, dl, A, B, C, D, z, None, False, False, smap, lib=lib, peek=True)
    ref, want, at = st0.clone(), [], 0
    for n, r in zip(lens, rows):
        for a, b, keep in ((at, at + n - 1, True), (at + n - 1, at + n, False)):
            if b > a and a >= at:
                row = ref[r:r + 1] if keep else ref[r:r + 1].clone()
                want.append(aum_hip.scan_stream(row, u[:, a:b], dl[:, a:b], A, B[:, a:b], C[:, a:b], D, z[:, a:b], None, False, False, None, lib=lib))
        at += n
    assert torch.equal(y, torch.cat(want, dim=1)) and torch.equal(st, ref) and torch.equal(st[0], st0[0]) and torch.equal(st[1], st0[1])
    # conv, width 5
    x, w, b5 = torch.randn(1, total, 64), torch.randn(64, 5) * 0.5, torch.randn(64)
    cs0 = torch.randn(4, 64, 5)
    assert not aum_hip.conv1d_tm_chunk_var_supported(x[0], cs0)
    cs = cs0.clone()
    y = aum_hip.conv1d_stream(x, cs, w, b5, True, smap, lib=lib, peek=True)
    ref, want, at = cs0.clone(), [], 0
    for n, r in zip(lens, rows):
        for a, b, keep in ((at, at + n - 1, True), (at + n - 1, at + n, False)):
            if b > a and a >= at:
                row = ref[r:r + 1] if keep else ref[r:r + 1].clone()
                want.append(aum_hip.conv1d_stream(x[:, a:b], row, w, b5, True, None, lib=lib))
        at += n
    assert torch.equal(y, torch.cat(want, dim=1)) and torch.equal(cs, ref) and torch.equal(cs[0], cs0[0])


# ---- module ------------------------------------------------------------------------------------------------------------------------
def check_mamba_peek(m, h, device, bar, cache_bar, seq_map=None, pool_rows=None, exact_caches=False, expect_fused=None):
    """step_chunk(h, peek=True) against step_chunk(all rows but each session's last) followed by step_chunk(the last rows) on copies of
    the resulting caches.  bar: outputs; cache_bar: the caches (exact_caches: torch.equal first, see the caller)"""
    nrows = h.shape[0] if pool_rows is None else pool_rows
    with torch.no_grad():
        c, s = m.allocate_inference_cache(nrows, 0, dtype=torch.float32)
        torch.manual_seed(5)
        c.copy_(torch.randn(c.shape)), s.copy_(torch.randn(s.shape) * 0.3)
        c0, s0 = c.clone(), s.clone()
        calls = []
        orig = aum_hip.stream_block
        aum_hip.stream_block = lambda *a, **kw: (calls.append(kw.get("peek")), orig(*a, **kw))[1]
        try:
            out, _, _ = m.step_chunk(h, c, s, seq_map=seq_map, peek=True)
        finally:
            aum_hip.stream_block = orig
        if expect_fused is not None:
            assert calls == ([True] if expect_fused else []), calls
        ca, sa = c0.clone(), s0.clone()
        if seq_map is None:
            T = h.shape[1]
            if T > 1:
                o1, _, _ = m.step_chunk(h[:, :-1], ca, sa)
            cb, sb = ca.clone(), sa.clone()
            o2, _, _ = m.step_chunk(h[:, -1:], cb, sb)
            ref = torch.cat((o1, o2), dim=1) if T > 1 else o2
        else:
            body, last, at = [], [], 0
            for n in seq_map.lens:
                body += list(range(at, at + n - 1))
                last += [at + n - 1] if n else []
                at += n
            ref = torch.zeros_like(out)
            if body:
                mb = aum_hip.seq_map([max(n - 1, 0) for n in seq_map.lens], seq_map.rows, device=device)
                ref[0, body] = m.step_chunk(h[:, body], ca, sa, seq_map=mb)[0][0]
            cb, sb = ca.clone(), sa.clone()
            ml = aum_hip.seq_map([min(n, 1) for n in seq_map.lens], seq_map.rows, device=device)
            ref[0, last] = m.step_chunk(h[:, last], cb, sb, seq_map=ml)[0][0]
    e_out = rel_err(_np(out), _np(ref))
    e_c, e_s = rel_err(_np(c), _np(ca)), rel_err(_np(s), _np(sa))
    print(f"step_chunk(peek=True) vs two calls: out {e_out:.3e} (bar {bar:.0e}), conv cache {e_c:.3e}, ssm cache {e_s:.3e} (bar {cache_bar:.0e}), "
          f"caches bit-equal: {torch.equal(c, ca) and torch.equal(s, sa)}")
    assert e_out < bar
    if exact_caches and torch.equal(c, ca) and torch.equal(s, sa):
        return
    assert e_c < cache_bar and e_s < cache_bar
    assert not torch.equal(s, s0)


# ---- model -------------------------------------------------------------------------------------------------------------------------
HOPS = (1, 1, 2, 4, 8)


def _ctx(device, autocast_dtype):
    if autocast_dtype is None:
        return contextlib.nullcontext
    return lambda: torch.autocast(device_type=torch.device(device).type, dtype=autocast_dtype)


def _cache_err(a, b):
    return max(max(rel_err(_np(c1), _np(c2)), rel_err(_np(s1), _np(s2))) for (c1, s1), (c2, s2) in zip(a["layers"].values(), b["layers"].values()))


def check_model_push_read(embed_dim, device, autocast_dtype=None):
    """every stream_push(read=True) returns the column count of a plain push and the logits stream_read gives on a twin cache advanced
    by plain pushes; after the last hop the logits are model(spec)'s; the two sessions' caches agree"""
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(11)
    spec = torch.randn(2, 256, 128, device=device)
    bar = 1e-4 if autocast_dtype is None else 2e-2
    with torch.no_grad(), _ctx(device, autocast_dtype)():
        full = model(spec)
        cache, twin = model.allocate_inference_cache(2), model.allocate_inference_cache(2)
        col = 0
        for k in HOPS:
            piece = spec[:, 16 * col:16 * (col + k)]
            cols, logits = model.stream_push(piece, cache, read=True)
            assert cols == model.stream_push(piece, twin) == col + k == cache["columns"]
            want = model.stream_read(twin)
            col += k
            e = rel_err(_np(logits), _np(want))
            print(f"push(read=True) at column {col}: logits vs push + stream_read {e:.3e} (bar {bar:.0e})")
            assert logits.shape == want.shape == (2, 7)
            assert e < bar
        feats = model.stream_read(twin, return_features=True)
        e_full, e_cache = rel_err(_np(logits), _np(full)), _cache_err(cache, twin)
        print(f"last push(read=True) vs model(spec) {e_full:.3e}, caches vs plain pushes {e_cache:.3e} (bar {bar:.0e})")
        assert e_full < bar and e_cache < bar
        # the features form, on fresh caches: the whole clip in one hop -- 128 tokens and the peek row, one row more than the one-launch path takes
        c2 = model.allocate_inference_cache(2)
        cols, f = model.stream_push(spec, c2, read=True, return_features=True)
        assert cols == 16 and f.shape == feats.shape and rel_err(_np(f), _np(feats)) < bar


def check_model_push_many_read(embed_dim, device, autocast_dtype=None):
    """two sessions at different offsets with different hop sizes in a pool of 4, read=True: each session's logits against the same
    session served alone (stream_push + stream_read on a cache of its own), in the order of `sessions`"""
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
        for ka, kb in ((1, 2), (2, 1), (4, 3), (8, 2)):
            pieces = [spec[0, 16 * at[0]:16 * (at[0] + ka)], spec[1, 16 * at[1]:16 * (at[1] + kb)]]
            cols, logits = model.stream_push_many(pieces, pool, sessions, read=True)
            at = [at[0] + ka, at[1] + kb]
            assert cols == at and [pool["columns"][r] for r in sessions] == at
            assert logits.shape == (2, 7)
            for i, piece in enumerate(pieces):
                model.stream_push(piece.unsqueeze(0), alone[i])
                want = model.stream_read(alone[i])
                e = rel_err(_np(logits[i:i + 1]), _np(want))
                print(f"push_many(read=True) session {sessions[i]} at column {at[i]}: vs served alone {e:.3e} (bar {bar:.0e})")
                assert e < bar
        assert at[0] == 15
        for i, r in enumerate(sessions):
            for (pc, ps), (ac, as_) in zip(pool["layers"].values(), alone[i]["layers"].values()):
                assert rel_err(_np(pc[r]), _np(ac[0])) < bar and rel_err(_np(ps[r]), _np(as_[0])) < bar
        for pc, ps in pool["layers"].values():                  # rows no session owns
            assert not pc[1].any() and not pc[3].any() and not ps[1].any() and not ps[3].any()
        feats = model.stream_push_many([spec[0, 240:]], pool, [2], read=True, return_features=True)[1]
        assert feats.shape == (1, embed_dim)
        e = rel_err(_np(model.head(feats)), _np(model(spec[:1])))
        print(f"push_many(read=True) last column, features -> head vs model(spec): {e:.3e} (bar {bar:.0e})")
        assert e < bar


def check_model_read_refusals(device):
    """calls that fail the existing argument checks, with read=True, leave caches and column counts as they were"""
    model = make_causal_aum(64, device, depth=2)
    torch.manual_seed(13)
    spec = torch.randn(1, 256, 128, device=device)
    with torch.no_grad():
        cache, pool = model.allocate_inference_cache(1), model.allocate_stream_pool(3)
        model.stream_push(spec[:, :32], cache, read=True)
        model.stream_push_many([spec[0, :32]], pool, [1], read=True)
        snap = lambda cch: [(c.clone(), s.clone()) for c, s in cch["layers"].values()]
        same = lambda cch, sn: all(torch.equal(c, c1) and torch.equal(s, s1) for (c, s), (c1, s1) in zip(cch["layers"].values(), sn))
        s_cache, s_pool = snap(cache), snap(pool)
        for bad in (spec[:, :24], spec[:, :0], spec[:, :32, :64], spec[0, :32], spec.expand(2, -1, -1)[:, :32], spec[:, :240]):
            with pytest.raises(ValueError):
                model.stream_push(bad, cache, read=True)
        with pytest.raises(ValueError, match="stream_push_many"):
            model.stream_push(spec[:, :32], pool, read=True)
        for args in (([spec[0, :24]], [1]), ([spec[0, :32], spec[0, :32]], [1, 1]), ([spec[0, :32]], [3]), ([spec[0, :32]], [1, 2]),
                     ([spec[0, :240]], [1]), ([], [])):
            with pytest.raises(ValueError):
                model.stream_push_many(args[0], pool, args[1], read=True)
        with pytest.raises(ValueError, match="pool"):
            model.stream_push_many([spec[0, :32]], cache, [0], read=True)
        assert cache["columns"] == 2 and pool["columns"] == [0, 2, 0]
        assert same(cache, s_cache) and same(pool, s_pool)
