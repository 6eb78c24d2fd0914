"""Shared bodies of the park / resume tests (aum_stream_park, aum_hip.stream_park / stream_park_layout, AudioMamba.stream_park /
stream_resume / stream_fork): tests/test_stream_park.py runs them on the lane-array build with host tensors, tests/test_gpu_stream_park.py
on the device library.  Every comparison is torch.equal on bit patterns: the feature moves bytes and has no tolerance.  The expected
values never come from the code under test: an uninterrupted session on a pool of its own, the pools' own bytes before the call, and
plain indexed copies."""
import contextlib
import ctypes as C

import pytest
import torch

import aum_hip
import stream_checks as sc
from stream_prefill_checks import product_lib


def bits(t):
    """the bytes of a tensor (of contiguous memory) as they are"""
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t.contiguous()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def nan_bytes(n, device, salt=0):
    """n bytes (a multiple of 4) of NaN words whose payload counts up: no two 16-byte pieces alike"""
    w = (torch.arange(n // 4, dtype=torch.int64) + salt * 7919) % (1 << 20) + 0x7FC00000
    return w.to(torch.int32).view(torch.uint8).to(device)


def counting_bytes(n, device, salt):
    g = torch.Generator().manual_seed(1000 + salt)
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(device)


# ---- 1: the kernel, raw ------------------------------------------------------------------------------
ROW_BYTES = (16, 4112, 24576)           # one lane; one chunk and a 16-byte tail; AuM-Tiny's ssm_state row (six whole chunks)
ROW_STRIDES = (48, 4112 + 64, 24576 + 4096)
BLOB_OFFS = (32, 96, 96 + 4112 + 48)    # 16-byte multiples with padding in front, between and behind
RECORD = (BLOB_OFFS[2] + ROW_BYTES[2] + 255) // 256 * 256 + 256
POOL_ROWS = 5


def _raw_pools(device, fill):
    """three byte pools of POOL_ROWS strided rows"""
    return [fill(POOL_ROWS * st, device, 10 + i) for i, st in enumerate(ROW_STRIDES)]


def _raw_args(pools, rows_t, blob_t, n, restore, **over):
    a = aum_hip.ParkArgs()
    for t, p in enumerate(pools):
        a.base[t], a.row_stride[t], a.row_bytes[t], a.blob_off[t] = p.data_ptr(), ROW_STRIDES[t], ROW_BYTES[t], BLOB_OFFS[t]
    a.rows, a.blob, a.blob_stride = rows_t.data_ptr(), blob_t.data_ptr(), RECORD
    a.n_tensors, a.n_sessions, a.flags = len(pools), n, aum_hip.PARK_RESTORE if restore else 0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _call(lib, a, like):
    rc = lib.c.aum_stream_park(C.byref(a), lib.stream(like))
    if like.device.type == "cuda":
        torch.cuda.synchronize()
    return rc


def check_kernel_raw(lib, device):
    """park rows [3, 0] of three strided pools into a NaN-filled blob with a sentinel record behind it, restore them into rows [1, 4] of
    NaN-filled pools; only the named bytes move.  Then one session, and the refusals -- each leaves every byte as it was and is refused
    by the Python mirror as well."""
    rows, dst = [3, 0], [1, 4]
    rows_t = torch.tensor(rows, dtype=torch.int32).to(device)
    dst_t = torch.tensor(dst, dtype=torch.int32).to(device)
    pools = _raw_pools(device, counting_bytes)
    pools0 = [p.clone() for p in pools]
    blob = nan_bytes(3 * RECORD, device).reshape(3, RECORD)
    blob0 = blob.clone()
    a = _raw_args(pools, rows_t, blob, 2, False)
    assert aum_hip.stream_park_args_ok(a) and _call(lib, a, blob) == 0
    assert all(torch.equal(p, p0) for p, p0 in zip(pools, pools0)), "parking wrote to a pool"
    expect = blob0.clone()
    for i, r in enumerate(rows):
        for p0, st, nb, off in zip(pools0, ROW_STRIDES, ROW_BYTES, BLOB_OFFS):
            expect[i, off:off + nb] = p0[r * st:r * st + nb]
    assert torch.equal(blob[:2], expect[:2]), "records differ from the named rows, or the padding between the ranges was written"
    assert torch.equal(blob[2], blob0[2]), "the sentinel record behind the blob was written"
    # restore into rows [1, 4] of NaN-filled pools
    back = _raw_pools(device, nan_bytes)
    back0 = [p.clone() for p in back]
    a = _raw_args(back, dst_t, blob, 2, True)
    assert aum_hip.stream_park_args_ok(a) and _call(lib, a, blob) == 0
    assert torch.equal(blob, expect), "restoring wrote to the blob"
    for p, p0, src0, st, nb in zip(back, back0, pools0, ROW_STRIDES, ROW_BYTES):
        want = p0.clone()
        for r_from, r_to in zip(rows, dst):
            want[r_to * st:r_to * st + nb] = src0[r_from * st:r_from * st + nb]
        assert torch.equal(p, want), f"rows of {nb} bytes: a byte outside the named rows' row_bytes changed, or the rows differ"
    # one session; and every session from ONE record (blob_stride 0, restore only)
    one = nan_bytes(RECORD, device, 3).reshape(1, RECORD)
    a = _raw_args(pools, rows_t[1:], one, 1, False)
    assert aum_hip.stream_park_args_ok(a) and _call(lib, a, one) == 0
    assert torch.equal(one[0, BLOB_OFFS[1]:BLOB_OFFS[1] + ROW_BYTES[1]], pools0[1][0:ROW_BYTES[1]])
    assert torch.equal(one[0, :BLOB_OFFS[0]], nan_bytes(RECORD, device, 3)[:BLOB_OFFS[0]])
    both = _raw_pools(device, nan_bytes)
    a = _raw_args(both, dst_t, one, 2, True, blob_stride=0)
    assert aum_hip.stream_park_args_ok(a) and _call(lib, a, one) == 0
    for p, st, nb, off in zip(both, ROW_STRIDES, ROW_BYTES, BLOB_OFFS):
        assert all(torch.equal(p[r * st:r * st + nb], one[0, off:off + nb]) for r in dst)
    # refusals: nothing is written, and the mirror says the same
    blob.copy_(blob0)
    snap = [p.clone() for p in pools]
    many = aum_hip.ParkArgs()
    for t in range(aum_hip.PARK_MAX_TENSORS):
        many.base[t], many.row_stride[t], many.row_bytes[t], many.blob_off[t] = pools[0].data_ptr(), 48, 16, 16 * t
    many.rows, many.blob, many.blob_stride, many.n_tensors, many.n_sessions = rows_t.data_ptr(), blob.data_ptr(), RECORD, 64, 2
    assert aum_hip.stream_park_args_ok(many)                 # 64 tensors are taken (not launched here: the ranges are made up) ...
    many.n_tensors = 65                                       # ... 65 are not
    for a, code in ((_raw_args(pools, rows_t, blob, 2, False, blob_off=(1, BLOB_OFFS[1] + 8)), -4), (many, -4),
                    (_raw_args(pools, rows_t, blob, 0, False), -4), (_raw_args(pools, rows_t, blob, 2, False, n_tensors=0), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, base=(2, pools[2].data_ptr() + 4)), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, row_stride=(1, ROW_STRIDES[1] + 8)), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, row_bytes=(1, ROW_BYTES[1] + 8)), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, row_stride=(2, ROW_BYTES[2] - 16)), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, blob_off=(2, BLOB_OFFS[1] + ROW_BYTES[1] - 16)), -4),      # ranges overlap
                    (_raw_args(pools, rows_t, blob, 2, False, blob_stride=BLOB_OFFS[2] + ROW_BYTES[2] - 16), -4),       # record too short
                    (_raw_args(pools, rows_t, blob, 2, False, blob_stride=0), -4),                                      # one record: restore only
                    (_raw_args(pools, rows_t, blob, 2, False, blob=blob.data_ptr() + 8), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, rows=rows_t.data_ptr() + 2), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, flags=2), -4),
                    (_raw_args(pools, rows_t, blob, 2, False, rows=None), -1), (_raw_args(pools, rows_t, blob, 2, False, blob=None), -1),
                    (_raw_args(pools, rows_t, blob, 2, False, base=(1, None)), -1)):
        assert not aum_hip.stream_park_args_ok(a)
        assert _call(lib, a, blob) == code
        if a.blob_stride:                                    # the other direction refuses the same (one record for all is its own rule)
            a.flags |= aum_hip.PARK_RESTORE
            assert not aum_hip.stream_park_args_ok(a) and _call(lib, a, blob) == code
    assert lib.c.aum_stream_park(None, None) == -1
    assert torch.equal(blob, blob0) and all(torch.equal(p, q) for p, q in zip(pools, snap))


def check_binding(lib, device):
    """aum_hip.stream_park on strided pool tensors of several dtypes = indexed copies; the layout; refused calls change nothing"""
    torch.manual_seed(5)
    big = [torch.randn(POOL_ROWS, 2, 6, 4, device=device), torch.randn(POOL_ROWS, 1028 + 4, device=device).to(torch.bfloat16),
           torch.randn(POOL_ROWS, 384, 16, device=device)]
    # rows of 96 bytes at a stride of 192, of 2048 bytes at a stride of 2064, of 24 576 bytes back to back
    tensors = [big[0][:, 0], big[1].as_strided((POOL_ROWS, 1024), (1032, 1)), big[2]]
    lay = aum_hip.stream_park_layout(tensors)
    assert lay.row_bytes == (96, 2048, 24576) and lay.offsets == (0, 96, 2144) and lay.record == 26880 and lay.record % 256 == 0
    big0 = [b.clone() for b in big]
    blob = aum_hip.stream_park(tensors, [3, 0], lib=lib)
    assert blob.shape == (2, lay.record) and blob.dtype == torch.uint8 and all(torch.equal(bits(b), bits(b0)) for b, b0 in zip(big, big0))
    for i, r in enumerate([3, 0]):
        for t, off, nb in zip(tensors, lay.offsets, lay.row_bytes):
            assert torch.equal(blob[i, off:off + nb], bits(t[r]).reshape(-1))
        assert not blob[i, lay.offsets[-1] + lay.row_bytes[-1]:].any()     # the padding of a fresh blob is zero
    other = [torch.zeros_like(b) for b in big]
    views = [other[0][:, 0], other[1].as_strided((POOL_ROWS, 1024), (1032, 1)), other[2]]
    aum_hip.stream_park(views, aum_hip.row_map([1, 4], device=device), blob, restore=True, lib=lib)
    for v, t in zip(views, tensors):
        assert same(v[1], t[3]) and same(v[4], t[0]) and not bits(v[0]).any() and not bits(v[2]).any() and not bits(v[3]).any()
    assert not bits(other[0][:, 1]).any() and not bits(other[1][:, 1024:]).any()        # what lies between the strided rows
    # refusals
    snap = [bits(o).clone() for o in other]
    for call, exc in ((lambda: aum_hip.stream_park(views, [1, 1], blob, restore=True, lib=lib), ValueError),
                      (lambda: aum_hip.stream_park(views, [1, POOL_ROWS], blob, restore=True, lib=lib), ValueError),
                      (lambda: aum_hip.stream_park(views, [], blob, restore=True, lib=lib), ValueError),
                      (lambda: aum_hip.stream_park(views, [1, 4], blob[:, :-256], restore=True, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park(views, [1, 4], blob[:1], restore=True, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park(views, [1, 4], None, restore=True, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park(views, [1, 4], blob.view(torch.int8), restore=True, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park([other[2].transpose(1, 2)], [1], None, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park([other[2][:, :, :3]], [1], None, lib=lib), RuntimeError),       # rows not contiguous
                      (lambda: aum_hip.stream_park([torch.zeros(POOL_ROWS, 6, device=device)], [1], None, lib=lib), RuntimeError),   # 24-byte rows
                      (lambda: aum_hip.stream_park([other[2], other[2][:4]], [1], None, lib=lib), RuntimeError),
                      (lambda: aum_hip.stream_park([other[2]] * 65, [1], None, lib=lib), RuntimeError)):
        with pytest.raises(exc):
            call()
    assert all(torch.equal(bits(o), s) for o, s in zip(other, snap))


# ---- the model ---------------------------------------------------------------------------------------
def tiny_clip_model(device, depth=2, **over):
    """bimamba 'none', end cls, time-major, depth 2, embed_dim 192, 128 x 128 spectrograms: 8 time columns, the smallest clip"""
    return sc.make_causal_aum(192, device, depth=depth, spectrogram_size=(128, 128), **over)


def clip(seed, device, batch=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((128, 128) if batch is None else (batch, 128, 128), generator=g).to(device)


def pool_bits(pool, ws=None):
    out = [bits(t).clone() for i in sorted(pool["layers"]) for t in pool["layers"][i]] + [list(pool["columns"]) if isinstance(pool["columns"], list)
                                                                                         else pool["columns"]]
    if ws is not None:
        out += [ws.tails.clone(), list(ws.tail_len), list(ws.samples), list(ws.frames), list(ws.ended)]
    return out


def pools_same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def row_same(pool_a, ra, pool_b, rb):
    return all(same(ta[ra], tb[rb]) for i in pool_a["layers"] for ta, tb in zip(pool_a["layers"][i], pool_b["layers"][i]))


def _autocast(device, dtype):
    return contextlib.nullcontext() if dtype is None else torch.autocast(device_type=torch.device(device).type, dtype=dtype)


def check_continuation(lib, device, autocast_dtype=None, to_host=False):
    """2: A pushed 3 columns in row 2 of P, parked, reset, the row advanced by another clip; A resumed in row 0 of Q and pushed the other
    5 columns with read=True: logits of every hop and the final caches = an uninterrupted session's, bit for bit"""
    with torch.no_grad(), product_lib(lib), _autocast(device, autocast_dtype):
        model = tiny_clip_model(device)
        a, other = clip(1, device), clip(2, device)
        U = model.allocate_stream_pool(1)                                   # the uninterrupted session
        ref = [model.stream_push_many([a[:48]], U, [0], read=True)[1]]
        P, Q = model.allocate_stream_pool(4), model.allocate_stream_pool(3)
        model.stream_push_many([other[:32], other[:16]], P, [0, 3])          # neighbours at other positions
        _, lg = model.stream_push_many([a[:48]], P, [2], read=True)
        assert torch.equal(lg, ref[0])
        state = model.stream_park(P, [2], to_host=to_host)
        assert len(state) == 1 and state.columns == [3] and state.blob.dtype == torch.uint8 and state.blob.shape[1] % 256 == 0
        assert state.blob.device.type == ("cpu" if to_host else torch.device(device).type)
        if to_host and torch.device(device).type == "cuda":
            assert state.blob.is_pinned()
        model.stream_reset(P, [2])
        model.stream_push_many([other[:64]], P, [2])                         # stale state in the old row would show
        model.stream_push_many([other[16:48]], Q, [0])                       # and what the new row held is overwritten
        model.stream_resume(state, Q, [0])
        assert Q["columns"] == [3, 0, 0] and row_same(Q, 0, U, 0)
        for c0, c1 in ((3, 4), (4, 6), (6, 8)):
            ref.append(model.stream_push_many([a[16 * c0:16 * c1]], U, [0], read=True)[1])
            counts, lg = model.stream_push_many([a[16 * c0:16 * c1]], Q, [0], read=True)
            assert counts == [c1] and torch.equal(lg, ref[-1]), f"logits after column {c1} differ from the uninterrupted session"
        assert row_same(Q, 0, U, 0), "final caches differ from the uninterrupted session"


def check_neighbours(lib, device):
    """3: parking or resuming sessions [3, 1] of a 4-row pool leaves rows 0 and 2 of every layer, and their counts, as they were"""
    with torch.no_grad(), product_lib(lib):
        model = tiny_clip_model(device)
        x = clip(3, device, batch=4)
        P, Q = model.allocate_stream_pool(4), model.allocate_stream_pool(4)
        model.stream_push_many([x[0, :16], x[1, :32], x[2, :48], x[3, :64]], P, [0, 1, 2, 3])
        model.stream_push_many([x[3, :16], x[2, :32], x[1, :48], x[0, :64]], Q, [0, 1, 2, 3])
        p0, q0 = pool_bits(P), pool_bits(Q)
        state = model.stream_park(P, [3, 1])
        assert pools_same(pool_bits(P), p0), "parking changed the pool"
        assert state.columns == [4, 2] and state[1].columns == [2] and state.select([1, 0]).columns == [2, 4]
        assert torch.equal(state.select([1, 0]).blob, state.blob.flip(0)) and torch.equal(state[0].blob, state.blob[:1])
        model.stream_resume(state, Q, [3, 1])
        q1 = pool_bits(Q)
        for i in Q["layers"]:
            for t, before in zip(Q["layers"][i], (q0[2 * i], q0[2 * i + 1])):
                now = bits(t)
                assert torch.equal(now[0], before[0]) and torch.equal(now[2], before[2]), f"layer {i}: a neighbour's row changed"
        assert Q["columns"] == [1, 2, 3, 4] and row_same(Q, 3, P, 3) and row_same(Q, 1, P, 1)
        model.stream_resume(state.select([1, 0]), Q, [0, 2])                 # split and reordered: session 1 to row 0, session 3 to row 2
        assert Q["columns"] == [2, 2, 4, 4] and row_same(Q, 0, P, 1) and row_same(Q, 2, P, 3) and row_same(Q, 3, P, 3)
        # fixed-batch caches are pools of `batch` rows
        Cc = model.allocate_inference_cache(2)
        model.stream_push(x[:2, :32], Cc)
        st = model.stream_park(Cc, [1, 0])
        assert st.columns == [2, 2]
        D = model.allocate_inference_cache(2)
        model.stream_resume(st, D, [0, 1])
        assert D["columns"] == 2 and row_same(D, 0, Cc, 1) and row_same(D, 1, Cc, 0)
        d0 = pool_bits(D)
        with pytest.raises(ValueError, match="one column count"):
            model.stream_resume(state[0], D, [1])                            # a session at 4 columns into a cache at 2
        assert pools_same(pool_bits(D), d0)
        model.stream_resume(state[1], D, [1])                                # at 2 columns: fits
        assert row_same(D, 1, P, 1)


def check_fork(lib, device):
    """4: fork 1 -> [0, 3]; the same column into 0, 1, 3 gives three equal logit rows; different columns into 0 and 3 leave row 1 alone"""
    with torch.no_grad(), product_lib(lib):
        model = tiny_clip_model(device)
        x = clip(4, device, batch=3)
        P = model.allocate_stream_pool(4)
        model.stream_push_many([x[0, :48], x[1, :16]], P, [1, 2])
        before = pool_bits(P)
        model.stream_fork(P, src=1, dst=[0, 3])
        assert P["columns"] == [3, 3, 1, 3] and row_same(P, 0, P, 1) and row_same(P, 3, P, 1)
        after = pool_bits(P)
        for k, (b, a) in enumerate(zip(before[:-1], after[:-1])):
            assert torch.equal(b[1], a[1]) and torch.equal(b[2], a[2]), "the fork changed its source or a neighbour"
        col = x[0, 48:64]
        counts, lg = model.stream_push_many([col, col, col], P, [0, 1, 3], read=True)
        assert counts == [4, 4, 4] and torch.equal(lg[0], lg[1]) and torch.equal(lg[2], lg[1])
        one = pool_bits(P)
        model.stream_push_many([x[1, 64:80], x[2, 64:80]], P, [0, 3])
        two = pool_bits(P)
        assert all(torch.equal(a[1], b[1]) for a, b in zip(one[:-1], two[:-1])) and P["columns"] == [5, 4, 1, 5]
        assert not row_same(P, 0, P, 3)
        snap = pool_bits(P)
        for kw in ({"src": 1, "dst": [1, 2]}, {"src": 1, "dst": [2, 2]}, {"src": 4, "dst": [0]}, {"src": 1, "dst": []}, {"src": 1, "dst": [0, 4]}):
            with pytest.raises(ValueError):
                model.stream_fork(P, **kw)
        assert pools_same(pool_bits(P), snap)


def check_wave(lib, device):
    """5: raw audio in hops of 1000 and 777 samples (no whole column: the tail is what the session is), parked with its wave stream,
    resumed in another pool and stream on another row, streamed to the end: the logits of the uninterrupted stream, bit for bit"""
    import stream_wave_checks as wc
    with torch.no_grad(), product_lib(lib):
        model, fe = wc.make(device)
        w = wc.clip_wave(81).to(device)
        other = wc.clip_wave(82).to(device)
        cuts = [1000, 777, 2900, 9000]

        def stream(pool, ws, row, start, wave=w):
            at, out = sum(cuts[:start]), []
            for m in cuts[start:]:
                out.append(model.stream_push_wave_many([wave[at:at + m]], pool, ws, [row], read=True)[1])
                at += m
            out.append(model.stream_push_wave_many([wave[at:]], pool, ws, [row], read=True, end=True)[1])
            return out
        U, wu = model.allocate_stream_pool(1), model.allocate_wave_stream(1, fe)
        ref = stream(U, wu, 0, 0)
        P, wp = model.allocate_stream_pool(3), model.allocate_wave_stream(3, fe)
        Q, wq = model.allocate_stream_pool(4), model.allocate_wave_stream(4, fe)
        model.stream_push_wave_many([other[:5000]], P, wp, [0])
        model.stream_push_wave_many([other[:7000]], Q, wq, [3])               # the row A will land on holds another clip's tail
        got = [model.stream_push_wave_many([w[:1000]], P, wp, [1], read=True)[1], model.stream_push_wave_many([w[1000:1777]], P, wp, [1], read=True)[1]]
        assert wp.tail_len[1] == 1777 and wp.frames[1] == 0 and P["columns"][1] == 0          # nothing but a tail so far
        p0 = pool_bits(P, wp)
        state = model.stream_park(P, [1], wave_stream=wp)
        assert pools_same(pool_bits(P, wp), p0)
        assert state.wave == {"tail_len": [1777], "samples": [1777], "frames": [0], "ended": [False]} and state.signature[-1] == wc.CAP
        model.stream_reset(P, [1])
        wp.reset([1])
        model.stream_push_wave_many([other[:4000]], P, wp, [1])
        q0 = pool_bits(Q, wq)
        with pytest.raises(ValueError, match="layout"):
            model.stream_resume(state, Q, [3])                                # parked with a tail, resumed without a wave stream
        assert pools_same(pool_bits(Q, wq), q0)
        model.stream_resume(state, Q, [3], wave_stream=wq)
        assert (wq.tail_len[3], wq.samples[3], wq.frames[3], wq.ended[3]) == (1777, 1777, 0, False) and Q["columns"][3] == 0
        assert torch.equal(wq.tails[3, :1777], w[:1777]) and torch.equal(wq.tails[:3], q0[-5][:3])
        got += stream(Q, wq, 3, 2)
        assert len(got) == len(ref) == 5 and all(torch.equal(g, r) for g, r in zip(got, ref))
        assert row_same(Q, 3, U, 0)
        # fork with the wave stream: the copy streams on as its source does
        model.stream_reset(Q, [0, 1])
        wq.reset([0, 1])
        model.stream_push_wave_many([w[:3500]], Q, wq, [0])
        model.stream_fork(Q, src=0, dst=[1], wave_stream=wq)
        _, lg = model.stream_push_wave_many([w[3500:9000], w[3500:9000]], Q, wq, [0, 1], read=True)
        assert torch.equal(lg[0], lg[1]) and wq.tail_len[0] == wq.tail_len[1] and Q["columns"][0] == Q["columns"][1]


def check_refusals(lib, device):
    """6: another depth, duplicate rows, a row outside the pool, a blob of another record size (and the rest): refused, pools unchanged"""
    from aum.model import ParkedSessions
    with torch.no_grad(), product_lib(lib):
        model, deeper = tiny_clip_model(device), tiny_clip_model(device, depth=3)
        x = clip(6, device, batch=3)
        P, Q, R = model.allocate_stream_pool(4), model.allocate_stream_pool(3), deeper.allocate_stream_pool(3)
        model.stream_push_many([x[0, :32], x[1, :48]], P, [1, 3])
        model.stream_push_many([x[2, :16]], Q, [1])
        deeper.stream_push_many([x[2, :16]], R, [1])
        state = model.stream_park(P, [1, 3])
        snaps = [pool_bits(c) for c in (P, Q, R)]
        short = ParkedSessions(state.blob[:, :-256], state.columns, None, state.signature)
        other_dtype = model.allocate_stream_pool(3, dtype=torch.bfloat16)
        for call, exc, msg in (
                (lambda: deeper.stream_resume(state, R, [0, 2]), ValueError, "layout"),                 # depth 2 against depth 3
                (lambda: model.stream_resume(state, Q, [2, 2]), ValueError, "not distinct"),
                (lambda: model.stream_resume(state, Q, [0, 3]), ValueError, "not all rows"),
                (lambda: model.stream_resume(state, Q, [0, -1]), ValueError, "not all rows"),
                (lambda: model.stream_resume(short, Q, [0, 2]), ValueError, "blob"),                    # a blob of another record size
                (lambda: model.stream_resume(state, Q, [0]), ValueError, "parked sessions"),
                (lambda: model.stream_resume(state, Q, []), ValueError, "at least one"),
                (lambda: model.stream_resume(state, other_dtype, [0, 2]), ValueError, "layout"),
                (lambda: model.stream_resume({"blob": state.blob}, Q, [0, 2]), TypeError, "stream_park"),
                (lambda: model.stream_park(P, [1, 1]), ValueError, "not distinct"),
                (lambda: model.stream_park(P, [4]), ValueError, "not all rows"),
                (lambda: model.stream_park(P, []), ValueError, "at least one"),
                (lambda: model.stream_park(P, [1], wave_stream={"tails": None}), TypeError, "allocate_wave_stream"),
                (lambda: state.select([2]), IndexError, "select")):
            with pytest.raises(exc, match=msg):
                call()
            assert all(pools_same(pool_bits(c), s) for c, s in zip((P, Q, R), snaps)), msg
        assert not other_dtype["layers"][0][1].any() and other_dtype["columns"] == [0, 0, 0]


class count_calls:
    """counts the calls of aum_hip.<name> inside the block (tests/xdt_tiny_checks.py: how 'one aum_hip.stream_block call' is shown)"""

    def __init__(self, *names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        self.orig = {k: getattr(aum_hip, k) for k in self.names}
        for k in self.names:
            def wrap(*a, _k=k, **kw):
                self.n[_k] += 1
                return self.orig[_k](*a, **kw)
            setattr(aum_hip, k, wrap)
        return self.n

    def __exit__(self, *a):
        for k, v in self.orig.items():
            setattr(aum_hip, k, v)


@contextlib.contextmanager
def count_entry(lib):
    """counts the calls of the C entry point itself, and of the un-fused twin (the only code of the feature that indexes the caches)"""
    from aum.model import AudioMamba
    n = {"aum_stream_park": 0, "copies": 0}
    real, twin = lib.c.aum_stream_park, AudioMamba._park_copies

    def entry(*a):
        n["aum_stream_park"] += 1
        return real(*a)

    def copies(*a, **kw):
        n["copies"] += 1
        return twin(*a, **kw)
    lib.c.aum_stream_park, AudioMamba._park_copies = entry, staticmethod(copies)
    try:
        yield n
    finally:
        lib.c.aum_stream_park, AudioMamba._park_copies = real, staticmethod(twin)


def check_one_launch(lib, device):
    """7: stream_park and stream_resume of a depth-2 model are one aum_hip.stream_park call = one aum_stream_park each, whatever the
    number of sessions, and the indexed copies of the twin do not run; a fork is two"""
    with torch.no_grad(), product_lib(lib):
        model = tiny_clip_model(device)
        x = clip(7, device, batch=3)
        P, Q = model.allocate_stream_pool(4), model.allocate_stream_pool(4)
        model.stream_push_many([x[0, :32], x[1, :48], x[2, :16]], P, [1, 3, 0])
        with count_calls("stream_park") as n, count_entry(lib) as c:
            state = model.stream_park(P, [1, 3, 0])
            assert n == {"stream_park": 1} and c == {"aum_stream_park": 1, "copies": 0}, (n, c)
            model.stream_resume(state, Q, [0, 2, 3])
            assert n == {"stream_park": 2} and c == {"aum_stream_park": 2, "copies": 0}, (n, c)
            model.stream_fork(Q, src=0, dst=[1])
            assert n == {"stream_park": 4} and c == {"aum_stream_park": 4, "copies": 0}, (n, c)
            host = model.stream_park(P, [3], to_host=True)
            model.stream_resume(host, Q, [1])
            assert n == {"stream_park": 6} and c == {"aum_stream_park": 6, "copies": 0}, (n, c)
        assert row_same(Q, 0, P, 1) and row_same(Q, 2, P, 3) and row_same(Q, 3, P, 0) and row_same(Q, 1, P, 3)


def check_twin(lib):
    """8: on CPU tensors the indexed copies give the ParkedSessions the kernel path of the host build gives, byte for byte, and resume
    the same pools"""
    import stream_wave_checks as wc
    from aum.model import AudioMamba
    with torch.no_grad(), product_lib(lib):
        model, fe = wc.make("cpu")
        w = wc.clip_wave(91)
        P, wp = model.allocate_stream_pool(4), model.allocate_wave_stream(4, fe)
        model.stream_push_wave_many([w[:6000], w[100:3000], w[:9999]], P, wp, [2, 0, 3])
        with count_entry(lib) as c:
            fused = model.stream_park(P, [3, 0, 2], wave_stream=wp)
            assert c == {"aum_stream_park": 1, "copies": 0}
        old, aum_hip._product = aum_hip._product, None                      # no host-pointer library: the twin
        try:
            with count_entry(lib) as c:
                plain = model.stream_park(P, [3, 0, 2], wave_stream=wp)
                assert c == {"aum_stream_park": 0, "copies": 1}
            Q, wq = model.allocate_stream_pool(4), model.allocate_wave_stream(4, fe)
            model.stream_resume(fused, Q, [1, 2, 0], wave_stream=wq)          # kernel-made records through the copies
        finally:
            aum_hip._product = old
        assert torch.equal(fused.blob, plain.blob) and fused.columns == plain.columns and fused.wave == plain.wave
        assert fused.signature == plain.signature and fused.blob.shape == (3, aum_hip.stream_park_layout(AudioMamba._park_tensors(model, P, wp)).record)
        Q2, wq2 = model.allocate_stream_pool(4), model.allocate_wave_stream(4, fe)
        model.stream_resume(plain, Q2, [1, 2, 0], wave_stream=wq2)            # copy-made records through the kernel
        assert pools_same(pool_bits(Q, wq), pool_bits(Q2, wq2))
        assert row_same(Q, 1, P, 3) and row_same(Q, 2, P, 0) and row_same(Q, 0, P, 2) and torch.equal(wq.tails[1], wp.tails[3])
