"""Shared bodies of the raw-audio streaming tests (aum_fbank_stream_fwd, aum_hip.fbank_stream / wave_map, AudioMamba.stream_push_wave*):
tests/test_stream_wave.py runs them on the lane-array build, tests/test_gpu_stream_wave.py on the device library.
Shapes: 128 mel bins, 16 kHz (win 400, shift 160), a clip grid of 16 columns = 256 frames = 41 200 samples, 3 sessions in a pool of 5."""
import pytest
import torch

import aum_hip
import stream_checks as sc
from conftest import rel_err

WIN, SHIFT, T, CAP, POOL = 400, 160, 256, 2800, 5
CLIP = WIN + (T - 1) * SHIFT                                  # 41 200
MEAN, STD = -4.2677393, 4.5689974
CANARY = 7.5

# every list sums to CLIP.  A: the hop sizes around the shift, the window overlap, a column and a tail row, an empty hop, a backlog of
# several columns; it opens with two hops that produce no frame.  B .. F put the tail / hop boundary where the docstring of
# check_any_cut says.
CUTS = {
    "A": [1, 159, 160, 161, 239, 240, 241, 2559, 2560, 2561, 2799, 2800, 2801, 0, 8000, 15919],
    "B": [1, 2799, 50, 60, 38290],
    "C": [2959, 2401, 0, 35840],
    "D": [2880, 2560, 35760],
    "E": [2800, 38400],
    "F": [CLIP],
}
assert all(sum(c) == CLIP for c in CUTS.values())


def tables(dev):
    from aum.frontend import FbankTables
    return FbankTables(dev)


def clip_wave(seed, n=CLIP):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 0.2


def host_plan(n_before, emitted, m, end):
    """the host formula: (frames of this push, n_real) of a session that holds n_before samples and has emitted `emitted` frames"""
    n = n_before + m
    avail = 0 if n < WIN else 1 + (n - WIN) // SHIFT
    return (T - emitted, avail) if end else ((avail - emitted) // 16 * 16, -1)


class KStream:
    """the host side of a stream at kernel level: a pool of tails filled with a canary, per row tail length / samples / frames"""

    def __init__(self, dev, lib):
        self.dev, self.lib, self.tabs = dev, lib, tables(dev)
        self.tails = torch.full((POOL, CAP), CANARY, device=dev)
        self.tl, self.n, self.fr = [0] * POOL, [0] * POOL, [0] * POOL
        self.log = []                                         # (row, tail_len before, m, frames) of every push of every session

    def push(self, hops, rows, ends=None):
        """hops[i]: (m_i,) new samples of row rows[i] -> [frames_i (f_i, 128)]"""
        ends = ends or [False] * len(rows)
        plans = [host_plan(self.n[r], self.fr[r], h.shape[0], e) for h, r, e in zip(hops, rows, ends)]
        wmap = aum_hip.wave_map([h.shape[0] for h in hops], [self.tl[r] for r in rows], [p[0] for p in plans], [self.fr[r] for r in rows],
                                [p[1] for p in plans], rows, device=self.dev)
        out = aum_hip.fbank_stream(torch.cat(hops) if len(hops) > 1 else hops[0], wmap, self.tails, self.tabs.tables, MEAN, STD, lib=self.lib)
        for i, r in enumerate(rows):
            self.log.append((r, self.tl[r], hops[i].shape[0], plans[i][0]))
            have = self.tl[r] + hops[i].shape[0]
            self.tl[r] = have - min(plans[i][0] * SHIFT, have)
            assert self.tl[r] == wmap.new_tail_lens[i]
            self.n[r] += hops[i].shape[0]
            self.fr[r] += plans[i][0]
        return list(out.split([p[0] for p in plans], dim=0))


def run_cuts(dev, lib, waves, cuts, rows, check_tails=True):
    """session i pushes waves[i] cut by cuts[i] on row rows[i]; a session is in a call while it has hops left.  Returns (frames per
    session, the KStream).  check_tails: after every push the row holds exactly the last tail_len samples pushed so far."""
    ks = KStream(dev, lib)
    got = [[] for _ in rows]
    at = [0] * len(rows)
    for step in range(max(len(c) for c in cuts)):
        live = [i for i in range(len(rows)) if step < len(cuts[i])]
        hops = [waves[i][at[i]:at[i] + cuts[i][step]] for i in live]
        outs = ks.push(hops, [rows[i] for i in live])
        for i, o in zip(live, outs):
            got[i].append(o)
            at[i] += cuts[i][step]
            if check_tails:
                r = rows[i]
                assert ks.tl[r] == (at[i] if at[i] < WIN else at[i] - ((at[i] - WIN) // SHIFT + 1) // 16 * 16 * SHIFT)
                assert torch.equal(ks.tails[r, :ks.tl[r]], waves[i][at[i] - ks.tl[r]:at[i]]), (r, step)
    return [torch.cat(g) for g in got], ks


def whole(dev, lib, wave, target=T):
    return aum_hip.fbank_fwd(wave[None].contiguous(), tables(dev).tables, target, MEAN, STD, lib=lib)[0]


def bits(t):
    return t.contiguous().view(torch.int32)


def check_any_cut(dev, lib):
    """1: frames streamed under any cut of the sample stream == the rows of fbank_fwd on the whole waveform, bit for bit.  The lists put
    the tail / hop boundary at frame offset 0 (no tail), at 1, inside the window, at win - 1 and exactly at the start of a later frame."""
    log = []
    for names, rows in ((("A", "B", "C"), [3, 0, 4]), (("D", "E", "F"), [1, 2, 0])):
        waves = [clip_wave(20 + ord(n)).to(dev) for n in names]
        got, ks = run_cuts(dev, lib, waves, [CUTS[n] for n in names], rows)
        for n, w, g in zip(names, waves, got):
            ref = whole(dev, lib, w)
            assert g.shape == ref.shape == (T, 128)
            assert torch.equal(bits(g), bits(ref)), f"cut list {n}: {(bits(g) != bits(ref)).any(dim=1).sum().item()} frames differ"
        log += ks.log
    hit = [(tl, f) for _, tl, _, f in log if f > 0]
    offs = {tl - j * SHIFT for tl, f in hit for j in range(f) if 0 <= tl - j * SHIFT < WIN}
    assert (0, 16) in [(tl, f) for tl, f in hit] and 1 in offs and WIN - 1 in offs and any(1 < o < WIN - 1 for o in offs)
    assert any(tl > 0 and tl % SHIFT == 0 for tl, _ in hit)                         # the boundary is the first sample of a later frame
    hops = {m for _, _, m, _ in log}
    assert {1, 159, 160, 161, 239, 240, 241, 2559, 2560, 2561, 2799, 2800, 2801, 0} <= hops
    assert any(f >= 48 for _, _, _, f in log)                                        # a backlog of several columns
    a = [e for e in log if e[0] == 3]
    assert a[0][3] == 0 and a[1][3] == 0 and a[1][1] == 1                            # two hops in a row only append


def check_independence(dev, lib):
    """2: a session's frames and its tail row do not depend on who else is in the call or on its row; rows outside a call keep the canary"""
    cuts = [161, 2800, 0, 2559, 4000]
    w = clip_wave(5).to(dev)
    others = [clip_wave(6).to(dev), clip_wave(7).to(dev)]
    (alone,), ks0 = run_cuts(dev, lib, [w], [cuts], [0])
    assert torch.equal(ks0.tails[1:], torch.full((POOL - 1, CAP), CANARY, device=dev))
    base_row = ks0.tails[0].clone()
    n_cut = [[100, 50, 3000, 160, 1], [2801, 1, 0, 5000, 239]]                        # other hop sizes; the first starts with hops of no frame
    for rows, order in (([0, 1, 2], (0, 1, 2)), ([1, 2, 0], (1, 2, 0)), ([3, 4, 1], (0, 1, 2)), ([2, 0, 4], (1, 0, 2))):
        # order: where the session under test stands in the pack (first, last, on another row, in the middle)
        waves, cl = [None] * 3, [None] * 3
        me = order.index(0)
        waves[me], cl[me] = w, cuts
        for o, slot in zip(range(2), [i for i in range(3) if i != me]):
            waves[slot], cl[slot] = others[o], n_cut[o]
        got, ks = run_cuts(dev, lib, waves, cl, rows)
        assert torch.equal(bits(got[me]), bits(alone))
        assert torch.equal(bits(ks.tails[rows[me]]), bits(base_row))
        for r in set(range(POOL)) - set(rows):
            assert torch.equal(ks.tails[r], torch.full((CAP,), CANARY, device=dev)), r


# ---- model level ---------------------------------------------------------------------------------
def make(dev):
    from aum.frontend import WaveInput
    model = sc.make_causal_aum(64, dev, depth=2)
    fe = WaveInput(tables(dev), target_length=T)
    return model, fe


class Recorder:
    """records the (frames, sessions) of every stream_push_many a push of raw audio makes"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __enter__(self):
        inner = self.model.stream_push_many

        def spy(specs, pool, sessions, **kw):
            self.calls.append(([s.clone() for s in specs], list(sessions)))
            return inner(specs, pool, sessions, **kw)
        self.model.stream_push_many = spy
        return self

    def __exit__(self, *exc):
        del self.model.stream_push_many


def caches_equal(a, b):
    return all(torch.equal(a["layers"][i][0], b["layers"][i][0]) and torch.equal(a["layers"][i][1], b["layers"][i][1]) for i in a["layers"]) \
        and a["columns"] == b["columns"]


# the clips of check_end: 200 real frames (column 12 half real, columns 13 .. 15 padding only), 250 real frames (the last column part
# real, part padding, no column of padding alone) and a clip shorter than the window (no real frame)
END_LENS = (WIN + 199 * SHIFT + 37, WIN + 249 * SHIFT + 159, WIN - 1)


def check_end(dev, lib):
    """4: end=True pushes the remaining real frames and the padding rows -> fbank_fwd(wave, 256) bit for bit, the caches of
    stream_push_many on the same frames in the same groups, stream_read = model(spec)"""
    model, fe = make(dev)
    rows = [4, 1, 2]
    waves = [clip_wave(40 + i, n).to(dev) for i, n in enumerate(END_LENS)]
    pool, ws = model.allocate_stream_pool(POOL), model.allocate_wave_stream(POOL, fe)
    hops = [[9000, 12000, END_LENS[0] - 21000], [161, 30000, END_LENS[1] - 30161], [100, 200, WIN - 301]]
    with Recorder(model) as rec:
        for step in range(3):
            at = [sum(h[:step]) for h in hops]
            counts = model.stream_push_wave_many([w[a:a + h[step]] for w, a, h in zip(waves, at, hops)], pool, ws, rows, end=step == 2)
    assert counts == [16, 16, 16] and all(ws.ended[r] for r in rows) and [ws.samples[r] for r in rows] == list(END_LENS)
    specs = []
    for i, r in enumerate(rows):
        mine = torch.cat([s for sp, ses in rec.calls for s, q in zip(sp, ses) if q == r])
        ref = whole(dev, lib, waves[i])
        assert torch.equal(bits(mine), bits(ref)), (i, (bits(mine) != bits(ref)).any(dim=1).sum().item())
        specs.append(ref)
    assert abs(float(specs[2][0, 0]) - (0.0 - MEAN) / (2 * STD)) < 1e-6 and torch.equal(specs[2], specs[2][:1].expand(T, -1))   # padding rows only
    pool2 = model.allocate_stream_pool(POOL)
    for sp, ses in rec.calls:
        model.stream_push_many(sp, pool2, ses)
    assert caches_equal(pool, pool2)
    with torch.no_grad():
        full = model(torch.stack(specs))
    got = model.stream_read(pool, sessions=rows)
    e = rel_err(got.cpu().numpy(), full.cpu().numpy())
    print(f"end of clip: stream_read vs model(spec) {e:.3e} (bar 1e-4)")
    assert e < 1e-4
    with pytest.raises(ValueError, match="ended"):
        model.stream_push_wave_many([waves[0][:10]], pool, ws, [rows[0]])
    model.stream_reset(pool, rows[:1])
    ws.reset(rows[:1])
    assert model.stream_push_wave_many([waves[0][:2800]], pool, ws, rows[:1]) == [1]


def check_read(dev, lib):
    """5: read=True returns stream_push_many(read=True) for the sessions that gained columns and stream_read for the others"""
    model, fe = make(dev)
    rows = [3, 0, 2]
    waves = [clip_wave(60 + i).to(dev) for i in range(3)]
    pool, ws = model.allocate_stream_pool(POOL), model.allocate_wave_stream(POOL, fe)
    pool2 = model.allocate_stream_pool(POOL)
    for hop, gain in (([2800, 100, 5600], [True, False, True]), ([100, 50, 10], [False, False, False]), ([2500, 2700, 2560], [True, True, True])):
        at = [ws.samples[r] for r in rows]
        with Recorder(model) as rec:
            counts, logits = model.stream_push_wave_many([w[a:a + h] for w, a, h in zip(waves, at, hop)], pool, ws, rows, read=True)
        assert logits.shape == (3, 7) and counts == [pool["columns"][r] for r in rows]
        assert [len(rec.calls) == 1 and r in rec.calls[0][1] for r in rows] == gain if any(gain) else not rec.calls
        ref = torch.empty_like(logits)
        if rec.calls:
            sp, ses = rec.calls[0]
            _, lg = model.stream_push_many(sp, pool2, ses, read=True)
            for j, r in enumerate(ses):
                ref[rows.index(r)] = lg[j]
        quiet = [r for r, g in zip(rows, gain) if not g]
        if quiet:
            lg = model.stream_read(pool2, sessions=quiet)
            for j, r in enumerate(quiet):
                ref[rows.index(r)] = lg[j]
        assert torch.equal(logits, ref)
        assert caches_equal(pool, pool2)
    # the fixed-batch, lockstep form: the same frames as fbank_fwd, stream_push underneath
    cache, ws1 = model.allocate_inference_cache(2), model.allocate_wave_stream(2, fe)
    two = torch.stack(waves[:2])
    assert model.stream_push_wave(two[:, :1000], cache, ws1) == 0
    n, lg = model.stream_push_wave(two[:, 1000:9000], cache, ws1, read=True)
    assert n == 3 and lg.shape == (2, 7)
    n, lg = model.stream_push_wave(two[:, 9000:], cache, ws1, read=True, end=True)
    cache2 = model.allocate_inference_cache(2)
    spec = torch.stack([whole(dev, lib, w) for w in waves[:2]])
    model.stream_push(spec[:, :48], cache2)
    n2, lg2 = model.stream_push(spec[:, 48:], cache2, read=True)
    assert n == n2 == 16 and torch.equal(lg, lg2) and caches_equal(cache, cache2)


def _snapshot(ws, caches):
    return (ws.tails.clone(), list(ws.tail_len), list(ws.samples), list(ws.frames), list(ws.ended),
            [{i: (c.clone(), s.clone()) for i, (c, s) in ch["layers"].items()} for ch in caches], [ch["columns"] if isinstance(ch["columns"], int)
                                                                                                   else list(ch["columns"]) for ch in caches])


def _same(a, b):
    return (torch.equal(a[0], b[0]) and a[1:5] == b[1:5] and a[6] == b[6]
            and all(torch.equal(x[i][0], y[i][0]) and torch.equal(x[i][1], y[i][1]) for x, y in zip(a[5], b[5]) for i in x))


def check_refusals(dev, lib):
    """6: every refusal of stream_push_wave* leaves tails, counters and caches as they were; the frontend and kernel-level refusals"""
    from aum.frontend import FbankTables, WaveInput
    model, fe = make(dev)
    pool, ws = model.allocate_stream_pool(POOL), model.allocate_wave_stream(POOL, fe)
    w = clip_wave(70).to(dev)
    model.stream_push_wave_many([w[:3000], w[:500]], pool, ws, [1, 3])
    model.stream_push_wave_many([w[:100]], pool, ws, [4], end=True)
    before = _snapshot(ws, [pool])
    elsewhere = torch.zeros(10, device="meta" if torch.device(dev).type == "cpu" else "cpu")
    ok = w[3000:3100]
    cases = [
        (lambda: model.stream_push_wave_many([w[2999:], w[:161]], pool, ws, [1, 0]), ValueError, "do not fit"),           # 41 201 samples
        (lambda: model.stream_push_wave_many([w[2999:], w[:161]], pool, ws, [1, 0], end=True), ValueError, "do not fit"),
        (lambda: model.stream_push_wave_many([ok, w[:10]], pool, ws, [1, 4]), ValueError, "ended"),
        (lambda: model.stream_push_wave_many([ok, w[:10].double()], pool, ws, [1, 0]), ValueError, "fp32"),
        (lambda: model.stream_push_wave_many([ok, elsewhere], pool, ws, [1, 0]), ValueError, "fp32 on"),
        (lambda: model.stream_push_wave_many([ok, w[:10].reshape(1, 10)], pool, ws, [1, 0]), ValueError, "samples"),
        (lambda: model.stream_push_wave_many([ok, ok], pool, ws, [1, 1]), ValueError, "not distinct"),
        (lambda: model.stream_push_wave_many([ok, ok], pool, ws, [1, POOL]), ValueError, "not all rows"),
        (lambda: model.stream_push_wave_many([ok], pool, ws, [1, 0]), ValueError, "one waveform piece per session"),
        (lambda: model.stream_push_wave_many([ok, ok], pool, ws, [1, 0], end=[True]), ValueError, "one end flag"),
        (lambda: model.stream_push_wave_many([ok], pool, model.allocate_wave_stream(POOL - 1, fe), [1]), ValueError, "built for"),
        (lambda: model.stream_push_wave_many([ok], pool, {"tails": None}, [1]), TypeError, "allocate_wave_stream"),
        (lambda: model.stream_push_wave(w[None, :100], pool, ws), ValueError, "stream_push_wave_many"),
    ]
    for call, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            call()
        assert _same(before, _snapshot(ws, [pool])), msg
    cache, ws1 = model.allocate_inference_cache(2), model.allocate_wave_stream(2, fe)
    model.stream_push_wave(torch.stack((w[:3000], w[:3000])), cache, ws1)
    before = _snapshot(ws1, [cache])
    for call, exc, msg in [
        (lambda: model.stream_push_wave(w[:100], cache, ws1), ValueError, "batch=2"),
        (lambda: model.stream_push_wave(w[None, :100], cache, ws1), ValueError, "batch=2"),
        (lambda: model.stream_push_wave(torch.stack((w, w))[:, 2999:], cache, ws1), ValueError, "do not fit"),
        (lambda: model.stream_push_wave(torch.stack((ok, ok)).double(), cache, ws1), ValueError, "fp32"),
        (lambda: model.stream_push_wave(torch.stack((ok, ok)), cache, ws), ValueError, "built for"),
    ]:
        with pytest.raises(exc, match=msg):
            call()
        assert _same(before, _snapshot(ws1, [cache])), msg
    # the frontend: aug set, noise set, another FFT size, another clip length
    tabs = tables(dev)
    for bad, msg in ((WaveInput(tabs, target_length=T, aug=torch.zeros(1, 8, device=dev)), "aug"),
                     (WaveInput(tabs, target_length=T, noise=torch.zeros(1, T, 128, device=dev)), "noise"),
                     (WaveInput(FbankTables(dev, sample_rate=8000), target_length=T), "padded"),
                     (WaveInput(tabs, target_length=1024), "target_length")):
        with pytest.raises(ValueError, match=msg):
            model.allocate_wave_stream(POOL, bad)
    # the binding: operands the kernel does not take, maps the host check refuses
    tails = torch.zeros(POOL, CAP, device=dev)
    good = aum_hip.wave_map([100], [0], [0], [0], [-1], [2], device=dev)
    for kw, wave_, tails_, tabs_ in (({"aug": torch.zeros(1, 8, device=dev)}, ok, tails, tabs.tables), ({"noise": torch.zeros(1, device=dev)}, ok, tails, tabs.tables),
                                     ({}, ok[None], tails, tabs.tables), ({}, ok.half(), tails, tabs.tables), ({}, ok, tails[:, :CAP - 1], tabs.tables),
                                     ({}, ok, tails, FbankTables(dev, sample_rate=8000).tables)):
        with pytest.raises(RuntimeError, match="fbank_stream: unsupported operands"):
            aum_hip.fbank_stream(wave_, good, tails_, tabs_, MEAN, STD, lib=lib, **kw)
    assert not aum_hip.fbank_stream_supported(ok[None], tails, tabs.tables) and aum_hip.fbank_stream_supported(ok, tails, tabs.tables)
    with pytest.raises(ValueError, match="pool row"):
        aum_hip.fbank_stream(ok, aum_hip.wave_map([100], [0], [0], [0], [-1], [POOL], device=dev), tails, tabs.tables, MEAN, STD, lib=lib)
    with pytest.raises(ValueError, match="describes"):
        aum_hip.fbank_stream(ok[:50], good, tails, tabs.tables, MEAN, STD, lib=lib)
    assert torch.equal(tails, torch.zeros_like(tails))
    for args, msg in ((([-1], [0], [0], [0], [-1]), ">= 0"), (([10], [CAP], [0], [0], [-1]), "tail_len"), (([10, 10], [0, 0], [0, 0], [0, 0], [-1, -1], [1, 1]), "distinct"),
                      (([2799], [0], [16], [0], [-1]), "asks for"), (([2800], [2799], [0], [0], [-1]), "left with"), (([10], [0, 0], [0], [0], [-1]), "one entry")):
        with pytest.raises(ValueError, match=msg):
            aum_hip.wave_map(*args, device=dev)


def check_c_codes(lib):
    """the AUM_E_* codes of aum_fbank_stream_fwd itself, on host buffers (the lane-array build)"""
    import ctypes as C
    tabs = tables("cpu").tables
    m = aum_hip.wave_map([100], [0], [0], [0], [-1], [1], device="cpu")
    wave, tails, held = torch.arange(100.0) + 1, torch.zeros(POOL, CAP), torch.zeros(8)

    def run(**kw):
        a = aum_hip.FbankStreamArgs()
        f = a.fbank
        f.wave, f.window, f.twiddle = wave.data_ptr(), tabs["window"].data_ptr(), tabs["twiddle"].data_ptr()
        f.mel_start_f, f.mel_count_f, f.mel_w = tabs["mel_start_f"].data_ptr(), tabs["mel_count_f"].data_ptr(), tabs["mel_w"].data_ptr()
        f.win, f.shift, f.padded, f.num_mel, f.mel_wstride = WIN, SHIFT, 512, 128, tabs["mel_w"].shape[1]
        a.cu_samples, a.cu_frames, a.tail_len = m.cu_samples.data_ptr(), m.cu_frames.data_ptr(), m.tail_len.data_ptr()
        a.first_frame, a.n_real, a.idx, a.tails = m.first_frame.data_ptr(), m.n_real_t.data_ptr(), m.idx.data_ptr(), tails.data_ptr()
        a.total_samples, a.total_frames, a.nseq, a.nrows, a.cap = 100, 0, 1, POOL, CAP
        for k, v in kw.items():
            setattr(a.fbank if k in ("aug", "noise", "padded", "win", "window") else a, k, v)
        return lib.c.aum_fbank_stream_fwd(C.byref(a), None)
    assert run() == 0 and torch.equal(tails[1, :100], wave) and float(tails.sum()) == float(wave.sum())
    assert run(aug=held.data_ptr()) == -4 and run(noise=held.data_ptr()) == -4 and run(padded=256) == -4 and run(padded=1024) == -4
    assert run(cap=CAP - 1) == -4 and run(cap=CAP + 1) == -4 and run(win=0) == -2
    assert run(tails=None) == -1 and run(window=None) == -1 and run(cu_samples=None) == -1 and run(tail_len=None) == -1
    assert run(nseq=0) == -2 and run(nrows=0) == -2 and run(total_samples=0) == -2 and run(total_samples=-1) == -2
    assert run(idx=m.idx.data_ptr() + 2) == -4
    assert lib.c.aum_fbank_stream_fwd(None, None) == -1
