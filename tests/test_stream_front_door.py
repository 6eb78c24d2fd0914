"""CPU: the streaming front door -- AudioMamba.stream_push / stream_prefill / stream_push_many / stream_prefill_many / stream_read /
stream_reset and Mamba.step_chunk(seq_map=) / prefill_chunk(seq_map=) -- held to what it did BEFORE its checks, its packer and its x/dt
stage were folded into one helper each: every refusal (exception type and full message text, which refusal wins when two apply, nothing
touched behind a refusal) and the launch sequence of one valid call of every entry point, as literals recorded on the commit before
the refactor.  The model runs on the lane-array build of the kernel sources (tests/emu), as the other host stream tests run it.
This file passed unmodified on that commit and passes unmodified on the refactor; tests/test_gpu_stream_front_door.py holds the
launch sequences where the one-launch path is taken."""
import copy
import os
import sys
import types

import pytest
import torch

import aum_hip
import stream_checks as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
NONSTREAMABLE = {"v1": {"bimamba_type": "v1"}, "bidir": {"if_bidirectional": True}, "middle": {"use_middle_cls_token": True},
                 "noend": {"use_end_cls_token": False}, "notm": {"transpose_token_sequence": False}}


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture()
def emu_as_product(lib):
    old = aum_hip._product
    aum_hip._product = lib
    yield
    aum_hip._product = old


@pytest.fixture(scope="module")
def models():
    """the depth-2 causal model (16 time columns) and its five non-streamable siblings, which take the good model's caches"""
    out = {"ok": sc.make_causal_aum(64, "cpu", depth=2)}
    for k, over in NONSTREAMABLE.items():
        out[k] = sc.make_causal_aum(64, "cpu", depth=2, **over)
    return out


def make_base(models, lib):
    """one valid call of every entry point starts here: a fixed-batch cache of 2 at column 3 and a pool of 3 at columns [2, 0, 5],
    all caches non-zero; the calls push 1 column (fixed batch) and 1 and 2 columns to sessions [2, 0]"""
    old, aum_hip._product = aum_hip._product, lib
    try:
        m = models["ok"]
        torch.manual_seed(21)
        spec = torch.randn(3, 256, 128)
        with torch.no_grad():
            cache = m.allocate_inference_cache(2)
            m.stream_push(spec[:2, :48], cache)
            pool = m.allocate_stream_pool(3)
            m.stream_push_many([spec[0, :32], spec[2, :80]], pool, [0, 2])
            m.stream_push_many([spec[1, :16]], pool, [1])
            m.stream_reset(pool, [1])
            m.stream_push_many([spec[1, :16]], pool, [1])
            m.stream_reset(pool, [1])
        assert cache["columns"] == 3 and pool["columns"] == [2, 0, 5]
        return types.SimpleNamespace(spec=spec[:2, 48:64], cache=cache, specs=[spec[2, 80:96], spec[0, 32:64]], pool=pool, sessions=[2, 0])
    finally:
        aum_hip._product = old


@pytest.fixture(scope="module")
def base(models, lib):
    return make_base(models, lib)


def fresh(base):
    s = copy.deepcopy(base)
    s.model = "ok"
    return s


ENTRY = {
    "push": lambda m, s, **kw: m.stream_push(s.spec, s.cache, **kw),
    "prefill": lambda m, s, **kw: m.stream_prefill(s.spec, s.cache, **kw),
    "push_many": lambda m, s, **kw: m.stream_push_many(s.specs, s.pool, s.sessions, **kw),
    "prefill_many": lambda m, s: m.stream_prefill_many(s.specs, s.pool, s.sessions),
    "prefill_many_packed": lambda m, s: m.stream_prefill_many(s.specs, s.pool, s.sessions, packed=True),
    "read": lambda m, s: m.stream_read(s.cache),
    "read_sessions": lambda m, s: m.stream_read(s.pool, sessions=s.sessions),
    "reset": lambda m, s: m.stream_reset(s.pool, s.sessions),
}


def _set(**kw):
    def f(s):
        for k, v in kw.items():
            setattr(s, k, v(s))
    return f


def _cols_full(s):
    s.cache["columns"] = 16
    s.pool["columns"][2] = 15           # session 2 gets 1 column, session 0 gets 2: 15 + 1 fits, so only ...
    s.pool["columns"][0] = 15           # ... session 0 (the SECOND piece) overflows


FAULTS = {
    **{k: _set(model=lambda s, k=k: k) for k in NONSTREAMABLE},
    "pool_for_cache": _set(cache=lambda s: s.pool),
    "cache_for_pool": _set(pool=lambda s: s.cache),
    "rank": _set(spec=lambda s: s.spec[0], specs=lambda s: [s.specs[0][None], s.specs[1]]),
    "zero_frames": _set(spec=lambda s: s.spec[:, :0], specs=lambda s: [s.specs[0], s.specs[1][:0]]),
    "odd_frames": _set(spec=lambda s: s.spec[:, :9], specs=lambda s: [s.specs[0], s.specs[1][:24]]),
    "mel_bins": _set(spec=lambda s: s.spec[:, :, :64], specs=lambda s: [s.specs[0][:, :64], s.specs[1]]),
    "batch": _set(spec=lambda s: s.spec[:1]),
    "no_fit": _cols_full,
    "no_fit_first": lambda s: s.pool["columns"].__setitem__(2, 16),
    "duplicate": _set(sessions=lambda s: [2, 2]),
    "out_of_range": _set(sessions=lambda s: [2, 3]),
    "negative": _set(sessions=lambda s: [-1, 0]),
    "empty": _set(sessions=lambda s: [], specs=lambda s: []),
    "one_spec": _set(specs=lambda s: s.specs[:1]),
}

MANY = ("push_many", "prefill_many", "prefill_many_packed")
# (entry point, the faults applied in this order, exception, message) -- recorded on the commit before the refactor
REFUSALS = [
    ('push', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('prefill', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('push_many', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('prefill_many', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('prefill_many_packed', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('read', ('v1',), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('push', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('prefill', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('push_many', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('prefill_many', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('prefill_many_packed', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('read', ('bidir',), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('push', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('prefill', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('push_many', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('prefill_many', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('prefill_many_packed', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('read', ('middle',), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('push', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('prefill', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('push_many', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('prefill_many', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('prefill_many_packed', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('read', ('noend',), 'ValueError',
     'streaming inference needs use_end_cls_token=True (the cls token must close the sequence)'),
    ('push', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('prefill', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('push_many', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('prefill_many', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('prefill_many_packed', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('read', ('notm',), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('push', ('pool_for_cache',), 'ValueError',
     'stream_push advances all rows of a cache from allocate_inference_cache together; a pool from allocate_stream_pool is advanced by stream_push_many(specs, pool, sessions)'),
    ('prefill', ('pool_for_cache',), 'ValueError',
     'stream_prefill advances all rows of a cache from allocate_inference_cache together; a pool from allocate_stream_pool is advanced by stream_prefill_many(specs, pool, sessions)'),
    ('push_many', ('cache_for_pool',), 'ValueError',
     'stream_push_many takes a pool from allocate_stream_pool'),
    ('prefill_many', ('cache_for_pool',), 'ValueError',
     'stream_prefill_many takes a pool from allocate_stream_pool'),
    ('prefill_many_packed', ('cache_for_pool',), 'ValueError',
     'stream_prefill_many takes a pool from allocate_stream_pool'),
    ('reset', ('cache_for_pool',), 'ValueError',
     'stream_reset takes a pool from allocate_stream_pool'),
    ('push', ('rank',), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (16, 128)'),
    ('prefill', ('rank',), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (16, 128)'),
    ('push_many', ('rank',), 'ValueError',
     'stream_push_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (1, 16, 128) for session 2'),
    ('prefill_many', ('rank',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (1, 16, 128) for session 2'),
    ('prefill_many_packed', ('rank',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (1, 16, 128) for session 2'),
    ('push', ('zero_frames',), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 0, 128)'),
    ('prefill', ('zero_frames',), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 0, 128)'),
    ('push_many', ('zero_frames',), 'ValueError',
     'stream_push_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (0, 128) for session 0'),
    ('prefill_many', ('zero_frames',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (0, 128) for session 0'),
    ('prefill_many_packed', ('zero_frames',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (0, 128) for session 0'),
    ('push', ('odd_frames',), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 9, 128)'),
    ('prefill', ('odd_frames',), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 9, 128)'),
    ('push_many', ('odd_frames',), 'ValueError',
     'stream_push_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (24, 128) for session 0'),
    ('prefill_many', ('odd_frames',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (24, 128) for session 0'),
    ('prefill_many_packed', ('odd_frames',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (24, 128) for session 0'),
    ('push', ('mel_bins',), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 16, 64)'),
    ('prefill', ('mel_bins',), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 16, 64)'),
    ('push_many', ('mel_bins',), 'ValueError',
     'stream_push_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
    ('prefill_many', ('mel_bins',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
    ('prefill_many_packed', ('mel_bins',), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
    ('push', ('batch',), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (1, 16, 128)'),
    ('prefill', ('batch',), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (1, 16, 128)'),
    ('push', ('no_fit',), 'ValueError',
     'the clip has 16 time columns: 16 pushed, 1 more do not fit'),
    ('prefill', ('no_fit',), 'ValueError',
     'the clip has 16 time columns: 16 pushed, 1 more do not fit'),
    ('push_many', ('no_fit',), 'ValueError',
     'the clip has 16 time columns: session 0 pushed 15, 2 more do not fit'),
    ('prefill_many', ('no_fit',), 'ValueError',
     'the clip has 16 time columns: session 0 pushed 15, 2 more do not fit'),
    ('prefill_many_packed', ('no_fit',), 'ValueError',
     'the clip has 16 time columns: session 0 pushed 15, 2 more do not fit'),
    ('push_many', ('duplicate',), 'ValueError',
     'stream_push_many: the sessions [2, 2] are not distinct'),
    ('prefill_many', ('duplicate',), 'ValueError',
     'stream_prefill_many: the sessions [2, 2] are not distinct'),
    ('prefill_many_packed', ('duplicate',), 'ValueError',
     'stream_prefill_many: the sessions [2, 2] are not distinct'),
    ('reset', ('duplicate',), 'ValueError',
     'stream_reset: the sessions [2, 2] are not distinct'),
    ('push_many', ('out_of_range',), 'ValueError',
     'stream_push_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many', ('out_of_range',), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many_packed', ('out_of_range',), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('reset', ('out_of_range',), 'ValueError',
     'stream_reset: the sessions [2, 3] are not all rows of a cache of 3'),
    ('push_many', ('negative',), 'ValueError',
     'stream_push_many: the sessions [-1, 0] are not all rows of a cache of 3'),
    ('prefill_many', ('negative',), 'ValueError',
     'stream_prefill_many: the sessions [-1, 0] are not all rows of a cache of 3'),
    ('prefill_many_packed', ('negative',), 'ValueError',
     'stream_prefill_many: the sessions [-1, 0] are not all rows of a cache of 3'),
    ('reset', ('negative',), 'ValueError',
     'stream_reset: the sessions [-1, 0] are not all rows of a cache of 3'),
    ('read_sessions', ('out_of_range',), 'ValueError',
     'stream_read: the sessions [2, 3] are not all rows of a cache of 3'),
    ('read_sessions', ('negative',), 'ValueError',
     'stream_read: the sessions [-1, 0] are not all rows of a cache of 3'),
    ('read_sessions', ('empty',), 'ValueError',
     'stream_read: at least one session'),
    ('push_many', ('empty',), 'ValueError',
     'stream_push_many: one spectrogram piece per session, got 0 for the sessions []'),
    ('prefill_many', ('empty',), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 0 for the sessions []'),
    ('prefill_many_packed', ('empty',), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 0 for the sessions []'),
    ('push_many', ('one_spec',), 'ValueError',
     'stream_push_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('prefill_many', ('one_spec',), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('prefill_many_packed', ('one_spec',), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('push', ('v1', 'pool_for_cache'), 'ValueError',
     "streaming inference needs bimamba_type='none' (causal blocks), not 'v1'"),
    ('prefill', ('pool_for_cache', 'batch'), 'ValueError',
     'stream_prefill advances all rows of a cache from allocate_inference_cache together; a pool from allocate_stream_pool is advanced by stream_prefill_many(specs, pool, sessions)'),
    ('push', ('zero_frames', 'batch'), 'ValueError',
     'stream_push takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (1, 0, 128)'),
    ('prefill', ('mel_bins', 'no_fit'), 'ValueError',
     'stream_prefill takes (batch=2, a positive multiple of 16 frames, 128 mel bins), got (2, 16, 64)'),
    ('read', ('bidir', 'pool_for_cache'), 'ValueError',
     'streaming inference needs if_bidirectional=False'),
    ('read_sessions', ('notm', 'out_of_range'), 'ValueError',
     'streaming inference needs transpose_token_sequence=True (time-major token order)'),
    ('reset', ('cache_for_pool', 'duplicate'), 'ValueError',
     'stream_reset takes a pool from allocate_stream_pool'),
    ('reset', ('duplicate', 'out_of_range'), 'ValueError',
     'stream_reset: the sessions [2, 3] are not all rows of a cache of 3'),
    ('push_many', ('middle', 'cache_for_pool'), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('push_many', ('cache_for_pool', 'duplicate'), 'ValueError',
     'stream_push_many takes a pool from allocate_stream_pool'),
    ('push_many', ('duplicate', 'out_of_range'), 'ValueError',
     'stream_push_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('push_many', ('out_of_range', 'one_spec'), 'ValueError',
     'stream_push_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('push_many', ('mel_bins', 'one_spec'), 'ValueError',
     'stream_push_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('push_many', ('no_fit_first', 'odd_frames'), 'ValueError',
     'the clip has 16 time columns: session 2 pushed 16, 1 more do not fit'),
    ('push_many', ('no_fit', 'mel_bins'), 'ValueError',
     'stream_push_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
    ('prefill_many', ('middle', 'cache_for_pool'), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('prefill_many', ('cache_for_pool', 'duplicate'), 'ValueError',
     'stream_prefill_many takes a pool from allocate_stream_pool'),
    ('prefill_many', ('duplicate', 'out_of_range'), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many', ('out_of_range', 'one_spec'), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many', ('mel_bins', 'one_spec'), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('prefill_many', ('no_fit_first', 'odd_frames'), 'ValueError',
     'the clip has 16 time columns: session 2 pushed 16, 1 more do not fit'),
    ('prefill_many', ('no_fit', 'mel_bins'), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
    ('prefill_many_packed', ('middle', 'cache_for_pool'), 'ValueError',
     'streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)'),
    ('prefill_many_packed', ('cache_for_pool', 'duplicate'), 'ValueError',
     'stream_prefill_many takes a pool from allocate_stream_pool'),
    ('prefill_many_packed', ('duplicate', 'out_of_range'), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many_packed', ('out_of_range', 'one_spec'), 'ValueError',
     'stream_prefill_many: the sessions [2, 3] are not all rows of a cache of 3'),
    ('prefill_many_packed', ('mel_bins', 'one_spec'), 'ValueError',
     'stream_prefill_many: one spectrogram piece per session, got 1 for the sessions [2, 0]'),
    ('prefill_many_packed', ('no_fit_first', 'odd_frames'), 'ValueError',
     'the clip has 16 time columns: session 2 pushed 16, 1 more do not fit'),
    ('prefill_many_packed', ('no_fit', 'mel_bins'), 'ValueError',
     'stream_prefill_many takes (a positive multiple of 16 frames, 128 mel bins) per session, got (16, 64) for session 2'),
]


def _snapshot(s):
    return [(c.clone(), t.clone()) for d in (s.cache, s.pool) for c, t in d["layers"].values()], copy.deepcopy((s.cache["columns"], s.pool["columns"]))


def refusal(models, base, entry, faults):
    """-> (the exception of the refused call, whether every cache tensor and every column count is as before it)"""
    s = fresh(base)
    for f in faults:
        FAULTS[f](s)
    tensors, counts = _snapshot(s)
    try:
        with torch.no_grad():
            ENTRY[entry](models[s.model], s)
    except Exception as e:              # noqa: BLE001 -- the type is asserted by the caller
        now, counts_now = _snapshot(s)
        same = counts_now == counts and all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(tensors, now))
        return e, same
    return None, True


@pytest.mark.parametrize("entry,faults,exc,msg", REFUSALS, ids=[f"{r[0]}-{'+'.join(r[1])}" for r in REFUSALS])
def test_refusal_type_text_and_nothing_touched(models, base, emu_as_product, entry, faults, exc, msg):
    e, same = refusal(models, base, entry, faults)
    assert e is not None, "the call was not refused"
    assert (type(e).__name__, str(e)) == (exc, msg)
    assert same, "a refused call changed a cache tensor or a column count"


def test_the_table_covers_the_front_door():
    got = {(r[0], r[1]) for r in REFUSALS}
    assert len(got) == len(REFUSALS)
    for k in NONSTREAMABLE:
        assert {(e, (k,)) for e in ("push", "prefill", "read") + MANY} <= got
    for f in ("rank", "zero_frames", "odd_frames", "mel_bins", "no_fit"):
        assert {(e, (f,)) for e in ("push", "prefill") + MANY} <= got
    assert {("push", ("pool_for_cache",)), ("prefill", ("pool_for_cache",)), ("push", ("batch",)), ("prefill", ("batch",))} <= got
    for f in ("cache_for_pool", "duplicate", "out_of_range", "negative"):
        assert {(e, (f,)) for e in MANY + ("reset",)} <= got
    assert {(e, (f,)) for e in MANY for f in ("empty", "one_spec")} <= got
    assert {("read_sessions", ("out_of_range",)), ("read_sessions", ("negative",)), ("read_sessions", ("empty",))} <= got
    assert sum(len(r[1]) == 2 for r in REFUSALS) >= 5


def test_valid_calls_are_taken(models, base, emu_as_product):
    """the calls the refusals are one fault away from"""
    for entry in ENTRY:
        e, _ = refusal(models, base, entry, ())
        assert e is None, (entry, e)


# ---- Mamba.step_chunk(seq_map=) / prefill_chunk(seq_map=) -------------------------------------------------------------
def _mamba():
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(5)
    m = Mamba(32, layer_idx=0, bimamba_type="none").eval()
    conv, ssm = m.allocate_inference_cache(3, 0, dtype=torch.float32)
    torch.manual_seed(6)
    return m, conv.normal_(), ssm.normal_(), torch.randn(1, 5, 32)


MAMBA_FAULTS = {
    "rank": lambda h, c, s, sm: (h[0], c, s, sm),
    "batch": lambda h, c, s, sm: (h.expand(2, -1, -1), c, s, sm),
    "pools": lambda h, c, s, sm: (h, c, s[:2], sm),
    "no_map": lambda h, c, s, sm: (h, c, s, (2, 3)),
    "map_total": lambda h, c, s, sm: (h, c, s, aum_hip.seq_map([2, 4], [2, 0], device="cpu")),
    "map_row": lambda h, c, s, sm: (h, c, s, aum_hip.seq_map([2, 3], [3, 0], device="cpu")),
    "batch+no_map": lambda h, c, s, sm: (h.expand(2, -1, -1), c, s, (2, 3)),
}
# (fault, exception, message with {f} for the entry point's name) -- recorded on the commit before the refactor
MAMBA_REFUSALS = [
    ('rank', 'ValueError',
     '{f}(seq_map=): hidden_states (1, total, d_model), pools of one size, not 3 / 3 rows'),
    ('batch', 'ValueError',
     '{f}(seq_map=): hidden_states (1, total, d_model), pools of one size, not 3 / 3 rows'),
    ('pools', 'ValueError',
     '{f}(seq_map=): hidden_states (1, total, d_model), pools of one size, not 3 / 2 rows'),
    ('no_map', 'TypeError',
     '{f}: seq_map must come from aum_hip.seq_map()'),
    ('map_total', 'ValueError',
     '{f}: seq_map describes 6 rows, the packed stream has 5'),
    ('map_row', 'ValueError',
     '{f}: seq_map names cache row 3, the pool has 3 rows'),
    ('batch+no_map', 'ValueError',
     '{f}(seq_map=): hidden_states (1, total, d_model), pools of one size, not 3 / 3 rows'),
]


@pytest.mark.parametrize("entry", ["step_chunk", "prefill_chunk"])
@pytest.mark.parametrize("fault,exc,msg", MAMBA_REFUSALS, ids=[r[0] for r in MAMBA_REFUSALS])
def test_mamba_packed_entry_refusals(emu_as_product, entry, fault, exc, msg):
    m, conv, ssm, h = _mamba()
    conv0, ssm0 = conv.clone(), ssm.clone()
    a = MAMBA_FAULTS[fault](h, conv, ssm, aum_hip.seq_map([2, 3], [2, 0], device="cpu"))
    with pytest.raises(Exception) as e, torch.no_grad():
        getattr(m, entry)(*a[:3], seq_map=a[3])
    assert (e.type.__name__, str(e.value)) == (exc, msg.format(f=entry))
    assert torch.equal(conv, conv0) and torch.equal(ssm, ssm0)


def test_mamba_refusal_table_is_complete():
    assert {r[0] for r in MAMBA_REFUSALS} == set(MAMBA_FAULTS)


@pytest.mark.parametrize("entry", ["step_chunk", "prefill_chunk"])
def test_mamba_empty_map_returns_empty(emu_as_product, entry):
    m, conv, ssm, h = _mamba()
    conv0, ssm0 = conv.clone(), ssm.clone()
    with torch.no_grad():
        out, c, s = getattr(m, entry)(h[:, :0], conv, ssm, seq_map=aum_hip.seq_map([0, 0], [2, 0], device="cpu"))
    assert out.shape == (1, 0, 32) and out.dtype == h.dtype and c is conv and s is ssm
    assert torch.equal(conv, conv0) and torch.equal(ssm, ssm0)


# ---- launch sequences -------------------------------------------------------------------------------------------------
def launches(monkeypatch, fn):
    """the (name, meta) of every aum_hip._launch under fn()"""
    seq = []
    real = aum_hip._launch

    def launch(f, args, stream_tensor, lib, name, meta=None):
        seq.append((name, meta))
        return real(f, args, stream_tensor, lib, name, meta)

    with monkeypatch.context() as mp:
        mp.setattr(aum_hip, "_launch", launch)
        with torch.no_grad():
            fn()
    return seq


# (entry point, read=True) -> the launches of the one valid call, recorded on the commit before the refactor
LAUNCHES = {
    ('push', False): [
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_chunk', (2, 128, 8, 4)),
        ('scan_tm_chunk', (2, 128, 8, 16, 4)),
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_chunk', (2, 128, 8, 4)),
        ('scan_tm_chunk', (2, 128, 8, 16, 4)),
    ],
    ('push', True): [
        ('rmsnorm_fwd', (18, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 18, 4)),
        ('scan_tm_chunk_var', (2, 128, 18, 16, 4)),
        ('rmsnorm_fwd', (18, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 18, 4)),
        ('scan_tm_chunk_var', (2, 128, 18, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
    ],
    ('prefill', False): [
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (2, 128, 11, 4)),
        ('scan_tm_fwd_state', (2, 128, 8, 16, 4, 1)),
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (2, 128, 11, 4)),
        ('scan_tm_fwd_state', (2, 128, 8, 16, 4, 1)),
    ],
    ('prefill', True): [
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (2, 128, 11, 4)),
        ('scan_tm_fwd_state', (2, 128, 8, 16, 4, 1)),
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (2, 128, 11, 4)),
        ('scan_tm_fwd_state', (2, 128, 8, 16, 4, 1)),
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
    ],
    ('push_many', False): [
        ('rmsnorm_fwd', (24, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 24, 4)),
        ('scan_tm_chunk_var', (2, 128, 24, 16, 4)),
        ('rmsnorm_fwd', (24, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 24, 4)),
        ('scan_tm_chunk_var', (2, 128, 24, 16, 4)),
    ],
    ('push_many', True): [
        ('rmsnorm_fwd', (26, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 26, 4)),
        ('scan_tm_chunk_var', (2, 128, 26, 16, 4)),
        ('rmsnorm_fwd', (26, 64, 4)),
        ('conv_tm_chunk_var', (2, 128, 26, 4)),
        ('scan_tm_chunk_var', (2, 128, 26, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
    ],
    ('prefill_many', False): [
        ('rmsnorm_fwd', (8, 64, 4)),
        ('conv_tm_fwd', (1, 128, 11, 4)),
        ('scan_tm_fwd_state', (1, 128, 8, 16, 4, 1)),
        ('rmsnorm_fwd', (8, 64, 4)),
        ('conv_tm_fwd', (1, 128, 11, 4)),
        ('scan_tm_fwd_state', (1, 128, 8, 16, 4, 1)),
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (1, 128, 19, 4)),
        ('scan_tm_fwd_state', (1, 128, 16, 16, 4, 1)),
        ('rmsnorm_fwd', (16, 64, 4)),
        ('conv_tm_fwd', (1, 128, 19, 4)),
        ('scan_tm_fwd_state', (1, 128, 16, 16, 4, 1)),
    ],
    ('prefill_many_packed', False): [
        ('rmsnorm_fwd', (24, 64, 4)),
        ('conv_tm_prefill_var', (2, 128, 24, 4)),
        ('scan_tm_fwd_state_var', (2, 128, 24, 16, 4, 0)),
        ('rmsnorm_fwd', (24, 64, 4)),
        ('conv_tm_prefill_var', (2, 128, 24, 4)),
        ('scan_tm_fwd_state_var', (2, 128, 24, 16, 4, 0)),
    ],
    ('read', False): [
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
    ],
    ('read_sessions', False): [
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
        ('conv_tm_chunk', (2, 128, 1, 4)),
        ('scan_tm_chunk', (2, 128, 1, 16, 4)),
        ('rmsnorm_fwd', (2, 64, 4)),
    ],
    ('reset', False): [
    ],
}
CALLS = [(e, r) for e in ENTRY for r in ((False, True) if e in ("push", "prefill", "push_many") else (False,))]


@pytest.mark.parametrize("entry,read", CALLS, ids=[f"{e}{'-read' if r else ''}" for e, r in CALLS])
def test_launch_sequence_of_a_valid_call(models, base, emu_as_product, monkeypatch, entry, read):
    s = fresh(base)
    seq = launches(monkeypatch, lambda: ENTRY[entry](models["ok"], s, **({"read": True} if read else {})))
    assert seq == LAUNCHES[(entry, read)]
