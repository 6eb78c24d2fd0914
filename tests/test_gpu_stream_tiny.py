"""GPU: streaming inference of an AuM-Tiny-width model (embed_dim 192: d_inner 384, dt_rank 12) in bf16 on the one-launch block path
and the fused x/dt projections behind prefill, through the padded layout of Mamba.stream_params.  The bar is the one the streaming model
tests use for 16-bit models at the Base / Small widths (2e-2, stream_block_checks.check_model_arms).
On the commit before the feature the launch-count assertions fail: every hop runs the ladder."""
import pytest
import torch

import xdt_tiny_checks as TC
from conftest import rel_err
from stream_block_checks import _fused

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-2
DEPTH, COLS = 2, 4
LADDER = ("conv1d_stream", "scan_stream")


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.fixture(scope="module")
def model():
    from aum.model import AudioMamba
    torch.manual_seed(3)
    m = AudioMamba(embed_dim=192, depth=DEPTH, spectrogram_size=(128, 16 * COLS), num_classes=7, bimamba_type="none", use_middle_cls_token=False,
                   use_end_cls_token=True, transpose_token_sequence=True, if_bidirectional=False)
    return m.eval().to(DEV).to(torch.bfloat16)


@pytest.fixture(scope="module")
def spec():
    torch.manual_seed(11)
    return torch.randn(3, 16 * COLS, 128, device=DEV).to(torch.bfloat16)


def _push_all(model, spec, hops):
    cache, col = model.allocate_inference_cache(spec.shape[0]), 0
    for k in hops:
        assert model.stream_push(spec[:, 16 * col:16 * (col + k)], cache) == col + k
        col += k
    return cache


def test_hops_then_read_match_the_whole_clip_and_the_ladder(model, spec):
    with torch.no_grad():
        full = model(spec[:2])
        reads = {}
        for hops in ((1, 1, 1, 1), (2, 2)):
            with TC.count_calls("stream_block", *LADDER) as n:
                cache = _push_all(model, spec[:2], hops)
                snap = [(c.clone(), s.clone()) for c, s in cache["layers"].values()]
                got = model.stream_read(cache)
            # one launch of the recurrent middle per block and hop, and one per block for the read (in place: commit=False)
            assert n == {"stream_block": DEPTH * (len(hops) + 1), "conv1d_stream": 0, "scan_stream": 0}, n
            for (c, s), (c1, s1) in zip(cache["layers"].values(), snap):
                assert torch.equal(c, c1) and torch.equal(s, s1)
            with _fused(False), TC.count_calls("stream_block", *LADDER) as n:
                ref = model.stream_read(_push_all(model, spec[:2], hops))
            assert n["stream_block"] == 0 and n["conv1d_stream"] == n["scan_stream"] == DEPTH * (len(hops) + 1), n
            e_full, e_lad = rel_err(_np(got), _np(full)), rel_err(_np(got), _np(ref))
            print(f"tiny stream hops {hops}: read vs model(spec) {e_full:.3e}, vs the ladder {e_lad:.3e} (bar {BAR:.0e})")
            assert e_full < BAR and e_lad < BAR
            reads[hops] = got
        assert rel_err(_np(reads[(1, 1, 1, 1)]), _np(reads[(2, 2)])) < BAR


def test_push_many_with_read_matches_sessions_served_alone(model, spec):
    with torch.no_grad():
        pool = model.allocate_stream_pool(3)
        alone = [model.allocate_inference_cache(1) for _ in range(3)]
        sessions = [2, 0, 1]
        model.stream_push_many([spec[1, :16]], pool, [0])                 # session 0 (clip 1) is a column ahead
        model.stream_push(spec[1:2, :16], alone[1])
        at = [0, 1, 0]
        for ks in ((1, 2, 1), (2, 1, 1)):
            pieces = [spec[i, 16 * at[i]:16 * (at[i] + k)] for i, k in enumerate(ks)]
            with TC.count_calls("stream_block", *LADDER) as n:
                cols, logits = model.stream_push_many(pieces, pool, sessions, read=True)
            assert n == {"stream_block": DEPTH, "conv1d_stream": 0, "scan_stream": 0}, n
            at = [a + k for a, k in zip(at, ks)]
            assert cols == at and logits.shape == (3, 7)
            for i, piece in enumerate(pieces):
                model.stream_push(piece.unsqueeze(0), alone[i])
                e = rel_err(_np(logits[i:i + 1]), _np(model.stream_read(alone[i])))
                print(f"tiny push_many(read=True) session {sessions[i]} at column {at[i]}: vs served alone {e:.3e} (bar {BAR:.0e})")
                assert e < BAR
        for i, r in enumerate(sessions):
            for (pc, ps), (ac, as_) in zip(pool["layers"].values(), alone[i]["layers"].values()):
                assert rel_err(_np(pc[r]), _np(ac[0])) < BAR and rel_err(_np(ps[r]), _np(as_[0])) < BAR


def test_prefill_then_live_push_matches_pushing_everything(model, spec):
    with torch.no_grad():
        want = model.stream_read(_push_all(model, spec[:1], (3, 1)))
        cache = model.allocate_inference_cache(1)
        with TC.count_calls("xdt_tm_fwd") as n:
            model.stream_prefill(spec[:1, :48], cache)
        assert n["xdt_tm_fwd"] == DEPTH, n                                 # the fused projections behind prefill
        model.stream_push(spec[:1, 48:], cache)
        e = rel_err(_np(model.stream_read(cache)), _np(want))
        print(f"tiny stream_prefill(3 columns) + push vs pushes: {e:.3e} (bar {BAR:.0e})")
        assert e < BAR
        # packed: backlogs of 3, 2 and 1 columns of three clips into rows 1, 2, 0, then the rest live
        pool, rows, ks = model.allocate_stream_pool(3), [1, 2, 0], (3, 2, 1)
        with TC.count_calls("xdt_tm_fwd") as n:
            assert model.stream_prefill_many([spec[i, :16 * k] for i, k in enumerate(ks)], pool, rows, packed=True) == list(ks)
        assert n["xdt_tm_fwd"] == DEPTH, n
        model.stream_push_many([spec[i, 16 * k:] for i, k in enumerate(ks)], pool, rows)
        got = model.stream_read(pool, sessions=rows)
        for i in range(3):
            ref = model.stream_read(_push_all(model, spec[i:i + 1], (ks[i], COLS - ks[i])))
            e = rel_err(_np(got[i:i + 1]), _np(ref))
            print(f"tiny stream_prefill_many(packed) clip {i} ({ks[i]} columns) + push vs pushes: {e:.3e} (bar {BAR:.0e})")
            assert e < BAR
