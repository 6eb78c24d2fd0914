"""GPU: the launch sequence of every streaming entry point where the one-launch block path is taken -- a depth-2 causal model at the
AuM-Tiny width (d_model 192, d_inner 384, dt_rank 12) in bf16 -- against the literal lists recorded on the commit before the front
door's checks, packer and x/dt stage were folded into one helper each (tests/test_stream_front_door.py: the same on the host, with
the refusals).  Hops of 1 and 2 columns (8 and 16 tokens per session), a ragged pool push, read=True, stream_read in place, and a
9-column prefill fixed-batch, packed and session by session.  The code under change is host code: no larger shape is needed."""
import pytest
import torch

import aum_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK = ["rmsnorm_fwd", "stream_block"]
PREFILL = ["rmsnorm_fwd", "conv_tm_fwd", "xdt_tm_fwd", "scan_tm_fwd_state"]
PACKED = ["rmsnorm_fwd", "conv_tm_prefill_var", "xdt_tm_fwd", "scan_tm_fwd_state_var"]
# call -> the names of its launches, recorded on the commit before the refactor
LAUNCHES = {
    "push_1_column": BLOCK * 2,
    "push_2_columns": BLOCK * 2,
    "push_read": BLOCK * 2 + ["rmsnorm_fwd"],
    "read_in_place": BLOCK * 2 + ["rmsnorm_fwd"],
    "prefill_9_columns": PREFILL * 2,
    "prefill_read": PREFILL * 2 + BLOCK * 2 + ["rmsnorm_fwd"],
    "push_many_ragged": BLOCK * 2,
    "push_many_read": BLOCK * 2 + ["rmsnorm_fwd"],
    "read_sessions": BLOCK * 2 + ["rmsnorm_fwd"],
    "read_a_row_twice": BLOCK * 2 + ["rmsnorm_fwd"],
    "prefill_many_packed": PACKED * 2,
    "prefill_many_loop": PREFILL * 4,
}


def make_model():
    from aum.model import AudioMamba
    torch.manual_seed(3)
    m = AudioMamba(embed_dim=192, depth=2, spectrogram_size=(128, 256), num_classes=7, bimamba_type="none", use_middle_cls_token=False,
                   use_end_cls_token=True, transpose_token_sequence=True, if_bidirectional=False)
    return m.eval().to(DEV).to(torch.bfloat16)


def run_calls(model, launches):
    """every call of LAUNCHES in order on one fixed-batch cache of 2 and one pool of 3 -> {call: launch names}"""
    torch.manual_seed(11)
    spec = torch.randn(3, 256, 128, device=DEV).to(torch.bfloat16)
    cache, pool = model.allocate_inference_cache(2), model.allocate_stream_pool(3)
    piece = lambda i, c0, k: spec[i, 16 * c0:16 * (c0 + k)]
    calls = {
        "push_1_column": lambda: model.stream_push(spec[:2, :16], cache),
        "push_2_columns": lambda: model.stream_push(spec[:2, 16:48], cache),
        "push_read": lambda: model.stream_push(spec[:2, 48:64], cache, read=True),
        "read_in_place": lambda: model.stream_read(cache),
        "prefill_9_columns": lambda: model.stream_prefill(spec[:2, 64:208], cache),
        "prefill_read": lambda: model.stream_prefill(spec[:2, 208:224], cache, read=True),
        "push_many_ragged": lambda: model.stream_push_many([piece(2, 0, 1), piece(0, 0, 2)], pool, [2, 0]),
        "push_many_read": lambda: model.stream_push_many([piece(2, 1, 2), piece(0, 2, 1)], pool, [2, 0], read=True),
        "read_sessions": lambda: model.stream_read(pool, sessions=[0, 2]),
        "read_a_row_twice": lambda: model.stream_read(pool, sessions=[2, 2]),
        "prefill_many_packed": lambda: model.stream_prefill_many([piece(2, 3, 9), piece(1, 0, 4)], pool, [2, 1], packed=True),
        "prefill_many_loop": lambda: model.stream_prefill_many([piece(0, 3, 9), piece(1, 4, 1)], pool, [0, 1]),
    }
    return {k: launches(fn) for k, fn in calls.items()}, cache, pool


def record(model):
    mp = pytest.MonkeyPatch()
    seq = []
    real = aum_hip._launch

    def launch(f, args, stream_tensor, lib, name, meta=None):
        seq.append(name)
        return real(f, args, stream_tensor, lib, name, meta)

    def launches(fn):
        del seq[:]
        with torch.no_grad():
            fn()
        return list(seq)

    mp.setattr(aum_hip, "_launch", launch)
    try:
        got, cache, pool = run_calls(model, launches)
        torch.cuda.synchronize()
    finally:
        mp.undo()
    assert cache["columns"] == 14 and pool["columns"] == [12, 5, 12]
    return got


@pytest.fixture(scope="module")
def recorded():
    return record(make_model())


def test_every_call_is_recorded(recorded):
    assert list(recorded) == list(LAUNCHES)


@pytest.mark.parametrize("call", list(LAUNCHES))
def test_launch_names_of_a_call(recorded, call):
    assert recorded[call] == LAUNCHES[call]
