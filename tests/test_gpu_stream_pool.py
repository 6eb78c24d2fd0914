"""GPU: many streaming sessions at different positions in one call on libaum_hip.so (aum_conv1d_tm_chunk_var, aum_scan_tm_chunk_var,
Mamba.step_chunk(seq_map=), AudioMamba.stream_push_many): the checks of tests/stream_pool_checks.py at the lane-array tests' shapes
(4 sessions) and at the AuM-Base width (dim 1536, 8 sessions).  Run with -m gpu on an MI355X."""
import pytest
import torch

import aum_hip
import stream_checks as sc
import stream_pool_checks as pc

pytestmark = pytest.mark.gpu

OPS = {"scan": (pc.ScanOp, sc.SCAN_CASES), "conv": (pc.ConvOp, sc.CONV_CASES)}
# (operator, case, sessions, dim): every case at the small shape; the AuM-Base width for one hop (8), a ragged chunk (9) and a long one (64)
SMALL = [(name, c, 4, None) for name, (_, cases) in OPS.items() for c in cases]
BASE = [(name, c, 8, 1536) for name, (_, cases) in OPS.items() for c in cases if c[0] in (8, 9, 64)]
_id = lambda p: f"{p[0]}-{sc.case_id(p[1])}-s{p[2]}-d{p[3] or 'small'}"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_packed_sessions_equal_batch1_calls_bitwise(p, lib):
    pc.check_packing_bitwise(OPS[p[0]][0], p[1], lib, "cuda", sessions=p[2], dim=p[3])


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_packed_calls_vs_oracle(p, lib):
    pc.check_var_vs_oracle(OPS[p[0]][0], p[1], lib, "cuda", sessions=p[2], dim=p[3])


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_null_state_indices_is_the_identity_mapping(p, lib):
    pc.check_null_indices(OPS[p[0]][0], p[1], lib, "cuda", sessions=p[2], dim=p[3])


def test_seq_map_validates_on_the_host(lib):
    pc.check_seq_map_validates("cuda")


@pytest.mark.parametrize("d_model", [32, 24, 768])
def test_mamba_step_chunk_takes_packed_sessions(d_model, lib):
    pc.check_mamba_pool(d_model, "cuda")


def test_model_pool_matches_whole_clips_fp32(lib):
    pc.check_model_pool(768, "cuda")


def test_model_pool_matches_whole_clips_bf16_autocast(lib):
    pc.check_model_pool(768, "cuda", autocast_dtype=torch.bfloat16)
