"""GPU: chunked streaming inference on libaum_hip.so (aum_conv1d_tm_chunk, aum_scan_tm_chunk, Mamba.step_chunk, AudioMamba.stream_*):
the checks of tests/stream_checks.py at the lane-array tests' shapes and at the AuM-Base width (dim 1536, batch 1 and 8).
Run with -m gpu on an MI355X."""
import pytest
import torch

import aum_hip
import stream_checks as sc

pytestmark = pytest.mark.gpu

# (case, batch, dim): every case at the small shape; the AuM-Base width for one hop (8), a ragged chunk (9) and a long one (64)
SMALL = [(c, 2, None) for c in sc.SCAN_CASES]
BASE = [(c, b, 1536) for c in sc.SCAN_CASES if c[0] in (8, 9, 64) for b in (1, 8)]
SMALL_CONV = [(c, 2, None) for c in sc.CONV_CASES]
BASE_CONV = [(c, b, 1536) for c in sc.CONV_CASES if c[0] in (8, 9, 64) for b in (1, 8)]
_id = lambda p: f"{sc.case_id(p[0])}-b{p[1]}-d{p[2] or 'small'}"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


def _scan(p):
    case, batch, dim = p
    return sc.scan_setup(case, "cuda", batch=batch, **({} if dim is None else {"dim": dim}))


def _conv(p):
    case, batch, dim = p
    return sc.conv_setup(case, "cuda", batch=batch, **({} if dim is None else {"dim": dim}))


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_scan_chunk_vs_oracle(p, lib):
    sc.check_vs_oracle(_scan(p), sc.scan_run, lib)


@pytest.mark.parametrize("p", SMALL_CONV + BASE_CONV, ids=_id)
def test_conv_chunk_vs_oracle(p, lib):
    sc.check_vs_oracle(_conv(p), sc.conv_run, lib)


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_scan_chunk_partition_is_bitwise(p, lib):
    sc.check_partition_bitwise(_scan(p), sc.scan_run, lib)


@pytest.mark.parametrize("p", SMALL_CONV + BASE_CONV, ids=_id)
def test_conv_chunk_partition_is_bitwise(p, lib):
    sc.check_partition_bitwise(_conv(p), sc.conv_run, lib)


@pytest.mark.parametrize("p", SMALL + BASE, ids=_id)
def test_scan_chunk_vs_per_token_kernel(p, lib):
    sc.check_vs_per_token(_scan(p), sc.scan_run, sc.scan_run_per_token, lib)


@pytest.mark.parametrize("p", SMALL_CONV + BASE_CONV, ids=_id)
def test_conv_chunk_vs_per_token_kernel(p, lib):
    sc.check_vs_per_token(_conv(p), sc.conv_run, sc.conv_run_per_token, lib)


@pytest.mark.parametrize("d_model", [32, 768])
def test_mamba_forward_takes_chunks_after_prefill(d_model, lib):
    """fails on the parent commit: ValueError at the first 4-token chunk"""
    sc.check_mamba_chunks(d_model, "cuda")


def test_model_stream_matches_whole_clip_fp32(lib):
    sc.check_model_stream(768, "cuda")


def test_model_stream_matches_whole_clip_bf16_autocast(lib):
    sc.check_model_stream(768, "cuda", autocast_dtype=torch.bfloat16)


def test_model_stream_rejects_non_causal_configurations(lib):
    sc.check_model_rejects("cuda")
