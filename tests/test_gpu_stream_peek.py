"""GPU: the peek row of streaming inference on the device library -- k_stream_block<..., PEEK>, k_convt_chunk_var<..., PEEK> and
k_stream_scan_chunk_var<..., PEEK> against the two calls the library had before the flag (a committed call on each session's first
len - 1 rows, an AUM_STREAM_NO_COMMIT call on its last row), bit for bit; one launch against the ladder under the flags; the limit of
128 rows counting the peek row; Mamba.step_chunk(peek=) on both arms and AudioMamba.stream_push / stream_push_many(read=) under bf16
autocast (tests/stream_peek_checks.py).  On the commit before the feature every test here fails: the `peek=` / `read=` keyword raises a
TypeError (aum_hip.STREAM_PEEK_LAST is an AttributeError; the raw call with the flag is refused with AUM_E_UNSUPPORTED)."""
import pytest
import torch

import aum_hip
import stream_block_checks as bc
import stream_peek_checks as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_T = bc.MAX_T


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", ["small", "base"])
def test_peek_equals_commit_then_uncommitted_last_row(shape, dt, lib):
    for lens, rows, nrows in pc.CASES.values():
        pc.check_peek_equals_two_calls(shape, dt, lens, rows, nrows, lib, DEV)
    pc.check_peek_equals_two_calls(shape, dt, (MAX_T, 1), (1, 0), 2, lib, DEV)         # the kernel's limit: 127 rows and the peek


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_flag_off_changes_nothing(dt, lib):
    pc.check_flag_off_unchanged("base", dt, lib, DEV)
    pc.check_flag_off_unchanged("small", dt, lib, DEV)


def test_limits_count_the_peek_row(lib):
    pc.check_limits(lib, DEV)
    # 129 rows: the three launches with the two flags still satisfy the property (the reference: 128 rows in one launch, then the last row)
    pc.check_peek_equals_two_calls("small", "bf16", (MAX_T + 1, 3), (0, 1), 2, lib, DEV, block=False)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fixed_batch_with_peek_goes_through_the_packed_kernels(dt, lib):
    pc.check_fixed_batch_goes_packed("base", dt, lib, DEV)


def _mamba(d_model):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(11)
    return Mamba(d_model, bimamba_type="none", layer_idx=0).to(DEV).to(torch.bfloat16)


@pytest.mark.parametrize("d_model", [384, 768])
def test_step_chunk_peek_both_arms(d_model):
    """bf16 module: outputs and caches against the two-call form within the 16-bit output bar (the in_proj GEMM sees one more row than
    in the two calls, and a library GEMM's bits may depend on its row count; the conv window holds its 16-bit outputs); one launch with
    the flag where the shapes fit, the ladder where fused is off -- and the two arms agree bit for bit (same in_proj rows)"""
    m = _mamba(d_model)
    torch.manual_seed(3)
    h = torch.randn(2, 9, d_model, device=DEV).to(torch.bfloat16)
    bar = bc.OUT_BAR["bf16"]
    res = {}
    for on in (True, False):
        with bc._fused(on):
            pc.check_mamba_peek(m, h, DEV, bar, bar, expect_fused=on)
            smap = aum_hip.seq_map([4, 1, 0, 9], [3, 0, 1, 2], device=DEV)
            pc.check_mamba_peek(m, h.reshape(1, 18, d_model)[:, :14], DEV, bar, bar, seq_map=smap, pool_rows=4, expect_fused=on)
            with torch.no_grad():
                c, s = m.allocate_inference_cache(2, 0, dtype=torch.float32)
                torch.manual_seed(5)
                c.copy_(torch.randn(c.shape)), s.copy_(torch.randn(s.shape) * 0.3)
                out, _, _ = m.step_chunk(h, c, s, peek=True)
                res[on] = (out, c, s)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_step_chunk_peek_129_rows_takes_the_ladder():
    m = _mamba(384)
    torch.manual_seed(6)
    h = torch.randn(1, MAX_T + 1, 384, device=DEV).to(torch.bfloat16)
    bar = bc.OUT_BAR["bf16"]
    pc.check_mamba_peek(m, h, DEV, bar, bar, expect_fused=False)
    pc.check_mamba_peek(m, h[:, :MAX_T], DEV, bar, bar, expect_fused=True)


def test_model_push_read_matches_push_then_read():
    pc.check_model_push_read(768, DEV, torch.bfloat16)


def test_model_push_many_read_matches_sessions_served_alone():
    pc.check_model_push_many_read(768, DEV, torch.bfloat16)


def test_model_read_refusals_touch_nothing():
    pc.check_model_read_refusals(DEV)
