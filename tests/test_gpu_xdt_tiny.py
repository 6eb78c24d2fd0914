"""GPU: AuM-Tiny's padded x/dt layout (48 columns, rank 16, dim 384) on the device kernels -- k_xdt_tm_fwd at NC = 48 and the NC = 48
instantiations of k_stream_block -- against fp64 products of the UNPADDED weights, the three launches (bit for bit), the fp64
restatement of the block, and the padding's exactness (tests/xdt_tiny_checks.py); the relaxed dim rule (dim % 128) at the widths the
kernel had before; and a Tiny Mamba block on the one-launch path.
On the commit before the feature every test here fails: the shapes are refused."""
import pytest
import torch

import aum_hip
import xdt_tiny_checks as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("softplus", [False, True], ids=["raw", "softplus"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_xdt_tm_fwd_tiny_vs_unpadded_fp64(lib, dt, softplus):
    for ntok in TC.NTOKS:
        TC.check_xdt_fwd(lib, DEV, ntok, dt, softplus)


@pytest.mark.parametrize("softplus", [False, True], ids=["raw", "softplus"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_delta_does_not_see_the_pad_columns(lib, dt, softplus):
    for ntok in (17, 129):
        TC.check_pad_columns_unread(lib, DEV, ntok, dt, softplus)


@pytest.mark.parametrize("ncols,rank,dim", [(56, 24, 128), (56, 24, 640), (80, 48, 384), (48, 16, 128), (48, 16, 1536)],
                         ids=lambda v: str(v))
def test_xdt_tm_fwd_dim_rule(lib, ncols, rank, dim):
    """dim / 64 steps: 2 (one short round), 10 and 6 (full rounds, then a short one), 24 (full rounds only: the shape rule's upper end)"""
    for dt in ("bf16", "f16"):
        TC.check_xdt_fwd_other_width(lib, DEV, ncols, rank, dim, 129, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_single_sessions(lib, dt):
    for T in (1, 8, 9, 128):
        TC.check_block(dt, (T,), (0,), 2, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_ragged_pack(lib, dt):
    TC.check_block(dt, (1, 9, 128), (2, 0, 1), 4, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_vs_fp64(lib, dt):
    for T in (1, 8, 9, 33, 128):
        TC.check_block_vs_oracle(dt, T, lib, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_chunk_invariance(lib, dt):
    TC.check_chunk_invariance(dt, lib, DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_tiny_block_takes_the_one_launch_path(dtype):
    """step_chunk on a Tiny block: one aum_hip.stream_block call and no ladder stage, for a plain hop, commit=False (returns instead of
    raising NotImplementedError, caches untouched) and peek=True; the ladder (aum_hip.debug.stream_fused off) gives the same bits"""
    m = TC.tiny_block(dtype, DEV)
    torch.manual_seed(3)
    h = torch.randn(2, 9, 192, device=DEV).to(dtype)
    with torch.no_grad():
        c, s = m.allocate_inference_cache(2, 0, dtype=torch.float32)
        c.copy_(torch.randn(c.shape)), s.copy_(torch.randn(s.shape) * 0.3)
        c0, s0 = c.clone(), s.clone()
        with TC.count_calls("stream_block", "conv1d_stream", "scan_stream", "xdt_tm_fwd") as n:
            y0, _, _ = m.step_chunk(h, c, s, commit=False)
            assert torch.equal(c, c0) and torch.equal(s, s0)
            yp, _, _ = m.step_chunk(h, c0.clone(), s0.clone(), peek=True)
            y, _, _ = m.step_chunk(h, c, s)
        assert n == {"stream_block": 3, "conv1d_stream": 0, "scan_stream": 0, "xdt_tm_fwd": 0}, n
        assert torch.equal(y, y0) and not torch.equal(s, s0)
        old, aum_hip.debug.stream_fused = aum_hip.debug.stream_fused, False
        try:
            cl, sl = c0.clone(), s0.clone()
            with TC.count_calls("stream_block", "conv1d_stream", "scan_stream", "xdt_tm_fwd") as n:
                yl, _, _ = m.step_chunk(h, cl, sl)
                ylp, _, _ = m.step_chunk(h, c0.clone(), s0.clone(), peek=True)
            assert n == {"stream_block": 0, "conv1d_stream": 2, "scan_stream": 2, "xdt_tm_fwd": 2}, n
        finally:
            aum_hip.debug.stream_fused = old
        assert torch.equal(yl, y) and torch.equal(cl, c) and torch.equal(sl, s) and torch.equal(ylp, yp)
