"""CPU: AuM-Tiny's padded x/dt layout (48 columns, rank 16, dim 384) on the lane-array build of the kernel sources (tests/emu) -- the
argument rules of csrc/xdt_args.h and aum_stream_block_tm shared with the device library, the binding's predicates, Mamba.stream_params
and the host composition of the one-launch block (tests/xdt_tiny_checks.py).  The device kernels are held to the same checks in
tests/test_gpu_xdt_tiny.py.  The lane-array build's aum_xdt_tm_fwd is a plain loop without the activation (the binding refuses
delta_softplus there), so the softplus form of the projection check runs on the device only.
On the commit before the feature every test here but the Base / Small plan check fails: the shape is refused (AUM_E_UNSUPPORTED, a False
predicate) and StreamParams has no b_off."""
import os
import sys

import pytest
import torch

import aum_hip
import xdt_tiny_checks as TC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("ntok", TC.NTOKS)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_xdt_tm_fwd_tiny_vs_unpadded_fp64(lib, dt, ntok):
    TC.check_xdt_fwd(lib, "cpu", ntok, dt, False)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_delta_does_not_see_the_pad_columns(lib, dt):
    TC.check_pad_columns_unread(lib, "cpu", 17, dt, False)


def test_supported_predicates_follow_the_dim_rule():
    """xdt_fwd_shape_ok as csrc/xdt_args.h states it: the three widths, dim % 128 == 0; the backward keeps its pairs and dim % 256"""
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    assert aum_hip.XDT_COLS_FWD == (80, 56, 48) and aum_hip.XDT_COLS_BWD == (80, 56)
    assert aum_hip.xdt_tm_supported(z(3, 384), z(48, 384), z(384, 16))
    assert aum_hip.xdt_tm_supported(z(3, 128), z(56, 128), z(128, 24)) and aum_hip.xdt_tm_supported(z(3, 640), z(80, 640), z(640, 48))
    assert not aum_hip.xdt_tm_supported(z(3, 384), z(44, 384), z(384, 12))          # the unpadded rows
    assert not aum_hip.xdt_tm_supported(z(3, 384), z(48, 384), z(384, 12))          # rank % 8
    assert not aum_hip.xdt_tm_supported(z(3, 320), z(48, 320), z(320, 16)) and not aum_hip.xdt_tm_supported(z(3, 192), z(48, 192), z(192, 16))
    assert not aum_hip.xdt_tm_supported(z(3, 384).float(), z(48, 384).float(), z(384, 16).float())
    assert not aum_hip.xdt_tm_bwd_widths(384, 16, 16, torch.bfloat16) and not aum_hip.xdt_tm_bwd_widths(384, 24, 16, torch.bfloat16)
    assert aum_hip.xdt_tm_bwd_widths(768, 24, 16, torch.bfloat16)


def test_c_check_agrees_with_the_binding(lib):
    """the raw entry point: (48, 16, 384) taken, dim 320 and the unpadded (44, 12) refused with AUM_E_UNSUPPORTED, nothing written"""
    def call(ncols, rank, dim):
        u, wx, wdt = torch.zeros(2, dim, dtype=torch.bfloat16), torch.zeros(ncols, dim, dtype=torch.bfloat16), torch.zeros(dim, max(rank, 8), dtype=torch.bfloat16)
        x, d = torch.full((2, 64), 7.0, dtype=torch.bfloat16), torch.full((2, dim), 7.0, dtype=torch.bfloat16)
        a = aum_hip.XdtArgs()
        a.u, a.wx, a.wdt, a.x_dbl, a.delta = (t.data_ptr() for t in (u, wx, wdt, x, d))
        a.ntok, a.dim, a.rank, a.ncols = 2, dim, rank, ncols
        a.ldu, a.ldwx, a.ldwdt, a.ldx, a.ldd, a.dtype = dim, dim, wdt.stride(0), 64, dim, aum_hip.AUM_BF16
        rc = lib.c.aum_xdt_tm_fwd(aum_hip.C_byref(a), None)
        return rc, bool((x == 7.0).all()) and bool((d == 7.0).all())
    assert call(48, 16, 384) == (0, False)
    assert call(48, 16, 320) == (-4, True) and call(44, 12, 384) == (-4, True) and call(48, 16, 192) == (-4, True)
    assert call(56, 24, 128)[0] == 0
    TC.check_scratch_bytes(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_single_sessions(lib, dt):
    for T in (1, 8, 9, 128):
        TC.check_block(dt, (T,), (0,), 2, lib, "cpu")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_ragged_pack(lib, dt):
    TC.check_block(dt, (1, 9, 128), (2, 0, 1), 4, lib, "cpu")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_vs_fp64(lib, dt):
    for T in (1, 8, 9, 128):
        TC.check_block_vs_oracle(dt, T, lib, "cpu")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stream_block_tiny_chunk_invariance(lib, dt):
    TC.check_chunk_invariance(dt, lib, "cpu")


def test_stream_block_refuses_the_unpadded_tiny_plan(lib):
    o = TC.operands("bf16", 8, 1, "cpu")
    p = o["plan"]
    plain = p._replace(w_x=torch.cat((p.w_x[:TC.R], p.w_x[TC.RP:])).contiguous(), w_dt=p.w_dt[:, :TC.R].contiguous())
    assert plain.w_x.shape == (44, TC.DIM)
    assert not aum_hip.stream_block_supported(o["x"], o["z"], o["conv"], o["state"], plain, 8)
    assert aum_hip.stream_block_supported(o["x"], o["z"], o["conv"], o["state"], p, 8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_stream_params_tiny_plan(dtype):
    TC.check_tiny_plan(dtype)


def test_stream_params_base_and_small_unpadded():
    TC.check_other_plans_unpadded()
