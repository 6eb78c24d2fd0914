"""CPU: aum_stream_block_tm / aum_hip.stream_block / Mamba.stream_params on the lane-array build of the kernel sources (tests/emu), where
the entry point is the host composition of the three existing entry points -- the ABI, the binding, the dispatch predicate and the
parameter cache; the kernel itself is held to the three launches on the device (tests/test_gpu_stream_block.py).  On the commit before
the feature every test here fails at the missing symbol / AttributeError."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import aum_hip
import stream_block_checks as bc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


def test_struct_layout_matches_header(tmp_path):
    cls = aum_hip.StreamBlockArgs
    lines = [f'printf("%zu\\n", sizeof(AumStreamBlockArgs));'] + [f'printf("%zu\\n", offsetof(AumStreamBlockArgs, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{ {" ".join(lines)} return 0; }}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]


def test_symbols_exported_abi_unchanged(lib):
    for name in ("aum_stream_block_tm", "aum_stream_block_scratch_bytes", "aum_stream_block_max_len"):
        assert name in aum_hip.EXPORTS and hasattr(lib.c, name)
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13
    assert lib.c.aum_stream_block_max_len() == aum_hip.STREAM_BLOCK_MAX_T >= 64
    assert lib.c.aum_stream_block_scratch_bytes(10, 256, 56) == 2 * 10 * (2 * 256 + 56)


def test_stream_block_equals_three_emulator_calls_ragged(lib):
    bc.check_fused_equals_three("small", "bf16", (3, 0, 17), (2, 0, 3), 4, lib, "cpu")
    bc.check_fused_equals_three("small", "bf16", (5, 2, 9), None, 4, lib, "cpu", null_idx=True)


def test_commit_false_is_honoured(lib):
    bc.check_no_commit("small", "bf16", lib, "cpu")


def test_refusals_touch_nothing(lib):
    bc.check_refusals(lib, "cpu")


def test_supported_truth_table():
    o = bc.operands("small", "bf16", 8, 2, "cpu")
    ok = lambda **kw: aum_hip.stream_block_supported(kw.get("x", o["x"]), kw.get("z", o["z"]), kw.get("conv", o["conv"]), kw.get("state", o["state"]),
                                                     kw.get("plan", o["plan"]), kw.get("max_len", 8))
    assert ok() and ok(max_len=bc.MAX_T) and not ok(max_len=bc.MAX_T + 1) and not ok(max_len=0)
    assert not ok(x=o["x"].float(), z=o["z"].float())
    assert not ok(x=o["x"].half())                                  # x and z of two dtypes
    assert not ok(conv=o["conv"].double()) and not ok(state=o["state"][:, :, :8].contiguous())
    assert not ok(conv=o["conv"][:1])                               # pools of two sizes
    assert not ok(x=o["x"][:, :192], z=o["z"][:, :192])             # dim % 256
    assert not ok(plan=o["plan"]._replace(w_x=o["plan"].w_x.half()))
    assert not ok(plan=o["plan"]._replace(w_x=o["plan"].w_x[:48]))  # an x_dbl width the kernels are not built for
    o2 = bc.operands("base", "f16", 4, 1, "cpu")
    assert aum_hip.stream_block_supported(o2["x"], o2["z"], o2["conv"], o2["state"], o2["plan"], 4)


def _mamba(dtype=torch.float32):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(4)
    return Mamba(64, bimamba_type="none", layer_idx=0).to(dtype)


def test_stream_params_cached_and_rebuilt():
    m = _mamba()
    p = m.stream_params()
    assert m.stream_params() is p and m.stream_params(torch.float32) is p
    assert m.stream_params(torch.bfloat16) is not p
    p = m.stream_params()
    with torch.no_grad():
        m.A_log.add_(1)                     # what an optimizer step does: an in-place write that moves _version
    q = m.stream_params()
    assert q is not p and torch.equal(q.A, -torch.exp(m.A_log.float()))
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    r = m.stream_params()
    assert r is not q and m.stream_params() is r
    m.half()
    h = m.stream_params()
    assert h is not r and h.dtype == torch.float16 and h.w_x.dtype == torch.float16 and h.A.dtype == torch.float32
    E = m.d_inner
    assert torch.equal(h.conv_w, m.conv1d.weight.float().reshape(E, -1)) and torch.equal(h.conv_b, m.conv1d.bias.float())
    assert torch.equal(h.A, -torch.exp(m.A_log.float())) and torch.equal(h.D, m.D.float()) and torch.equal(h.dt_bias, m.dt_proj.bias.float())
    assert torch.equal(h.w_x, m.x_proj.weight) and torch.equal(h.w_dt, m.dt_proj.weight)
    assert h.conv_w.data_ptr() % 16 == 0 and h.conv_w.is_contiguous()


def test_invalidate_stream_params_behind_a_data_write():
    """a write through p.data does not move _version, so the key cannot see it: invalidate_stream_params() is the way to say so"""
    m = _mamba()
    p = m.stream_params()
    m.D.data.add_(1)
    assert m.stream_params() is p
    m.invalidate_stream_params()
    q = m.stream_params()
    assert q is not p and torch.equal(q.D, m.D.float()) and m.stream_params() is q


def test_step_chunk_fp32_ladder_unchanged(lib):
    """the ladder path with the prepared parameters against the same computation with the per-call conversions written out"""
    import torch.nn.functional as F
    m = _mamba()
    old, aum_hip._product = aum_hip._product, lib
    try:
        torch.manual_seed(8)
        h = torch.randn(2, 5, 64)
        c, s = torch.randn(2, m.d_inner, 4), torch.randn(2, m.d_inner, 16) * 0.3
        c2, s2 = c.clone(), s.clone()
        with torch.no_grad():
            out, _, _ = m.step_chunk(h, c, s)
            E, N, R = m.d_inner, m.d_state, m.dt_rank
            xz = m.in_proj(h.reshape(10, -1)).view(2, 5, 2 * E)
            x, z = xz[..., :E], xz[..., E:]
            xc = aum_hip.conv1d_stream(x, c2, m.conv1d.weight.view(E, m.d_conv), m.conv1d.bias, True, None).contiguous()
            proj = m.x_proj(xc.reshape(10, E))
            delta = F.linear(proj[:, :R], m.dt_proj.weight)
            proj = proj.view(2, 5, -1)
            y = aum_hip.scan_stream(s2, xc, delta.view(2, 5, E), -torch.exp(m.A_log.float()), proj[..., R:R + N], proj[..., R + N:R + 2 * N], m.D, z,
                                    m.dt_proj.bias, True, False, None)
            ref = m.out_proj(y.reshape(10, E)).view(2, 5, -1)
        assert torch.equal(out, ref) and torch.equal(c, c2) and torch.equal(s, s2)
        with pytest.raises(NotImplementedError):
            m.step_chunk(h, c, s, commit=False)
    finally:
        aum_hip._product = old
