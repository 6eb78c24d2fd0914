"""CPU: many streaming sessions at different positions in one call (aum_conv1d_tm_chunk_var, aum_scan_tm_chunk_var, aum_hip.seq_map,
Mamba.step_chunk(seq_map=), AudioMamba.stream_push_many / allocate_stream_pool / stream_read(sessions=) / stream_reset) on the
lane-array build of the kernel sources (tests/emu) -- the same checks tests/test_gpu_stream_pool.py runs on the device library.
On the commit before the feature every test here fails at the missing symbols / AttributeError."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import aum_hip
import stream_checks as sc
import stream_pool_checks as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")
OPS = {"scan": (pc.ScanOp, sc.SCAN_CASES), "conv": (pc.ConvOp, sc.CONV_CASES)}
ALL = [(name, c) for name, (_, cases) in OPS.items() for c in cases]
_id = lambda p: f"{p[0]}-{sc.case_id(p[1])}"


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


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_packed_sessions_equal_batch1_calls_bitwise(p, lib):
    pc.check_packing_bitwise(OPS[p[0]][0], p[1], lib, "cpu")


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_packed_calls_vs_oracle(p, lib):
    pc.check_var_vs_oracle(OPS[p[0]][0], p[1], lib, "cpu")


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_null_state_indices_is_the_identity_mapping(p, lib):
    pc.check_null_indices(OPS[p[0]][0], p[1], lib, "cpu")


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_out_of_range_index_is_a_no_op(p, lib):
    pc.check_out_of_range_index(OPS[p[0]][0], p[1], lib)


def test_seq_map_validates_on_the_host(emu_as_product):
    pc.check_seq_map_validates("cpu")


def test_var_launchers_refuse_what_they_do_not_take(lib):
    m = aum_hip.seq_map([3], None, device="cpu")
    st, u = torch.zeros(1, 48, 16), torch.zeros(3, 48)
    assert not aum_hip.scan_tm_chunk_var_supported(st, u)                   # dim % 64
    with pytest.raises(RuntimeError, match="unsupported"):
        aum_hip.scan_tm_chunk_var(st, u, u, torch.zeros(48, 16), torch.zeros(3, 16), torch.zeros(3, 16), seq_map=m, lib=lib)
    assert not aum_hip.conv1d_tm_chunk_var_supported(torch.zeros(3, 8), torch.zeros(1, 8, 5))     # width > 4
    assert not aum_hip.conv1d_tm_chunk_var_supported(torch.zeros(3, 6), torch.zeros(1, 6, 4))     # rows are not 16-byte multiples
    assert lib.c.aum_scan_tm_chunk_var(ctypes.byref(aum_hip.ScanTmChunkVarArgs()), None) == -1    # AUM_E_NULL
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(aum_hip.ConvTmChunkVarArgs()), None) == -1
    # a complete conv call, then one field wrong at a time
    x, y, cs, w = torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(1, 8, 4), torch.zeros(8, 4)

    def conv_args(**over):
        a = aum_hip.ConvTmChunkVarArgs()
        a.x, a.conv_state, a.weight, a.y, a.cu_seqlens = x.data_ptr(), cs.data_ptr(), w.data_ptr(), y.data_ptr(), m.cu.data_ptr()
        a.x_ts = a.y_ts = 8
        a.total, a.nseq, a.nrows, a.dim, a.width = 3, 1, 1, 8, 4
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args()), None) == 0
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(cu_seqlens=None)), None) == -1
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(nseq=0)), None) == -2
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(nrows=0)), None) == -2
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(total=0)), None) == -2
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(cu_seqlens=m.cu.data_ptr() + 2)), None) == -4
    assert lib.c.aum_conv1d_tm_chunk_var(ctypes.byref(conv_args(total=1 << 30, x_ts=1 << 20)), None) == -4   # byte cursors are 32-bit


def test_shims_take_packed_sessions_and_fall_back_per_session(emu_as_product):
    """causal_conv1d_update / selective_scan_update with seq_map: at shapes the var kernels take and at shapes they refuse (dim % 64,
    width 5: a host loop over the sessions) = every session through the same function on its own"""
    from causal_conv1d import causal_conv1d_update
    from mamba_ssm.ops.selective_scan_interface import selective_scan_update
    from conftest import rel_err
    torch.manual_seed(0)
    lens, rows = (2, 0, 3, 1), (3, 1, 4, 0)
    m = aum_hip.seq_map(lens, rows, device="cpu")
    for dim, width in ((48, 5), (64, 4)):
        x = torch.randn(1, dim, 6)
        w, b = torch.randn(dim, width), torch.randn(dim)
        st = torch.randn(5, dim, width)
        st1 = st.clone()
        y = causal_conv1d_update(x, st, w, b, "silu", seq_map=m)
        o = 0
        for n, r in zip(lens, rows):
            if n:
                ys = causal_conv1d_update(x[:, :, o:o + n].contiguous(), st1[r:r + 1], w, b, "silu")
                assert rel_err(y[:, :, o:o + n].numpy(), ys.numpy()) < 1e-4
            o += n
        assert y.shape == (1, dim, 6) and rel_err(st.numpy(), st1.numpy()) < 1e-4 and torch.equal(st[2], st1[2])
    for dim in (48, 64):
        u, dl, z = torch.randn(1, 6, dim), torch.rand(1, 6, dim) * 0.2, torch.randn(1, 6, dim)
        Bm, Cm, A, D = torch.randn(1, 6, 16), torch.randn(1, 6, 16), -torch.rand(dim, 16), torch.randn(dim)
        s0 = torch.randn(5, dim, 16)
        s1 = s0.clone()
        y = selective_scan_update(s0, u, dl, A, Bm, Cm, D, z, torch.zeros(dim), True, seq_map=m)
        o = 0
        for n, r in zip(lens, rows):
            if n:
                ys = selective_scan_update(s1[r:r + 1], u[:, o:o + n], dl[:, o:o + n], A, Bm[:, o:o + n], Cm[:, o:o + n], D, z[:, o:o + n],
                                           torch.zeros(dim), True)
                assert rel_err(y[:, o:o + n].numpy(), ys.numpy()) < 1e-4
            o += n
        assert y.shape == (1, 6, dim) and rel_err(s0.numpy(), s1.numpy()) < 1e-4 and torch.equal(s0[2], s1[2])
    with pytest.raises(ValueError, match="pool has 5 rows"):
        causal_conv1d_update(torch.zeros(1, 64, 6), torch.zeros(5, 64, 4), torch.zeros(64, 4), seq_map=aum_hip.seq_map(lens, (0, 1, 2, 5), device="cpu"))


def test_bad_map_raises_at_every_entry_and_is_checked_once(lib, emu_as_product, monkeypatch):
    """a direct aum_hip.*_var call with a map that is no SeqMap, of another stream or naming a row outside the pool raises what it always
    raised and leaves the pool alone; Mamba.step_chunk(seq_map=) checks its map once for both recurrent stages"""
    from mamba_ssm.modules.mamba_simple import Mamba
    dim = 64
    u, bc, A, w = torch.randn(3, dim), torch.randn(3, 16), -torch.rand(dim, 16), torch.randn(dim, 4)
    for bad, exc in (((1, 2), TypeError), (aum_hip.seq_map([1, 3], None, device="cpu"), ValueError),
                     (aum_hip.seq_map([1, 2], [0, 2], device="cpu"), ValueError)):
        st, cs = torch.randn(2, dim, 16), torch.randn(2, dim, 4)
        st0, cs0 = st.clone(), cs.clone()
        with pytest.raises(exc):
            aum_hip.scan_tm_chunk_var(st, u, u, A, bc, bc, seq_map=bad, lib=lib)
        with pytest.raises(exc):
            aum_hip.conv1d_tm_chunk_var(u, cs, w, seq_map=bad, lib=lib)
        assert torch.equal(st, st0) and torch.equal(cs, cs0)
    calls = []
    real = aum_hip.check_seq_map
    monkeypatch.setattr(aum_hip, "check_seq_map", lambda *a: (calls.append(a[0]), real(*a))[1])
    m = Mamba(32, layer_idx=0, bimamba_type="none").eval()
    conv_pool, ssm_pool = m.allocate_inference_cache(3, 0, dtype=torch.float32)
    with torch.no_grad():
        m.step_chunk(torch.randn(1, 5, 32), conv_pool, ssm_pool, seq_map=aum_hip.seq_map([2, 3], [2, 0], device="cpu"))
    assert calls == ["step_chunk"]


def test_mamba_step_chunk_takes_packed_sessions(emu_as_product):
    pc.check_mamba_pool(32, "cpu")          # d_inner = 64: the var kernels


def test_mamba_step_chunk_packed_sessions_fallback(emu_as_product):
    pc.check_mamba_pool(24, "cpu")          # d_inner = 48: the scan falls back to a host loop over the sessions


def test_model_pool_matches_whole_clips_fp32(emu_as_product):
    pc.check_model_pool(64, "cpu")


def test_model_pool_matches_whole_clips_bf16_autocast(emu_as_product):
    pc.check_model_pool(64, "cpu", autocast_dtype=torch.bfloat16)


def test_var_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the two new argument structs from a C program compiled against the header vs the ctypes mirrors"""
    probes = {
        "AumConvTmChunkVarArgs": (aum_hip.ConvTmChunkVarArgs, ["x", "conv_state", "weight", "bias", "y", "cu_seqlens", "state_indices", "x_ts", "y_ts",
                                                            "total", "nseq", "nrows", "dim", "width", "dtype", "flags"]),
        "AumScanTmChunkVarArgs": (aum_hip.ScanTmChunkVarArgs, ["u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out", "cu_seqlens",
                                                            "state_indices", "u_ts", "delta_ts", "z_ts", "B_ts", "C_ts", "out_ts", "total", "nseq",
                                                            "nrows", "dim", "dstate", "dtype", "flags"]),
    }
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, (cls, fields) in probes.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        assert [f for f, _ in cls._fields_] == fields
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert aum_hip.ABI_VERSION == 13 and {"aum_conv1d_tm_chunk_var", "aum_scan_tm_chunk_var"} <= set(aum_hip.EXPORTS)
