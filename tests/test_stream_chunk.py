"""CPU: chunked streaming inference (aum_conv1d_tm_chunk, aum_scan_tm_chunk, Mamba.step_chunk, AudioMamba.stream_*) on the lane-array
build of the kernel sources (tests/emu) -- the same checks tests/test_gpu_stream_chunk.py runs on the device library."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import aum_hip
import stream_checks as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")


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


@pytest.mark.parametrize("case", sc.SCAN_CASES, ids=sc.case_id)
def test_scan_chunk_vs_oracle(case, lib):
    sc.check_vs_oracle(sc.scan_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.scan_run, lib)


@pytest.mark.parametrize("case", sc.CONV_CASES, ids=sc.case_id)
def test_conv_chunk_vs_oracle(case, lib):
    sc.check_vs_oracle(sc.conv_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.conv_run, lib)


@pytest.mark.parametrize("case", sc.SCAN_CASES, ids=sc.case_id)
def test_scan_chunk_partition_is_bitwise(case, lib):
    sc.check_partition_bitwise(sc.scan_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.scan_run, lib)


@pytest.mark.parametrize("case", sc.CONV_CASES, ids=sc.case_id)
def test_conv_chunk_partition_is_bitwise(case, lib):
    sc.check_partition_bitwise(sc.conv_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.conv_run, lib)


@pytest.mark.parametrize("case", sc.SCAN_CASES, ids=sc.case_id)
def test_scan_chunk_vs_per_token_kernel(case, lib):
    sc.check_vs_per_token(sc.scan_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.scan_run, sc.scan_run_per_token, lib)


@pytest.mark.parametrize("case", sc.CONV_CASES, ids=sc.case_id)
def test_conv_chunk_vs_per_token_kernel(case, lib):
    sc.check_vs_per_token(sc.conv_setup(case, "cpu", batch=1 if case[0] > 64 else 2), sc.conv_run, sc.conv_run_per_token, lib)


def test_chunk_kernels_refuse_what_they_do_not_take(lib):
    st = torch.zeros(1, 48, 16)
    u = torch.zeros(1, 3, 48)
    assert not aum_hip.scan_tm_chunk_supported(st, u)                      # dim % 64
    with pytest.raises(RuntimeError, match="unsupported"):
        aum_hip.scan_tm_chunk(st, u, u, torch.zeros(48, 16), torch.zeros(1, 3, 16), torch.zeros(1, 3, 16), lib=lib)
    assert not aum_hip.conv1d_tm_chunk_supported(torch.zeros(1, 3, 8), torch.zeros(1, 8, 5))      # width > 4
    assert not aum_hip.conv1d_tm_chunk_supported(torch.zeros(1, 3, 6), torch.zeros(1, 6, 4))      # rows are not 16-byte multiples
    a = aum_hip.ScanTmChunkArgs()
    assert lib.c.aum_scan_tm_chunk(ctypes.byref(a), None) == -1           # AUM_E_NULL
    c = aum_hip.ConvTmChunkArgs()
    assert lib.c.aum_conv1d_tm_chunk(ctypes.byref(c), None) == -1


def test_shims_take_sequences_and_fall_back_token_by_token(emu_as_product):
    """causal_conv1d_update with (batch, dim, seqlen) and selective_scan_update at shapes the chunk kernels refuse (dim % 64, width 5)
    run the per-token kernels; at shapes they take, the chunk kernels: same numbers at the fp32 bar"""
    from causal_conv1d import causal_conv1d_update
    from mamba_ssm.ops.selective_scan_interface import selective_scan_update
    from conftest import rel_err
    torch.manual_seed(0)
    for dim, width in ((48, 5), (64, 4)):
        x = torch.randn(2, dim, 6)
        w, b = torch.randn(dim, width), torch.randn(dim)
        st = torch.randn(2, dim, width)
        st1 = st.clone()
        y = causal_conv1d_update(x, st, w, b, "silu")
        ys = torch.stack([causal_conv1d_update(x[:, :, t].contiguous(), st1, w, b, "silu") for t in range(6)], dim=2)
        assert y.shape == (2, dim, 6) and rel_err(y.numpy(), ys.numpy()) < 1e-4 and rel_err(st.numpy(), st1.numpy()) < 1e-4
        assert torch.equal(st[:, :, -1], x[:, :, -1])
    for dim in (48, 64):
        u, dl, z = torch.randn(2, 5, dim), torch.rand(2, 5, dim) * 0.2, torch.randn(2, 5, dim)
        Bm, Cm, A, D = torch.randn(2, 5, 16), torch.randn(2, 5, 16), -torch.rand(dim, 16), torch.randn(dim)
        s0 = torch.randn(2, dim, 16)
        s1 = s0.clone()
        y = selective_scan_update(s0, u, dl, A, Bm, Cm, D, z, torch.zeros(dim), True)
        ys = torch.stack([aum_hip.state_update(s1, u[:, t], dl[:, t], A, Bm[:, t], Cm[:, t], D, z[:, t], torch.zeros(dim), True) for t in range(5)], dim=1)
        assert y.shape == (2, 5, dim) and rel_err(y.numpy(), ys.numpy()) < 1e-4 and rel_err(s0.numpy(), s1.numpy()) < 1e-4


def test_mamba_forward_takes_chunks_after_prefill(emu_as_product):
    """fails on the parent commit: ValueError at the first 4-token chunk"""
    sc.check_mamba_chunks(32, "cpu")


def test_step_keeps_its_one_token_rule_and_bidirectional_blocks_refuse(emu_as_product):
    from mamba_ssm.modules.mamba_simple import Mamba
    m = Mamba(32, layer_idx=0, bimamba_type="none").eval()
    c, s = m.allocate_inference_cache(1, 0)
    with pytest.raises(ValueError, match="exactly one token"):
        m.step(torch.zeros(1, 2, 32), c, s)
    v1 = Mamba(32, layer_idx=0, bimamba_type="v1").eval()
    with pytest.raises(NotImplementedError):
        v1.step_chunk(torch.zeros(1, 2, 32), c, s)


def test_model_stream_matches_whole_clip(emu_as_product):
    sc.check_model_stream(64, "cpu")


def test_model_stream_rejects_non_causal_configurations(emu_as_product):
    sc.check_model_rejects("cpu")


def test_model_stream_push_checks_its_input(emu_as_product):
    model = sc.make_causal_aum(64, "cpu", depth=1)
    cache = model.allocate_inference_cache(1)
    with pytest.raises(ValueError, match="multiple of 16"):
        model.stream_push(torch.zeros(1, 24, 128), cache)
    model.stream_push(torch.zeros(1, 16 * 15, 128), cache)
    with pytest.raises(ValueError, match="do not fit"):
        model.stream_push(torch.zeros(1, 32, 128), cache)


def test_new_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the two new argument structs from a C program compiled against the header vs the ctypes mirrors"""
    probes = {
        "AumConvTmChunkArgs": (aum_hip.ConvTmChunkArgs, ["x", "conv_state", "weight", "bias", "y", "x_bs", "x_ts", "y_bs", "y_ts", "batch", "dim", "len",
                                                         "width", "dtype", "flags"]),
        "AumScanTmChunkArgs": (aum_hip.ScanTmChunkArgs, ["u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out", "u_bs", "u_ts", "delta_bs",
                                                         "delta_ts", "z_bs", "z_ts", "B_bs", "B_ts", "C_bs", "C_ts", "out_bs", "out_ts", "batch", "dim",
                                                         "len", "dstate", "dtype", "flags"]),
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
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert aum_hip.ABI_VERSION == 13 and {"aum_conv1d_tm_chunk", "aum_scan_tm_chunk"} <= set(aum_hip.EXPORTS)
