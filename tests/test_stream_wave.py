"""CPU: streaming from raw audio (aum_fbank_stream_fwd, aum_hip.fbank_stream / wave_map, AudioMamba.stream_push_wave*) on the
lane-array build of the kernel sources (tests/emu) -- the checks tests/test_gpu_stream_wave.py runs on the device library, the struct
layout against the header, and the DC-offset residual against the fp64 oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aum_hip
import stream_wave_checks as wc

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


def test_any_cut_gives_the_same_bits(lib):
    wc.check_any_cut("cpu", lib)


def test_sessions_are_independent_and_other_rows_untouched(lib):
    wc.check_independence("cpu", lib)


def test_end_of_clip(lib, emu_as_product):
    wc.check_end("cpu", lib)


def test_read_with_the_push(lib, emu_as_product):
    wc.check_read("cpu", lib)


def test_refusals_leave_no_trace(lib, emu_as_product):
    wc.check_refusals("cpu", lib)


def test_entry_point_codes(lib):
    wc.check_c_codes(lib)


def test_product_library_refuses_host_tensors():
    import importlib.util
    spec = importlib.util.spec_from_file_location("aum_build", os.path.join(ROOT, "audio-mamba-aum_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    product = aum_hip.Lib(mod.build())
    m = aum_hip.wave_map([100], [0], [0], [0], [-1], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        aum_hip.fbank_stream(torch.zeros(100), m, torch.zeros(1, wc.CAP), wc.tables("cpu").tables, wc.MEAN, wc.STD, lib=product)


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of AumFbankStreamArgs from a C program compiled against the header vs the ctypes mirror"""
    fields = ["fbank", "cu_samples", "cu_frames", "tail_len", "idx", "first_frame", "n_real", "tails", "total_samples", "total_frames", "nseq", "nrows",
              "cap", "reserved"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(AumFbankStreamArgs));']
    lines += [f'printf("{f} %zu\\n", offsetof(AumFbankStreamArgs, {f}));' for f in fields] + ['return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(aum_hip.FbankStreamArgs)
    assert [f for f, _ in aum_hip.FbankStreamArgs._fields_] == fields
    for f in fields:
        assert int(got[f]) == getattr(aum_hip.FbankStreamArgs, f).offset, f
    assert aum_hip.ABI_VERSION == 13 and "aum_fbank_stream_fwd" in aum_hip.EXPORTS


DC_RESIDUAL = 6.96e-05     # measured on the lane-array build ("Streaming log-mel"); the assertion allows twice that


def test_dc_offset_residual(lib):
    """8: a stream cannot subtract the clip's mean as the offline loader does; the kernel removes each frame's own mean first.  A 440 Hz
    tone with a DC offset of 0.05 of full scale, streamed in fp32, against oracle/fbank.py in fp64 (which removes the clip mean): the
    largest difference of a normalised log-mel value is deterministic (fixed summation order) and held to twice the measured value."""
    from oracle import fbank as OF
    n = wc.WIN + 95 * wc.SHIFT
    t = np.arange(n) / 16000.0
    tone = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.05).astype(np.float32)
    m = aum_hip.wave_map([n], [0], [96], [0], [-1], device="cpu")
    tails = torch.zeros(1, wc.CAP)
    got = aum_hip.fbank_stream(torch.tensor(tone), m, tails, wc.tables("cpu").tables, wc.MEAN, wc.STD, lib=lib).numpy()
    ref = OF.frontend(tone.astype(np.float64), target_length=96)
    flat = aum_hip.fbank_stream(torch.tensor(tone - np.float32(0.05)), m, tails, wc.tables("cpu").tables, wc.MEAN, wc.STD, lib=lib).numpy()
    err, err_flat = float(np.abs(got - ref).max()), float(np.abs(flat - OF.frontend((tone - np.float32(0.05)).astype(np.float64), target_length=96)).max())
    print(f"DC offset 0.05: max |stream fp32 - oracle fp64| = {err:.6e} (the same tone without the offset: {err_flat:.6e})")
    assert err <= 2 * DC_RESIDUAL
