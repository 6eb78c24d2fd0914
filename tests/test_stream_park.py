"""CPU: parking and resuming streaming sessions (aum_stream_park, aum_hip.stream_park / stream_park_layout / row_map,
AudioMamba.stream_park / stream_resume / stream_fork, ParkedSessions) on the lane-array build of the kernel sources (tests/emu), host
tensors -- the checks tests/test_gpu_stream_park.py runs on the device library -- plus the struct layout against the header and the
un-fused twin.  On the commit before the feature every test here fails: the entry point and the methods do not exist."""
import ctypes
import os
import subprocess
import sys

import pytest

import aum_hip
import stream_park_checks as pk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


def test_kernel_raw(lib):
    pk.check_kernel_raw(lib, "cpu")


def test_binding_on_strided_pools(lib):
    pk.check_binding(lib, "cpu")


@pytest.mark.parametrize("to_host", [False, True], ids=["device_blob", "to_host"])
def test_continuation_is_exact_fp32(lib, to_host):
    pk.check_continuation(lib, "cpu", to_host=to_host)


def test_neighbours_untouched(lib):
    pk.check_neighbours(lib, "cpu")


def test_fork(lib):
    pk.check_fork(lib, "cpu")


def test_raw_audio_session_moves_with_its_tail(lib):
    pk.check_wave(lib, "cpu")


def test_refusals_change_nothing(lib):
    pk.check_refusals(lib, "cpu")


def test_one_launch_each_way(lib):
    pk.check_one_launch(lib, "cpu")


def test_twin_gives_the_same_bytes(lib):
    pk.check_twin(lib)


def test_product_library_refuses_host_tensors():
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("aum_build", os.path.join(ROOT, "audio-mamba-aum_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    product = aum_hip.Lib(mod.build())
    pool = torch.ones(2, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        aum_hip.stream_park([pool], [1], lib=product)


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of AumParkArgs from a C program compiled against the header vs the ctypes mirror; no version step"""
    fields = ["base", "row_stride", "row_bytes", "blob_off", "rows", "blob", "blob_stride", "n_tensors", "n_sessions", "flags"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(AumParkArgs));', 'printf("max %d\\n", AUM_PARK_MAX_TENSORS);', 'printf("restore %u\\n", AUM_PARK_RESTORE);']
    lines += [f'printf("{f} %zu\\n", offsetof(AumParkArgs, {f}));' for f in fields] + ['return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(aum_hip.ParkArgs)
    assert int(got["max"]) == aum_hip.PARK_MAX_TENSORS == 64 and int(got["restore"]) == aum_hip.PARK_RESTORE
    assert [f for f, _ in aum_hip.ParkArgs._fields_] == fields
    for f in fields:
        assert int(got[f]) == getattr(aum_hip.ParkArgs, f).offset, f
    assert aum_hip.ABI_VERSION == 13 and "aum_stream_park" in aum_hip.EXPORTS
