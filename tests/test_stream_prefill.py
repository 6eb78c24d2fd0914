"""CPU: streaming prefill on the lane-array build of the kernel sources (tests/emu) -- aum_scan_tm_fwd_state (state in / state out of the
token-major scan, uncut and in time segments), aum_hip.conv1d_tm_prefill, Mamba.prefill_chunk and AudioMamba.stream_prefill(_many): the
checks of tests/stream_prefill_checks.py, which tests/test_gpu_stream_prefill.py runs on the device.  On the commit before the feature
61 of the 62 tests fail at the missing symbol / AttributeError (run there); one passes, because it runs code that already existed:
test_state_bar_is_twice_the_chunk_kernels_error, the yardstick (aum_scan_tm_chunk against the oracle).  test_forward_offset0_then_steps
exercises the un-fused branch, which Mamba.forward at offset 0 keeps for host tensors -- the new path is a device path, held in
tests/test_gpu_stream_prefill.py -- and fails on the parent only because it asks which path ran."""
import ctypes
import os
import subprocess
import sys

import pytest

import aum_hip
import stream_prefill_checks as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


def test_struct_layout_matches_header(tmp_path):
    cls = aum_hip.ScanTmFwdStateArgs
    lines = ['printf("%zu\\n", sizeof(AumScanTmFwdStateArgs));'] + [f'printf("%zu\\n", offsetof(AumScanTmFwdStateArgs, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{ {" ".join(lines)} return 0; }}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]


def test_symbol_exported_abi_unchanged(lib):
    assert "aum_scan_tm_fwd_state" in aum_hip.EXPORTS and hasattr(lib.c, "aum_scan_tm_fwd_state")
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13


def test_state_bar_is_twice_the_chunk_kernels_error(lib):
    """the yardstick behind STATE_BAR, measured again: the existing aum_scan_tm_chunk's exit state against the fp64 oracle at this file's shapes"""
    worst = pc.chunk_state_error(lib, "cpu")
    print(f"worst rel_err of the scan_tm_chunk state: {worst:.3e}; recorded {pc.CHUNK_STATE_ERR:.3e}; STATE_BAR {pc.STATE_BAR:.3e}")
    assert worst <= pc.CHUNK_STATE_ERR * 1.0001 and pc.STATE_BAR == 2 * pc.CHUNK_STATE_ERR


@pytest.mark.parametrize("c", pc.KERNEL_CASES + pc.SEG_CASES, ids=pc.kcase_id)
def test_kernel_handoff(lib, c):
    pc.check_kernel_handoff(c, lib, "cpu")


def test_refusals(lib):
    pc.check_refusals(lib, "cpu")


@pytest.mark.parametrize("T,dt,kind", [(9, "f32", pc.KINDS[0]), (9, "bf16", pc.KINDS[1]), (129, "f16", pc.KINDS[5]), (129, "bf16", pc.KINDS[3])])
def test_partition_uncut_bitwise(lib, T, dt, kind):
    pc.check_partition_uncut(T, dt, kind, lib, "cpu")


@pytest.mark.parametrize("cut,seg", [(512, 2), (300, 2), (1000, 2), (512, 8), (333, 8)])
def test_partition_segmented(lib, cut, seg):
    pc.check_partition_segmented(("bf16", "f32")[seg == 8], pc.KINDS[0], cut, seg, lib, "cpu")


@pytest.mark.parametrize("case", pc.CONV_CASES, ids=pc.sc.case_id)
def test_conv_prefill(lib, case):
    pc.check_conv_prefill(case, lib, "cpu")


@pytest.mark.parametrize("d_model,dt_rank,dt,T,batch", [(32, "auto", "f32", 1, 1), (32, "auto", "f16", 3, 3), (32, "auto", "f32", 7, 3), (128, 24, "bf16", 8, 1),
                                                        (128, 24, "bf16", 9, 1), (128, 24, "f16", 64, 3), (32, "auto", "bf16", 129, 1),
                                                        (32, "auto", "f32", 513, 1)])
def test_mamba_prefill_then_live(lib, d_model, dt_rank, dt, T, batch):
    pc.check_mamba_handover(d_model, dt_rank, dt, T, batch, lib, "cpu")


def test_model_prefill_then_push(lib):
    pc.check_model_prefill(lib, "cpu")


def test_model_prefill_many(lib):
    pc.check_model_prefill_many(lib, "cpu")


def test_model_refusals_touch_nothing(lib):
    pc.check_model_refusals(lib, "cpu")


def test_forward_offset0_then_steps(lib):
    """host tensors: the un-fused branch (checked inside), whose caches step() must continue from as before"""
    assert pc.check_forward_offset0(32, lib, "cpu") is False
