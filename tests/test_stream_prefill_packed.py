"""CPU: PACKED streaming prefill on the lane-array build of the kernel sources (tests/emu) -- aum_conv1d_tm_prefill_var,
aum_scan_tm_fwd_state_var (uncut and cut into ranges), Mamba.prefill_chunk(seq_map=) and AudioMamba.stream_prefill_many(packed=True):
the checks of tests/stream_prefill_packed_checks.py, which tests/test_gpu_stream_prefill_packed.py runs on the device.
On the commit before the feature every test of this file fails (run there, on the parent's own lane-array build: 93 failed, 0 passed
of 93) -- at the missing ctypes struct, binding function or symbol (AttributeError), or at the unknown `packed` / `seq_map` keyword
(TypeError).  No test of this file passes on the parent.  The 34 tests of tests/test_gpu_stream_prefill_packed.py run the same checks
and fail there the same way."""
import ctypes
import os
import subprocess
import sys

import pytest

import aum_hip
import stream_checks as sc
import stream_prefill_checks as pc
import stream_prefill_packed_checks as pk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")
DTS = ("f32", "bf16", "f16")


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("name", ["ConvTmPrefillVarArgs", "ScanTmFwdStateVarArgs"])
def test_struct_layout_matches_header(tmp_path, name):
    cls = getattr(aum_hip, name)
    lines = [f'printf("%zu\\n", sizeof(Aum{name}));'] + [f'printf("%zu\\n", offsetof(Aum{name}, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{ {" ".join(lines)} return 0; }}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]


def test_symbols_exported_abi_unchanged(lib):
    for name in ("aum_conv1d_tm_prefill_var", "aum_scan_tm_fwd_state_var", "aum_scan_tm_fwd_state_var_carry_bytes"):
        assert name in aum_hip.EXPORTS and hasattr(lib.c, name)
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13


def test_var_range_rule():
    """scan_tm_segments with batch := sessions, length := the longest: no cut below 1024 steps or at one wave per two SIMDs and more"""
    f = lambda lens, dim: aum_hip.scan_tm_var_range(lens, dim, nsimd=1024)
    assert f((1023, 5), 1536) == 0 and f((4097,) * 32, 1536) == 0 and f((), 64) == 0
    assert f((4097, 2048, 9), 1536) == 136           # 3 sessions x 24 groups = 72 waves: 32 ranges (the cap), ceil(4097 / 32) = 129 -> 136
    r = f((1024,), 1536)
    assert r == 128 and r % aum_hip.SCAN_TM_CK == 0  # ranges no shorter than 128 steps: 8 of them


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k", [0, 2, 3, 5])
def test_conv(lib, dt, dim, k):
    pk.check_conv(dt, sc.CONV_KINDS[k], dim, lib, "cpu")


@pytest.mark.parametrize("dt", DTS)
def test_conv_zero_window(lib, dt):
    pk.check_conv(dt, sc.CONV_KINDS[0], 72, lib, "cpu", zero_window=True)


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_scan_uncut(lib, dt, dim, k):
    kind = pc.KINDS[k]
    if dt == "f32" and kind[0] == "act":
        kind = ("sp",) + kind[1:]
    pk.check_scan(dt, kind, dim, lib, "cpu", pk.SCAN_LENS, state_oracle=pk.session_state_oracle(dt, kind, dim, "cpu", pk.SCAN_LENS))


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k", [0, 1, 3])
def test_scan_cut_coinciding_ranges(lib, dt, dim, k):
    kind = pc.KINDS[k]
    if dt == "f32" and kind[0] == "act":
        kind = ("sp",) + kind[1:]
    for L in pk.CUT_LENS:            # scant_seg_len(L, ceil(L / 8)) == 8: the session's own cut has the pack's ranges
        assert L == 0 or -(-(-(-L // -(-L // 8))) // 8) * 8 == 8
    pk.check_scan(dt, kind, dim, lib, "cpu", pk.CUT_LENS, range_len=8, state_oracle=pk.session_state_oracle(dt, kind, dim, "cpu", pk.CUT_LENS))


@pytest.mark.parametrize("dt", DTS)
def test_scan_cut_other_ranges(lib, dt):
    """513 + 130 rows in ranges of 128: the sessions' own cuts have other ranges -- the oracle bars only"""
    kind = pc.KINDS[0]
    lens = (513, 130)
    pk.check_scan(dt, kind, 64, lib, "cpu", lens, range_len=128, bitwise=False, state_oracle=pk.session_state_oracle(dt, kind, 64, "cpu", lens))


def test_scan_cut_1024_in_8(lib):
    """fp32, 1024 steps cut in 8: the shape where the fixed-batch kernel's state error was largest"""
    kind = pc.KINDS[3]
    lens = (1024, 300)
    pk.check_scan("f32", kind, 64, lib, "cpu", lens, range_len=128, bitwise=False, state_oracle=pk.session_state_oracle("f32", kind, 64, "cpu", lens))


@pytest.mark.parametrize("dt,range_len", [("f32", 0), ("bf16", 0), ("f16", 8), ("bf16", 16)])
def test_packing_invariance_scan(lib, dt, range_len):
    pk.check_packing_invariance(dt, pc.KINDS[0], 64, lib, "cpu", range_len)


@pytest.mark.parametrize("dt", DTS)
def test_packing_invariance_conv(lib, dt):
    pk.check_conv_packing_invariance(dt, 72, lib, "cpu")


def test_refusals(lib):
    pk.check_refusals(lib, "cpu")


@pytest.mark.parametrize("d_model,dt_rank", [(128, 24), (32, "auto")])
@pytest.mark.parametrize("dt", DTS)
def test_block(lib, d_model, dt_rank, dt):
    pk.check_block(d_model, dt_rank, dt, lib, "cpu")


def test_model_packed_prefill(lib):
    pk.check_model(lib, "cpu")


def test_model_refusals_touch_nothing(lib):
    pk.check_model_refusals(lib, "cpu")
