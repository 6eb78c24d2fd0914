"""CPU: a streaming hop through all blocks in one library call (aum_stream_in_tm, aum_stream_out_tm, aum_stream_layers,
AudioMamba.stream_stack) on the lane-array build of the kernel sources (tests/emu), host tensors -- the checks
tests/test_gpu_stream_stack.py runs on the device library -- plus the conditions of the exact-input cases on the fp64 reference alone and
the struct layouts against the header.  On the commit before the feature every test here fails: the entry points and the methods do not exist."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import aum_hip
import stream_stack_checks as ss

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aum_hip.h")
WID = lambda w: f"{w[0]}x{w[1]}"


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_exact_input_conditions(widths, dtype):
    """the conditions of the exact-input cases, on the fp64 reference alone, at every total the device test uses"""
    ss.pooled_conditions(widths, dtype)
    for total in ss.TOTALS:
        ss.out_conditions(widths, dtype, total)
        ss.in_conditions(widths, dtype, total)


@pytest.mark.parametrize("with_res", [False, True], ids=["first_block", "residual"])
@pytest.mark.parametrize("total", [1, 17, 73])
@pytest.mark.parametrize("widths", ss.WIDTHS, ids=WID)
def test_norm_prologue_bitwise(lib, widths, total, with_res):
    ss.check_norm_prologue(lib, "cpu", widths, torch.bfloat16, total, with_res)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
@pytest.mark.parametrize("widths", ss.WIDTHS[:2], ids=WID)
def test_exact_inputs(lib, widths, dtype):
    for total in (1, 17):
        ss.check_out_exact(lib, "cpu", widths, dtype, total)
        ss.check_in_exact(lib, "cpu", widths, dtype, total)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=ss.gx.dt_id)
def test_random_inputs_interval(lib, dtype):
    ss.check_out_interval(lib, "cpu", ss.WIDTHS[0], dtype, 17)
    ss.check_in_interval(lib, "cpu", ss.WIDTHS[0], dtype, 17)


def test_partition_bitwise(lib):
    ss.check_partition(lib, "cpu", ss.WIDTHS[0], torch.bfloat16)


@pytest.mark.parametrize("mode", ["commit", "peek", "no_commit"])
@pytest.mark.parametrize("map_name", sorted(ss.MAPS))
def test_chain_is_the_composition(lib, map_name, mode):
    ss.check_chain(lib, "cpu", ss.WIDTHS[0], torch.bfloat16, map_name, mode)


def test_chain_fp16(lib):
    ss.check_chain(lib, "cpu", ss.WIDTHS[0], torch.float16, "ragged", "peek")


def test_refusals_touch_nothing(lib):
    ss.check_refusals(lib, "cpu")


def test_one_call_per_hop(lib):
    ss.check_one_call(lib, "cpu")


def test_hop_cut_bitwise(lib):
    ss.check_hop_cut(lib, "cpu")


def test_stack_cache(lib):
    ss.check_stack_cache(lib, "cpu")


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the four new structs from a C program compiled against the header vs the ctypes mirrors; no version step"""
    structs = {"AumStreamInArgs": aum_hip.StreamInArgs, "AumStreamOutArgs": aum_hip.StreamOutArgs, "AumStreamLayer": aum_hip.StreamLayer,
               "AumStreamLayersArgs": aum_hip.StreamLayersArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, mirror in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in mirror._fields_]
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(mirror, f).offset, (cname, f)
    assert aum_hip.ABI_VERSION == 13
    for name in ("aum_stream_in_tm", "aum_stream_out_tm", "aum_stream_layers", "aum_stream_layers_scratch_bytes"):
        assert name in aum_hip.EXPORTS
