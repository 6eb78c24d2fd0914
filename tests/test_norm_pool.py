"""Add + RMSNorm + mean over a sample's tokens (tests/norm_pool_checks.py) on the host: the lane-array build executes the kernel bodies that
hipcc compiles for gfx950, so the fixed summation orders, the chunk hand-over, the second launch and the backward's dy formed from
dpooled are held to their statements here without a GPU.  The operator runs on that library where libaum_hip.so would be."""
import os
import sys

import pytest

import aum_hip
import norm_pool_checks as NC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture
def emu_as_product(emu, monkeypatch):
    monkeypatch.setattr(aum_hip, "_product", emu)


shapes = pytest.mark.parametrize("case", NC.SHAPES, ids=NC.case_id)
cols = pytest.mark.parametrize("cols", NC.COLS)
dtypes = pytest.mark.parametrize("dt", NC.DTYPES, ids=NC.dtype_id)


@shapes
@cols
@dtypes
def test_forward(emu, case, cols, dt):
    NC.check_forward(emu, "cpu", case, cols, dt)


@shapes
@cols
@dtypes
def test_backward(emu, case, cols, dt):
    NC.check_backward(emu, "cpu", case, cols, dt)


@shapes
@cols
@dtypes
def test_samples_do_not_see_each_other(emu, case, cols, dt):
    NC.check_isolation(emu, "cpu", case, cols, dt)


@shapes
@cols
@dtypes
def test_nothing_unowned_is_written(emu, case, cols, dt):
    NC.check_guards(emu, "cpu", case, cols, dt)


def test_argument_rules(emu):
    NC.check_argument_rules(emu, "cpu")


@shapes
@cols
@dtypes
def test_operator(emu_as_product, case, cols, dt):
    NC.check_operator("cpu", case, cols, dt)


def test_operator_grad_home(emu_as_product):
    NC.check_operator_grad_home("cpu")


def test_cpu_tensors_without_a_library_run_the_twin(monkeypatch):
    NC.check_cpu_twin_without_library(monkeypatch)


def test_struct_layout_matches_header(tmp_path):
    """AumNormPoolArgs against the ctypes mirror: sizeof / offsetof from a C program that includes the header"""
    import ctypes
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aum_hip.h")
    fields = [f for f, _ in aum_hip.NormPoolArgs._fields_]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void){',
                              'printf("size %zu\\n", sizeof(AumNormPoolArgs));']
                             + [f'printf("{f} %zu\\n", offsetof(AumNormPoolArgs, {f}));' for f in fields] + ['return 0;}']))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(aum_hip.NormPoolArgs)
    for f in fields:
        assert int(got[f]) == getattr(aum_hip.NormPoolArgs, f).offset, f
