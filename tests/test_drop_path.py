"""Stochastic depth in the add + RMSNorm kernels (tests/drop_path_checks.py) on the host: the lane-array build executes the kernel bodies
that hipcc compiles for gfx950, so the per-sample factor, the skipped reads of dropped samples, the row tails and the sample boundaries
inside a backward wave's rows are held to the fp64 statement here without a GPU.  The op layer and the model run on that library where
libaum_hip.so would be (as tests/test_host_package.py does); bf16 autocast needs a GPU
(tests/test_gpu_drop_path.py)."""
import os
import sys

import pytest
import torch

import aum_hip
import drop_path_checks as DC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture
def emu_as_product(emu, monkeypatch):
    monkeypatch.setattr(aum_hip, "_product", emu)


shapes = pytest.mark.parametrize("case", DC.SHAPES, ids=DC.shape_id)
dtypes = pytest.mark.parametrize("dt", DC.DTYPES, ids=DC.dtype_id)


@shapes
@dtypes
def test_vs_fp64(emu, case, dt):
    DC.check_vs_fp64(emu, "cpu", case, dt)


@shapes
@dtypes
def test_ones_scale_is_the_unscaled_kernel(emu, case, dt):
    DC.check_ones_is_unscaled(emu, "cpu", case, dt)


@shapes
@dtypes
def test_zero_scale(emu, case, dt):
    DC.check_zero_scale(emu, "cpu", case, dt)


@shapes
@dtypes
def test_samples_do_not_see_each_other(emu, case, dt):
    DC.check_samples_independent(emu, "cpu", case, dt)


@shapes
@dtypes
def test_nothing_unowned_is_written(emu, case, dt):
    DC.check_guards(emu, "cpu", case, dt)


def test_argument_rules(emu):
    DC.check_argument_rules(emu, "cpu")


@dtypes
@pytest.mark.parametrize("prenorm", [True, False], ids=["prenorm", "postnorm"])
def test_op_layer(emu_as_product, dt, prenorm, monkeypatch):
    DC.check_op_layer("cpu", dt, prenorm, monkeypatch)


def test_op_layer_grad_home(emu_as_product):
    DC.check_op_layer_grad_home("cpu")


@pytest.mark.parametrize("bidirectional", [False, True], ids=["fo-bi", "if_bidirectional"])
def test_model_vs_torch_multiply(emu_as_product, bidirectional, monkeypatch):
    DC.check_model("cpu", bidirectional, False, monkeypatch)


def test_model_eval_and_rate_zero_are_the_plain_model(emu_as_product, monkeypatch):
    DC.check_model_behaviour("cpu", monkeypatch)


def test_model_draws_once(emu_as_product, monkeypatch):
    DC.check_model_draws("cpu", monkeypatch)


def test_drop_scales(monkeypatch):
    DC.check_drop_scales("cpu", monkeypatch)


def test_launcher_scope():
    DC.check_scope()


def test_launcher_trains_with_drop_path(emu_as_product, tmp_path, monkeypatch):
    DC.check_launcher_trains(tmp_path, monkeypatch)


def test_struct_layout_matches_header(tmp_path):
    """AumNormDropArgs is AumNormArgs followed by row_scale and rows_per_scale: sizeof / offsetof from a C program against the header
    equal the ctypes mirror's"""
    import ctypes
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aum_hip.h")
    fields = ["base", "row_scale", "rows_per_scale", "reserved"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void){',
                              'printf("size %zu\\n", sizeof(AumNormDropArgs));', 'printf("norm %zu\\n", sizeof(AumNormArgs));']
                             + [f'printf("{f} %zu\\n", offsetof(AumNormDropArgs, {f}));' for f in fields] + ['return 0;}']))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(aum_hip.NormDropArgs) and int(got["norm"]) == ctypes.sizeof(aum_hip.NormArgs)
    assert int(got["base"]) == 0 and int(got["row_scale"]) == int(got["norm"])          # the fields of AumNormArgs, then the two new ones
    for f in fields:
        assert int(got[f]) == getattr(aum_hip.NormDropArgs, f).offset, f
