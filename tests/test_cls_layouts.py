"""Double-cls, cls-free and randomly placed cls models (tests/cls_layout_checks.py) on the host: the model runs on the lane-array library
where libaum_hip.so would be, in fp32 (bf16 autocast, and with it the fused mean head, needs a GPU: tests/test_gpu_cls_layouts.py)."""
import os
import sys

import pytest

import aum_hip
import cls_layout_checks as LC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture
def emu_as_product(emu, monkeypatch):
    monkeypatch.setattr(aum_hip, "_product", emu)


@pytest.mark.parametrize("transpose", [False, True], ids=["freq-major", "time-major"])
@pytest.mark.parametrize("variant", list(LC.VARIANTS))
def test_model_vs_reference_tail(emu_as_product, variant, transpose):
    LC.check_model("cpu", variant, transpose)


def test_layout_rules(emu_as_product):
    LC.check_layout_rules()


def test_double_cls_checkpoint():
    LC.check_double_cls_checkpoint()


def test_launcher_scope():
    LC.check_scope()


@pytest.mark.parametrize("flags", [["--use_double_cls_token", "True", "--use_middle_cls_token", "False"],
                                   ["--if_cls_token", "False", "--final_pool_type", "mean"]], ids=["double", "cls-free-mean"])
def test_launcher_trains(emu_as_product, tmp_path, flags):
    LC.check_launcher_trains(tmp_path, flags)
