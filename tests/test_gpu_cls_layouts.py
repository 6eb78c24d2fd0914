"""Double-cls, cls-free and randomly placed cls models (tests/cls_layout_checks.py) on an MI355X under bf16 autocast: one model check per
variant, and the cls-free mean head on the fused add + norm + mean pair.  Run with -m gpu."""
import pytest
import torch

import aum_hip
import cls_layout_checks as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()


@pytest.mark.parametrize("variant", list(LC.VARIANTS))
def test_model_vs_reference_tail(lib, variant):
    LC.check_model("cuda", variant, True, autocast=True)


def test_mean_head_is_the_fused_pair(lib, monkeypatch):
    LC.check_mean_head_is_fused("cuda", monkeypatch)
