"""Add + RMSNorm + mean over a sample's tokens (tests/norm_pool_checks.py) of the product library on an MI355X.  Run with -m gpu."""
import pytest
import torch

import aum_hip
import norm_pool_checks as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


shapes = pytest.mark.parametrize("case", NC.SHAPES, ids=NC.case_id)
cols = pytest.mark.parametrize("cols", NC.COLS)
dtypes = pytest.mark.parametrize("dt", NC.DTYPES, ids=NC.dtype_id)


@shapes
@cols
@dtypes
def test_forward(lib, case, cols, dt):
    NC.check_forward(lib, "cuda", case, cols, dt)


@shapes
@cols
@dtypes
def test_backward(lib, case, cols, dt):
    NC.check_backward(lib, "cuda", case, cols, dt)


@shapes
@cols
@dtypes
def test_samples_do_not_see_each_other(lib, case, cols, dt):
    NC.check_isolation(lib, "cuda", case, cols, dt)


@shapes
@cols
@dtypes
def test_nothing_unowned_is_written(lib, case, cols, dt):
    NC.check_guards(lib, "cuda", case, cols, dt)


def test_argument_rules(lib):
    NC.check_argument_rules(lib, "cuda")


@shapes
@cols
@dtypes
def test_operator(lib, case, cols, dt):
    NC.check_operator("cuda", case, cols, dt)


def test_operator_grad_home(lib):
    NC.check_operator_grad_home("cuda")
