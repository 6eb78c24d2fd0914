"""GPU: timeline training on the device library -- k_scanp_fwd_ckpt, k_scanp_bwd and k_convp_bwd against the inference kernel (forward, bit
for bit) and the float64 twins (gradients), the leak / repeatability / isolation properties, the refusals, Mamba.forward(peek_every=) and
AudioMamba.forward_timeline with and without bf16 autocast (tests/timeline_train_checks.py).
On the commit before the feature every test here fails: the library has no aum_*_tm_peeks_* symbols, aum_hip no *_tm_peeks_* functions,
`peek_every=` is no argument of Mamba.forward and AudioMamba has no forward_timeline."""
import pytest
import torch

import aum_hip
import timeline_train_checks as tt

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


def _kind(P, dim):
    return tt.PERIODS.index(P) + tt.DIMS.index(dim)


@pytest.mark.parametrize("dim", tt.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_forward_is_the_inference_kernel_on_a_zeroed_pool(dt, dim, lib):
    for P in tt.PERIODS:
        tt.check_forward_identity(dt, dim, P, lib, DEV, kind=_kind(P, dim))


@pytest.mark.parametrize("dim", tt.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_gradients_against_float64(op, dt, dim, lib):
    for P in tt.PERIODS:
        tt.check_gradients(op, dt, dim, P, lib, DEV, kind=_kind(P, dim))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peek_rows_do_not_leak(op, dt, lib):
    for P in tt.PERIODS:
        dim = tt.DIMS[tt.PERIODS.index(P) % 2]
        tt.check_peek_rows_do_not_leak(op, dt, dim, P, lib, DEV, kind=_kind(P, dim) + 1)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_repeatable_and_independent_of_the_pack(op, dt, lib):
    for P in tt.PERIODS:
        dim = tt.DIMS[(tt.PERIODS.index(P) + 1) % 2]
        tt.check_repeatable_and_isolated(op, dt, dim, P, lib, DEV, kind=_kind(P, dim) + 2)


def test_refusals_touch_nothing(lib):
    tt.check_refusals(lib, DEV)


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
@pytest.mark.parametrize("d_model", [64, 192])
def test_module_matches_its_ref_twin(d_model, autocast):
    tt.check_module(d_model, DEV, autocast)


@pytest.mark.parametrize("autocast", [None, torch.bfloat16])
@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_forward_timeline(embed_dim, autocast):
    tt.check_model(embed_dim, DEV, autocast)


def test_model_refuses_non_streamable_configurations():
    tt.check_model_refuses_non_streamable(DEV)


def test_model_forward_timeline_from_a_waveform():
    tt.check_model_frontend(DEV)
