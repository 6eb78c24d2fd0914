"""GPU: streaming prefill on the MI355X -- the checks of tests/stream_prefill_checks.py on libaum_hip.so: k_scant_fwd_state /
k_scant_seg_fwd_state against scan_tm_fwd (bitwise from a zero state) and the fp64 oracle, bitwise partition invariance of the uncut
form, conv1d_tm_prefill against conv1d_stream, Mamba.prefill_chunk handing over to step_chunk (d_inner 256 with dt_rank 24 runs
aum_xdt_tm_fwd), Mamba.forward(inference_params) at offset 0 on the new path (d_model 128) and on the un-fused branch (d_model 32), AudioMamba.stream_prefill(_many)."""
import pytest

import aum_hip
import stream_prefill_checks as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.mark.parametrize("c", pc.KERNEL_CASES + pc.SEG_CASES, ids=pc.kcase_id)
def test_kernel_handoff(lib, c):
    pc.check_kernel_handoff(c, lib, DEV)


def test_refusals(lib):
    pc.check_refusals(lib, DEV)


@pytest.mark.parametrize("T,dt,kind", [(9, "f32", pc.KINDS[0]), (9, "bf16", pc.KINDS[1]), (129, "f16", pc.KINDS[5]), (129, "bf16", pc.KINDS[3])])
def test_partition_uncut_bitwise(lib, T, dt, kind):
    pc.check_partition_uncut(T, dt, kind, lib, DEV)


@pytest.mark.parametrize("cut,seg", [(512, 2), (300, 2), (1000, 2), (512, 8), (333, 8)])
def test_partition_segmented(lib, cut, seg):
    pc.check_partition_segmented(("bf16", "f32")[seg == 8], pc.KINDS[0], cut, seg, lib, DEV)


@pytest.mark.parametrize("case", pc.CONV_CASES, ids=pc.sc.case_id)
def test_conv_prefill(lib, case):
    pc.check_conv_prefill(case, lib, DEV)


@pytest.mark.parametrize("d_model,dt_rank,dt,T,batch", [(32, "auto", "f32", 1, 1), (32, "auto", "f16", 3, 3), (32, "auto", "f32", 7, 3), (128, 24, "bf16", 8, 1),
                                                        (128, 24, "bf16", 9, 1), (128, 24, "f16", 64, 3), (32, "auto", "bf16", 129, 1),
                                                        (32, "auto", "f32", 513, 1), (128, 24, "bf16", 513, 1)])
def test_mamba_prefill_then_live(lib, d_model, dt_rank, dt, T, batch):
    pc.check_mamba_handover(d_model, dt_rank, dt, T, batch, lib, DEV)


def test_model_prefill_then_push(lib):
    pc.check_model_prefill(lib, DEV)


def test_model_prefill_many(lib):
    pc.check_model_prefill_many(lib, DEV)


def test_model_refusals_touch_nothing(lib):
    pc.check_model_refusals(lib, DEV)


@pytest.mark.parametrize("d_model,new_path", [(128, True), (32, False)])
def test_forward_offset0_then_steps(lib, d_model, new_path):
    """d_model 128 (dt_rank 8): token_major_ok holds, forward at offset 0 runs prefill_chunk (asserted inside by call counts); d_model 32
    (dt_rank 2): it does not, the un-fused branch stays -- both leave caches step() continues from"""
    assert pc.check_forward_offset0(d_model, lib, DEV) is new_path
