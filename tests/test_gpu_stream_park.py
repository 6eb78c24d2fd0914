"""GPU: parking and resuming streaming sessions on the device library -- k_stream_park through aum_stream_park, aum_hip.stream_park and
AudioMamba.stream_park / stream_resume / stream_fork: the checks of tests/stream_park_checks.py on the MI355X (tests/test_stream_park.py
runs them on the lane-array build).  All comparisons are bitwise.  On the commit before the feature every test here fails: the entry
point and the methods do not exist."""
import pytest
import torch

import aum_hip
import stream_park_checks as pk

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


def test_kernel_raw(lib):
    pk.check_kernel_raw(lib, DEV)


def test_binding_on_strided_pools(lib):
    pk.check_binding(lib, DEV)


@pytest.mark.parametrize("to_host", [False, True], ids=["device_blob", "to_host"])
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_continuation_is_exact(lib, dtype, to_host):
    pk.check_continuation(lib, DEV, autocast_dtype=dtype, to_host=to_host)


def test_neighbours_untouched(lib):
    pk.check_neighbours(lib, DEV)


def test_fork(lib):
    pk.check_fork(lib, DEV)


def test_raw_audio_session_moves_with_its_tail(lib):
    pk.check_wave(lib, DEV)


def test_refusals_change_nothing(lib):
    pk.check_refusals(lib, DEV)


def test_one_launch_each_way(lib):
    pk.check_one_launch(lib, DEV)
