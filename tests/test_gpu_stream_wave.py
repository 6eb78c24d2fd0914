"""GPU: streaming from raw audio on the device library -- the bodies of tests/stream_wave_checks.py that tests/test_stream_wave.py
runs on the lane-array build."""
import pytest

import stream_wave_checks as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    import aum_hip
    return aum_hip.get()


def test_any_cut_gives_the_same_bits(lib):
    wc.check_any_cut(DEV, lib)


def test_sessions_are_independent_and_other_rows_untouched(lib):
    wc.check_independence(DEV, lib)


def test_end_of_clip(lib):
    wc.check_end(DEV, lib)


def test_read_with_the_push(lib):
    wc.check_read(DEV, lib)


def test_refusals_leave_no_trace(lib):
    wc.check_refusals(DEV, lib)
