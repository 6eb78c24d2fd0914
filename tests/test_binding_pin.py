"""CPU: what the token-major scan / conv bindings tell the library -- every launch's name and Args struct, field for field -- on the
lane-array build of the kernel sources (tests/emu) with host tensors, against tests/golden/binding_args.json
(tests/binding_pin_checks.py), and the same for the row families (channel-major scan, per-token updates, conv, add + RMSNorm,
channel-major projections) against tests/golden/binding_args_rows.json.  The device library is held to the same records in
tests/test_gpu_binding_pin.py."""
import os
import sys

import pytest

import aum_hip
import binding_pin_checks as bp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture(scope="module")
def fixture():
    return bp.load_fixture()


def test_the_fixture_holds_exactly_the_cases(fixture):
    assert sorted(fixture) == sorted(bp.CASES)


@pytest.mark.parametrize("group", bp.GROUPS)
def test_bindings_tell_the_library_what_the_fixture_holds(group, lib, fixture):
    bp.check_group(group, lib, "cpu", fixture)


@pytest.fixture(scope="module")
def rows_fixture():
    return bp.load_fixture(bp.ROWS_FIXTURE)


def test_the_rows_fixture_holds_exactly_the_cases(rows_fixture):
    assert sorted(rows_fixture) == sorted(bp.ROW_CASES)


@pytest.mark.parametrize("group", bp.ROW_GROUPS)
def test_row_bindings_tell_the_library_what_the_fixture_holds(group, lib, rows_fixture):
    bp.check_group(group, lib, "cpu", rows_fixture, bp.ROW_CASES)
