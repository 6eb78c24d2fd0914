"""GPU: what the token-major scan / conv bindings tell the device library -- every launch's name and Args struct, field for field --
against tests/golden/binding_args.json, the record of the same cases on the lane-array build (tests/binding_pin_checks.py): nothing in it
depends on the address space.  The row families likewise against tests/golden/binding_args_rows.json, without the cases of
ROW_HOST_ONLY: calls with an operand of another type, shape or device than the kernel is told are never sent to the device."""
import pytest

import aum_hip
import binding_pin_checks as bp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return aum_hip.get()


@pytest.fixture(scope="module")
def fixture():
    return bp.load_fixture()


@pytest.mark.parametrize("group", bp.GROUPS)
def test_bindings_tell_the_library_what_the_fixture_holds(group, lib, fixture):
    bp.check_group(group, lib, "cuda", fixture)


@pytest.fixture(scope="module")
def rows_fixture():
    return bp.load_fixture(bp.ROWS_FIXTURE)


@pytest.mark.parametrize("group", bp.ROW_GROUPS)
def test_row_bindings_tell_the_library_what_the_fixture_holds(group, lib, rows_fixture):
    bp.check_group(group, lib, "cuda", rows_fixture, bp.ROW_CASES, skip=bp.ROW_HOST_ONLY)
