"""GPU: what the token-major scan / conv bindings tell the device library -- every launch's name and Args struct, field for field --
against tests/golden/binding_args.json, the record of the same cases on the lane-array build (tests/binding_pin_checks.py): nothing in it
depends on the address space."""
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
