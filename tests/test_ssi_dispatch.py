"""The kernel and library-GEMM sequence of one Mamba block on the host build (tests/emu injected where libaum_hip.so would be), case by
case against the lists recorded before selective_scan_interface's dispatch was refactored: ssi_dispatch_checks.py."""
import os
import sys

import pytest

import aum_hip
import ssi_dispatch_checks as DC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_as_product():
    import build_emu
    old = aum_hip._product
    aum_hip._product = aum_hip.Lib(build_emu.build(), host=True)
    yield
    aum_hip._product = old


@pytest.mark.parametrize("case", DC.CPU_CASES, ids=lambda c: c[0])
def test_block_dispatch_sequence(monkeypatch, case):
    """Mamba(64), (2, 70, 64) fp32: v1 / none / v2, token-major forced and channel-major, v1 also time-reversed"""
    DC.check(monkeypatch, case, "cpu")
