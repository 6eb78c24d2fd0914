"""The token-major scans' activated-delta mode (AUM_SCAN_DELTA_ACTIVATED: delta already holds softplus(raw + delta_bias), as the x/dt
kernel writes it) on the host, through the lane-array build of the same kernel sources, against the fp64 oracle fed the activated delta;
the backward's ddelta / ddelta_bias against the raw-space gradients.  Plus the argument rules of the mode."""
import os
import sys

import pytest
import torch

import aum_hip
import cases
import delta_act_checks as DA

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

ACT_CASES = [c for c in cases.SCAN_TM_CASES if c[5] and c[8]]          # with z and delta_softplus: the block's scans


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
def test_scan_tm_activated(emu, case, mode):
    DA.check_scan_tm_activated(emu, "cpu", case, torch.bfloat16, reverse=(mode == "rev"), bidir=(mode == "bidir"))


@pytest.mark.parametrize("case", [c for c in ACT_CASES if c[0] in ("tm_l25", "tm_l75")], ids=lambda c: c[0])
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("segments", [2, 3])
def test_scan_tm_activated_segments(emu, case, mode, segments):
    DA.check_scan_tm_activated(emu, "cpu", case, torch.bfloat16, reverse=(mode == "rev"), bidir=(mode == "bidir"), segments=segments)


def test_scan_tm_activated_fp16(emu):
    case = [c for c in ACT_CASES if c[0] == "tm_l75"][0]
    for mode in ("fwd", "bidir"):
        DA.check_scan_tm_activated(emu, "cpu", case, torch.float16, bidir=(mode == "bidir"))


def test_activated_mode_rules(emu):
    """the mode is built for the block's scans only (16-bit activations, z present); the host build's aum_xdt_tm_fwd ignores the
    activation fields, so the wrapper refuses them there instead of handing back the raw product"""
    B, L, E, N = 1, 16, 64, 16
    A = -torch.ones(E, N)
    for dt, with_z, ok in ((torch.float32, True, False), (torch.bfloat16, False, False), (torch.bfloat16, True, True)):
        u = torch.randn(B, L, E).to(dt)
        bc = torch.randn(B, L, 2 * N).to(dt)
        z = torch.randn(B, L, E).to(dt) if with_z else None
        run = lambda: aum_hip.scan_tm_fwd(u, u.abs(), A, bc[:, :, :N], bc[:, :, N:], None, z, None, True, lib=emu, delta_activated=True)
        if ok:
            run()
        else:
            with pytest.raises(RuntimeError):
                run()
    u = torch.randn(32, 256).bfloat16()
    wx, wdt = torch.randn(80, 256).bfloat16(), torch.randn(256, 48).bfloat16()
    with pytest.raises(RuntimeError):
        aum_hip.xdt_tm_fwd(u, wx, wdt, lib=emu, delta_bias=torch.zeros(256), delta_softplus=True)
    with pytest.raises(RuntimeError):
        aum_hip.xdt_tm_fwd(u, wx, wdt, lib=emu, delta_bias=torch.zeros(256))
    x_dbl, delta = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=emu)           # the default stays available
    assert delta.shape == (32, 256)
