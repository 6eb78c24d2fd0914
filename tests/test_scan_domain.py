"""Value-domain checks of the scans (tests/scan_domain_checks.py) on the host.  First the conditions on the regimes' inputs, on the fp64 oracle
alone, before any kernel runs; then the lane-array build, which executes the scan kernel bodies that hipcc compiles for gfx950: their softplus
and its derivative, carries, checkpoints and lane products are held to the regimes here without a GPU.  aum_selective_state_update is a plain
loop in that build (tests/emu/aum_emu.cpp): its run here checks the wrapper; the device kernel is held by tests/test_gpu_scan_domain.py, as
are the hardware's own exp2 / log2 / rcp."""
import os
import sys

import pytest

import aum_hip
import scan_domain_checks as SD
import timeline_train_checks as TT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_input_conditions(regime, dt):
    """every reference finite, no all-zero row of out / du / ddelta, big_state inside fp16's range, long_memory's out all state path"""
    for tag, (batch, dim, length) in SD.CM_SHAPES.items():
        SD.check_conditions(regime, tag, batch, dim, length, dt, bidir=length < 1024)
    for length in sorted({c[0] for c in SD.TM_CASES}):
        SD.check_conditions(regime, f"tm{length}", 1, 64, length, dt, bidir=True)
    SD.check_conditions(regime, "peeks", 1, 64, sum(TT.layout(SD.PEEK_P)), dt)
    SD.check_conditions(regime, "stream", 1, 64, SD.STREAM_LEN, dt)
    SD.check_conditions(regime, "state_update", 1, SD.STEP_DIM, SD.STEP_LEN, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("shape,path,mode", SD.CM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_domain(emu, regime, shape, path, mode, dt):
    SD.check_cm(emu, "cpu", regime, shape, path, mode, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("length,segments", SD.TM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_tm_domain(emu, regime, length, segments, mode, dt):
    SD.check_tm(emu, "cpu", regime, length, segments, mode, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_peeks_domain(emu, regime, dt):
    SD.check_peeks(emu, "cpu", regime, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("chunk", SD.STREAM_CHUNKS + (0,), ids=lambda c: f"chunk{c}" if c else "state_update")
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_stream_domain(emu, regime, chunk, dt):
    SD.check_stream(emu, "cpu", regime, dt, chunk)
