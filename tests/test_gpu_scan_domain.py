"""Value-domain checks of the scans (tests/scan_domain_checks.py) of the product library on an MI355X: every scan kernel family against the
fp64 oracle in the regimes fast_decay, threshold, long_memory, big_state and mixed_rows.  Run with -m gpu.  Measured on the MI355X: 495
cases in 12.5 s, the oracle's four runs per case (forward and backward, fp32 and fp64) included; the error / bar table is in the header of
scan_domain_checks.py."""
import pytest
import torch

import aum_hip
import scan_domain_checks as SD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return aum_hip.get()     # raises ImportError if the extension is missing: no fallback


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("shape,path,mode", SD.CM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_domain(lib, regime, shape, path, mode, dt):
    SD.check_cm(lib, "cuda", regime, shape, path, mode, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("mode", ["fwd", "rev", "bidir"])
@pytest.mark.parametrize("length,segments", SD.TM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_tm_domain(lib, regime, length, segments, mode, dt):
    SD.check_tm(lib, "cuda", regime, length, segments, mode, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_peeks_domain(lib, regime, dt):
    SD.check_peeks(lib, "cuda", regime, dt)


@pytest.mark.parametrize("dt", SD.DTYPES)
@pytest.mark.parametrize("chunk", SD.STREAM_CHUNKS + (0,), ids=lambda c: f"chunk{c}" if c else "state_update")
@pytest.mark.parametrize("regime", SD.REGIME_NAMES)
def test_scan_stream_domain(lib, regime, chunk, dt):
    SD.check_stream(lib, "cuda", regime, dt, chunk)
