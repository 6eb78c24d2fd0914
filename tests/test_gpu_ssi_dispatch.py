"""The kernel and library-GEMM sequence of one Mamba block on the device, at the smallest shapes where every kernel arm is live, against
the lists recorded before selective_scan_interface's dispatch was refactored (ssi_dispatch_checks.py): d_model 768 (d_inner 1536, dt_rank
48: the (3072, 768) / (1536, 768) aum_gemm_tn shapes, x/dt at (80, 48), the skinny weight gradients), d_model 384 (x/dt at (56, 24)), the
channel-major block, and the library arms of the projection GEMMs and of the x/dt backward."""
import pytest
import torch

import aum_hip
import ssi_dispatch_checks as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", DC.GPU_CASES, ids=lambda c: c[0])
def test_block_dispatch_sequence(monkeypatch, case):
    """one block, bf16 autocast, (2, 65, d_model)"""
    assert torch.cuda.is_available(), "these tests need a GPU"
    aum_hip.get()     # raises ImportError if the extension is missing: no fallback
    DC.check(monkeypatch, case, "cuda")
