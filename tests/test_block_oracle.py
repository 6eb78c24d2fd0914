"""The references the wide-block GPU tests (test_gpu_block_oracle.py) stand on, checked on the host without any product kernel:
the stage-by-stage reference of block_oracle_checks.py is the fp64 oracle when nothing is rounded, and the bars derived from it
(2.2 x what the 16-bit stage boundaries cost) are far below the mistakes the GPU tests exist to catch."""
import pytest
import torch

import block_oracle_checks as BC
import cases


@pytest.mark.parametrize("activated", [True, False], ids=["delta_activated", "delta_raw"])
@pytest.mark.parametrize("case", cases.INNER_WIDE_CASES, ids=lambda c: c[0])
def test_staged_reference_is_the_oracle_without_rounding(case, activated):
    """no 16-bit tensor stored (dtype float32): every quantity and measure within 1e-12 of oracle.inner_fwd / inner_full_bwd (v1, none)
    and of the MS:214-246 composition of inner_no_out_proj_fwd / inner_bwd (v2), with delta handed over activated and raw"""
    _, q = BC.operands(case, torch.float32)
    ref = BC.oracle_reference(case, q)
    d = BC.distances(BC.staged_reference(case, q, torch.float32, activated), ref)
    assert len(d) >= 2 * (10 + 5)
    worst = max(d, key=d.get)
    assert d[worst] < 1e-12, (worst, d[worst])


_SENS = [(BC.WIDE[n], m) for n in ("v1_d384_l65", "v2_d384_l65", "none_d768_l9") for m in BC.mutants_of(BC.WIDE[n][1])]


@pytest.mark.parametrize("case,mutant", _SENS, ids=lambda v: v if isinstance(v, str) else v[0])
def test_bars_see_the_mutant(case, mutant):
    """the fp64 oracle with ONE term of the backward wrong (BC.MUTANTS) is further from the true oracle than twice the bf16 bar of at
    least one quantity and measure -- bars as the GPU test forms them (delta activated, the arm's library weight gradients rounded)"""
    lib16 = BC.arm_roundings(case, "token_major", {}, False)[1]
    q, ref, r, bar = BC.reference_and_bars(case, torch.bfloat16, True, lib16)
    d = BC.distances(BC.staged_reference(case, q, torch.float32, True, mutant=mutant), ref)
    caught = {k: d[k] / bar[k] for k in d if d[k] >= 2 * bar[k]}
    print(f"mutant ({mutant}) {BC.MUTANTS[mutant]} on {case[0]}: trips " +
          ", ".join(f"{k[0]}/{k[1]} x{v:.0f}" for k, v in sorted(caught.items(), key=lambda kv: -kv[1])[:6]))
    assert caught, (mutant, max((d[k] / bar[k], k) for k in d))
    # and only the backward is wrong: out is still the oracle's
    assert d["out", "rel"] < 1e-12


def test_bars_are_16bit_sized():
    """the measured spread is neither nothing nor everything: in bf16 out and d xz cost between one rounding (2^-9 of the largest element)
    and the project's 16-bit bar for a single kernel times the ten roundings in between; in fp16 eight times less"""
    case = BC.WIDE["v1_d384_l65"]
    rb = BC.reference_and_bars(case, torch.bfloat16, True, {"out_proj_w"})[2]
    rh = BC.reference_and_bars(case, torch.float16, True, {"out_proj_w"})[2]
    for k in (("out", "rel"), ("xz.x", "rel"), ("xz.z", "rel")):
        assert 2.0 ** -10 < rb[k] < 10 * BC.KC.TOL_BF16, (k, rb[k])
        assert rb[k] / 16 < rh[k] < rb[k] / 4, (k, rb[k], rh[k])
