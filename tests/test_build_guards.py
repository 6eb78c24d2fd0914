"""csrc/build.py without a compiler: the no-scratch guard over synthetic hipcc logs (what it reports, and that it raises where it could not
have looked), and the digest's dependency set against the directory."""
import importlib.util
import os

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "audio-mamba-aum_amd", "csrc")
SCANT = "_ZN3aum11k_scant_bwdINS_6bf16_tELb1ELb1ELb1EEEv16AumScanTmBwdArgsNS_11ScanTBwdOutE"
SCANWG = "_ZN3aum12k_scanwg_fwdIfLi9ELi0ELi0EEEv14AumScanFwdArgsi"              # waits through the compiler: may spill
GEMM_TN = "_ZN4aumg12k_gemm_tn_psILb1EEEvNS_10GemmLaunchE"
GEMM_WGRAD = "_ZN4aumg12k_gemm_wgradILb1EEEv12AumGemmWArgs"


@pytest.fixture(scope="module")
def b():
    spec = importlib.util.spec_from_file_location("aum_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(name, scratch, wording="ScratchSize [bytes/lane]"):
    """one kernel's remarks as hipcc -Rpass-analysis=kernel-resource-usage prints them"""
    tail = " [-Rpass-analysis=kernel-resource-usage]\n"
    return (f"x.hip:1:1: remark: Function Name: {name}{tail}"
            f"x.hip:1:1: remark:     VGPRs: 256{tail}"
            f"x.hip:1:1: remark:     {wording}: {scratch}{tail}"
            f"x.hip:1:1: remark:     LDS Size [bytes/block]: 0{tail}")


def test_counted_kernel_with_scratch_is_reported(b):
    log = record(SCANT, 16)
    assert b.spilling_kernels(log) == [(SCANT, 16)]
    assert b.check_counted_seen("scantm_p6_d1.o", log) == [SCANT]          # seen; refusing the spill is spilling_kernels' part


def test_counted_kernel_without_scratch_is_not_reported(b):
    log = record(SCANT, 0)
    assert b.spilling_kernels(log) == []
    assert b.check_counted_seen("scantm_p6_d1.o", log) == [SCANT]


def test_uncounted_kernel_with_scratch_is_not_reported(b):
    log = record(SCANWG, 224)
    assert b.spilling_kernels(log) == []
    assert b.check_counted_seen("scan_p1_d0.o", log) == []                  # an object that is expected to hold no counted kernel


def test_gemm_object_without_its_counted_kernels_raises(b):
    with pytest.raises(RuntimeError, match="k_gemm_tn"):
        b.check_counted_seen("gemm.o", record(GEMM_WGRAD, 0) + record(SCANWG, 0))
    with pytest.raises(RuntimeError, match="k_gemm_wgrad"):
        b.check_counted_seen("gemm.o", record(GEMM_TN, 0))
    with pytest.raises(RuntimeError, match="k_gemm_tn"):
        b.check_counted_seen("gemm.o", "")
    with pytest.raises(RuntimeError, match="k_scant_"):
        b.check_counted_seen("scantm_p5_d0.o", record(GEMM_TN, 0))
    assert b.check_counted_seen("gemm.o", record(GEMM_TN, 0) + record(GEMM_WGRAD, 0)) == [GEMM_TN, GEMM_WGRAD]
    # every object of the build that holds counted kernels by its name has an expectation, the others have none
    expecting = [name for name, _ in b.parts() if any(name.startswith(p) for p in b.EXPECTED)]
    assert sorted(expecting) == ["gemm.o"] + [f"scantm_p{p}_d{d}.o" for p in (5, 6) for d in (0, 1, 2)]


def test_scratch_line_of_another_wording_raises(b):
    log = record(GEMM_TN, 0) + record(GEMM_WGRAD, 16, wording="Scratch Size [bytes/lane]")
    assert b.spilling_kernels(log) == []                                    # the old guard alone would have passed this spill
    with pytest.raises(RuntimeError, match="ScratchSize"):
        b.check_counted_seen("gemm.o", log)
    with pytest.raises(RuntimeError, match="ScratchSize"):                  # any record, in any object
        b.check_counted_seen("api.o", record(SCANWG, 16, wording="ScratchSize [bytes/wave]"))


def test_digest_covers_every_source_of_csrc(b):
    listed = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".inc", ".hip")))
    assert len(listed) > 30 and "gemm.hip" in listed and "launch.h" in listed and "xdt_fwd_body.inc" in listed
    deps = b.dep_files()
    assert deps[:-1] == listed
    assert os.path.samefile(os.path.join(CSRC, deps[-1]), os.path.join(CSRC, "..", "..", "include", "aum_hip.h"))
