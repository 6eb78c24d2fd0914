"""Which kernels and library GEMMs one Mamba block issues, in order: the shared body of test_ssi_dispatch.py (host build) and
test_gpu_ssi_dispatch.py (device).  The sequence of one forward + backward is compared with the list recorded from the commit BEFORE the
host-side dispatch of selective_scan_interface was folded into one projection path and named block stages
(tests/golden/ssi_dispatch.json): the refactor moved code, it must not move a launch.

Recorded, in issue order:
  ["launch", name]              every aum_hip._launch (the name the binding gives the kernel)
  [op, shape, shape(, shape)]   every torch.matmul / torch.bmm / Tensor.addmm_ / F.linear whose CALLER is selective_scan_interface or
                                mamba_simple (the operands' shapes; addmm_ with the tensor it adds to in front)
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":          # run as a script (the recorder below): what conftest.py does for the tests
    sys.path[:0] = [os.path.join(os.path.dirname(_HERE), "audio-mamba-aum_amd"), os.path.join(_HERE, "emu")]

import aum_hip  # noqa: E402

GOLDEN = os.path.join(_HERE, "golden", "ssi_dispatch.json")
_CALLERS = ("mamba_ssm.ops.selective_scan_interface", "mamba_ssm.modules.mamba_simple")

# (id, d_model, bimamba_type, _TM_MIN_WAVES, time_reversed, module switches)
CPU_CASES = [(f"cpu-{b}-{'tm' if w == 0 else 'cm'}{'-rev' if r else ''}", 64, b, w, r, {})
             for b in ("v1", "none", "v2") for w in (0, 10 ** 9) for r in ((False, True) if b == "v1" else (False,))]
GPU_CASES = [("gpu-768-v1-tm", 768, "v1", 0, False, {}),
             ("gpu-768-none-tm", 768, "none", 0, False, {}),
             ("gpu-768-v2-tm", 768, "v2", 0, False, {}),
             ("gpu-384-v1-tm", 384, "v1", 0, False, {}),
             ("gpu-768-v1-cm", 768, "v1", 10 ** 9, False, {}),
             ("gpu-768-v1-tm-gemmlib", 768, "v1", 0, False, {"_GEMM_MODE": "lib", "_HIP_GEMM": False}),
             ("gpu-768-v1-tm-xdtbwdlib", 768, "v1", 0, False, {"_XDT_BWD_HIP": False})]


def _shapes(*ts):
    return [list(t.shape) for t in ts]


def record(monkeypatch, d_model, btype, min_waves, time_reversed, switches, device):
    """one Mamba(d_model) block, forward and backward, on `device` ("cpu": fp32 (2, 70, d_model) on whatever library aum_hip.get() holds;
    "cuda": (2, 65, d_model) under bf16 autocast) -> the recorded list"""
    import mamba_ssm.ops.selective_scan_interface as ssi
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(7)
    m = Mamba(d_model, bimamba_type=btype, if_devide_out=btype == "v2").to(device)
    x = (0.5 * torch.randn(2, 70 if device == "cpu" else 65, d_model, device=device)).requires_grad_(True)
    w = torch.randn_like(x) / 100
    seq = []

    def from_block():
        return sys._getframe(2).f_globals.get("__name__") in _CALLERS

    def wrap(real, name, operands):
        def f(*a, **k):
            if from_block():
                seq.append([name] + _shapes(*a[:operands]))
            return real(*a, **k)
        return f

    real_launch = aum_hip._launch

    def launch(fn, args, stream_tensor, lib, name, meta=None):
        seq.append(["launch", name])
        return real_launch(fn, args, stream_tensor, lib, name, meta)

    monkeypatch.setattr(ssi, "_TM_MIN_WAVES", min_waves)
    for k, v in switches.items():
        monkeypatch.setattr(ssi, k, v)
    with monkeypatch.context() as mp:
        mp.setattr(aum_hip, "_launch", launch)
        mp.setattr(torch, "matmul", wrap(torch.matmul, "matmul", 2))
        mp.setattr(torch, "bmm", wrap(torch.bmm, "bmm", 2))
        mp.setattr(torch.Tensor, "addmm_", wrap(torch.Tensor.addmm_, "addmm_", 3))
        mp.setattr(F, "linear", wrap(F.linear, "linear", 2))
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=device != "cpu"):
            y = m(x, time_reversed=time_reversed)
        (y.float() * w).sum().backward()
        if device != "cpu":
            torch.cuda.synchronize()
    assert x.grad is not None and all(p.grad is not None for p in m.parameters())
    return seq


def check(monkeypatch, case, device):
    cid = case[0]
    got = record(monkeypatch, *case[1:], device)
    with open(GOLDEN) as f:
        want = json.load(f)[cid]
    assert got == want, (cid, [(i, g, w_) for i, (g, w_) in enumerate(zip(got, want)) if g != w_][:4], len(got), len(want))


if __name__ == "__main__":
    # python tests/ssi_dispatch_checks.py cpu|cuda OUT.json: record every case of that device (how the golden lists were made, on the
    # commit before the refactor; merged into OUT.json if it exists)
    import pytest
    device, out = sys.argv[1], sys.argv[2]
    if device == "cpu":
        import build_emu
        aum_hip._product = aum_hip.Lib(build_emu.build(), host=True)
    lists = json.load(open(out)) if os.path.exists(out) else {}
    for case in (CPU_CASES if device == "cpu" else GPU_CASES):
        mp = pytest.MonkeyPatch()
        lists[case[0]] = record(mp, *case[1:], device)
        mp.undo()
        print(case[0], len(lists[case[0]]), "entries")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in lists.items()) + "\n}\n")
