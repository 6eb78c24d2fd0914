"""GPU: the EPIC-Sounds frontend kernels (aum_stft_logmel_fwd, aum_spec_time_warp) against the fp64 oracle (tests/epic_oracle.py) and
the reference's SpecAugment golden (tests/golden/epic_specaug.npz), and `python -m aum.train --dataset epic_sounds` end to end on a toy set."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "audio-mamba-aum_amd")
sys.path[:0] = [p for p in (HERE, PKG) if p not in sys.path]

import epic_oracle as EO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, TL = 12, 1024
SHIP = 122880          # samples the 1024 kept frames read


def _tables():
    from aum.epic import StftTables
    return StftTables(DEV)


def _run(x, n):
    import aum_hip
    tab = _tables()
    out = aum_hip.stft_logmel_fwd(torch.tensor(x, device=DEV), torch.tensor(n, dtype=torch.int32, device=DEV), tab.tables, TL, 1e-6)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tab.mel


def _check_all(x, n):
    got, mel = _run(x, n)
    for b in range(x.shape[0]):
        EO.check_logmel(got[b], x[b], min(int(n[b]), x.shape[1]), mel, TL)


def test_logmel_white_noise_gpu():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((B, SHIP)) * rng.uniform(0.01, 1.0, (B, 1))).astype(np.float32)
    _check_all(x, [239999] * B)


def test_logmel_sines_gpu():
    """pure tones: the window's deep sidelobes put most bands many decades below the peak (the absolute half of the bar)"""
    t = np.arange(SHIP) / 24000.0
    f = np.linspace(50.0, 11500.0, B)
    x = (0.5 * np.sin(2 * np.pi * f[:, None] * t[None, :] + np.arange(B)[:, None])).astype(np.float32)
    _check_all(x, [SHIP] * B)


def test_logmel_silence_and_short_clips_gpu():
    rng = np.random.default_rng(2)
    x = np.zeros((B, SHIP), np.float32)
    n = [0, 1, 50, 119, 120, 121, 4000, 24000, 122879, 122880, 200000, 239999]
    n[0] = 1                         # a silent clip of one sample
    for b in range(2, B):
        m = min(n[b], SHIP)
        x[b, :m] = rng.standard_normal(m) * 0.1
    _check_all(x, n)


def test_logmel_mixed_lengths_gpu():
    rng = np.random.default_rng(3)
    n = rng.integers(1, 240000, B)
    x = np.zeros((B, SHIP), np.float32)
    for b in range(B):
        m = min(int(n[b]), SHIP)
        x[b, :m] = rng.standard_normal(m) * rng.uniform(0.001, 1.0)
    _check_all(x, n)


def test_time_warp_and_masks_vs_reference_golden_gpu():
    import aum_hip
    from aum.epic import warp_table, apply_masks
    g = np.load(os.path.join(HERE, "golden", "epic_specaug.npz"))
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_golden_epic import spectrogram
    for name in g["case_names"]:
        frames, nseed, *_ = g[f"{name}_meta"]
        dist = int(g[f"{name}_meta"][8])
        spec = spectrogram(int(nseed), int(frames))                       # (128, T), the reference's (F, T) image
        x = torch.tensor(spec.T.copy(), device=DEV).unsqueeze(0)         # (1, T, F): the kernel's layout
        table = warp_table([torch.tensor(g[f"{name}_point"])], [dist], [torch.tensor(g[f"{name}_eps"])], 128, int(frames)).to(DEV)
        warped = aum_hip.spec_time_warp(x, table)
        ref = g[f"{name}_warped"].T
        slope = float(np.abs(np.diff(spec, axis=1)).max())
        err = float(np.abs(warped[0].cpu().numpy() - ref).max())
        # the flow is a float32 spline whose terms reach |phi w| ~ 1e2: a few ulp of it, times the largest step between frames
        assert err <= 1e-5 + 1e-4 * slope, (name, err, slope)
        fb = torch.tensor(np.maximum(g[f"{name}_f_bands"], 0))[None]
        tb = torch.tensor(np.maximum(g[f"{name}_t_bands"], 0))[None]
        out = apply_masks(warped, fb.to(DEV), tb.to(DEV))
        err = float(np.abs(out[0].cpu().numpy() - g[f"{name}_out"].T).max())
        assert err <= 1e-4 + 1e-4 * slope, (name, err)


def _toy(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_toy_epic
    make_toy_epic.main([str(tmp_path / "toy"), "--videos", "2", "--train", "24", "--val", "12"])
    return tmp_path / "toy"


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_train_epic_end_to_end_gpu(tmp_path, precision):
    toy = _toy(tmp_path)
    exp = tmp_path / "exp"
    common = ["--dataset", "epic_sounds", "--n_class", "44", "--loss", "CE", "--metrics", "acc", "--model_type", "tiny", "--depth", "2",
              "--epic_annotations_dir", str(toy / "annotations"), "--epic_audio", str(toy / "audio"), "-b", "4", "-w", "0",
              "--freqm", "48", "--timem", "192", "--mixed_precision", precision, "--exp-dir", str(exp), "--lr", "1e-4"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "aum.train"] + common
                       + ["--n-epochs", "2", "--max-steps", "3", "--warmup", "True"], cwd=PKG, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = np.loadtxt(exp / "result.csv", delimiter=",")
    assert res.shape == (2, 8) and np.isfinite(res[:, [0, 5, 6, 7]]).all(), res        # acc, train / valid loss, lr (AUC: toy classes)
    from aum.epic import epic_warm_lr
    # acc; the LR of the last step: step 5 of a 2 x 6-step warm-up (24 clips / -b 4, drop_last), TT:99-112
    assert 0.0 <= res[0, 0] <= 1.0 and res[1, 7] == pytest.approx(epic_warm_lr(5, 1e-4, 12))
    ck = exp / "models" / "best_audio_model.pth"
    assert ck.exists()
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "aum.train"] + common
                       + ["--run_type", "eval", "--aum_pretrain", "True", "--aum_pretrain_path", str(ck)], cwd=PKG, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ev = np.loadtxt(exp / "result_eval.csv", delimiter=",")
    assert np.isfinite(ev[[0, 5]]).all() and 0.0 <= ev[0] <= 1.0
