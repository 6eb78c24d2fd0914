"""CPU: the EPIC-Sounds path without a GPU -- the fp64 log-mel oracle against an independent rfft path, the HTK mel matrix, the clip and
frame-count rules, the spline solve and the draws against the reference's golden (tests/golden/epic_specaug.npz), the LR schedule, the
ctypes mirrors of the new structs, the new kernels' sources in the lane-array build, and the launcher's argument handling."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "audio-mamba-aum_amd")
sys.path[:0] = [p for p in (HERE, PKG, os.path.join(HERE, "golden")) if p not in sys.path]

import aum_hip  # noqa: E402
import epic_oracle as EO  # noqa: E402
from aum import epic as E  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "epic_specaug.npz"))


def _rfft_logmel(x, n, mel, target_length, hop=120, n_fft=2048, win=240, eps=1e-6):
    """librosa's recipe spelled out: pad n_fft // 2 zeros each side, frames of n_fft, the periodic Hann centred in the frame, rfft"""
    y = np.concatenate([np.zeros(n_fft // 2), np.asarray(x[:n], np.float64), np.zeros(n_fft // 2)])
    w = np.zeros(n_fft)
    w[(n_fft - win) // 2:(n_fft - win) // 2 + win] = EO.hann_periodic(win)
    nf = 1 + (len(y) - n_fft) // hop
    spec = np.stack([np.abs(np.fft.rfft(y[t * hop:t * hop + n_fft] * w, n=n_fft)) for t in range(nf)])
    lm = np.log(spec @ mel.astype(np.float64).T + eps)
    if nf < target_length:
        lm = np.pad(lm, ((0, target_length - nf), (0, 0)), "edge")
    return lm[:target_length]


def test_oracle_matches_rfft_frames():
    mel = E.htk_mel_matrix()
    rng = np.random.default_rng(0)
    for n in (1, 77, 1000, 5000):
        x = rng.standard_normal(n) * 0.3
        a, b = EO.logmel(x, n, mel, 64), _rfft_logmel(x, n, mel, 64)
        assert np.abs(a - b).max() < 1e-9, n


def test_htk_mel_matrix_closed_form():
    """each band is the triangle between HTK mel points i, i + 1, i + 2 evaluated at the bin frequencies k * sr / n_fft"""
    mel = E.htk_mel_matrix(24000, 2048, 128)
    assert mel.shape == (128, 1025) and mel.dtype == np.float32
    top = 2595.0 * math.log10(1.0 + 12000.0 / 700.0)
    for i in (0, 1, 63, 127):
        lo, c, hi = (700.0 * (10.0 ** (top * (i + j) / 129.0 / 2595.0) - 1.0) for j in range(3))
        f = np.arange(1025) * 24000.0 / 2048
        tri = np.clip(np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)), 0.0, None)
        np.testing.assert_allclose(mel[i], tri.astype(np.float32), rtol=1e-5, atol=1e-6)
    assert (mel.max(axis=1) > 0).all() and mel.max() <= 1.0


@pytest.mark.parametrize("n", [1, 119, 122879, 122880, 239999])
def test_frame_count_and_support(n):
    assert EO.frame_count(n) == 1 + n // 120
    # only the first 122 880 samples reach frames 0 .. 1023
    assert E.samples_needed(1024, 120, 2048, 240) == 122880
    assert EO.frame_start(1023) + 240 == 122880 and EO.frame_start(0) == -120


def test_clip_rules():
    clip = 240000
    random.seed(0)
    for n_ann in (5, 119, 122879, 122880, 239999, 240000, 240001, 500000):
        lo, hi = E.clip_bounds(1000, 1000 + n_ann, clip)
        if n_ann < clip:
            assert (lo, hi) == (1000, 1000 + n_ann)
        else:
            assert hi - lo == clip - 1 and 1000 <= lo and hi <= 1000 + n_ann
    # one uniform draw per clip either way (AL:44-49)
    random.seed(5)
    E.clip_bounds(0, 10, clip)
    a = random.random()
    random.seed(5)
    random.uniform(0, 0)
    assert random.random() == a
    assert E.timestamp_to_sec("00:01:02.345") == pytest.approx(62.345)


def test_dataset_items(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_toy_epic
    make_toy_epic.main([str(tmp_path), "--videos", "2", "--train", "12", "--val", "4"])
    ds = E.EpicSoundsDataset(str(tmp_path / "annotations" / "EPIC_Sounds_train.pkl"), str(tmp_path / "audio"), 10, 1024)
    random.seed(0)
    for i in range(len(ds)):
        w, n, y, aid = ds[i]
        r = ds.records[i]
        assert w.shape == (122880,) and y.shape == (44,) and y.sum() == 1 and y[r["label"]] == 1
        assert n == min(r["stop"] - r["start"], 239999) or (r["stop"] - r["start"] >= 240000 and n == 239999)
    np.save(tmp_path / "audio" / "int.npy", np.zeros(100, np.int16))
    with pytest.raises(ValueError):
        E.AudioSource(str(tmp_path / "audio")).read("int", 0, 10)


def _golden_cases():
    return [str(n) for n in GOLDEN["case_names"]]


@pytest.mark.parametrize("name", _golden_cases())
def test_draws_match_reference(name):
    frames, _, pseed, _, fm, tm, w, pos, dist = (int(v) for v in GOLDEN[f"{name}_meta"])
    random.seed(pseed)
    d = E.draw_specaug(frames, 128, tm, fm, w)
    assert (d["pos"], d["dist"]) == (pos, dist)
    fb, tb = GOLDEN[f"{name}_f_bands"], GOLDEN[f"{name}_t_bands"]
    assert [tuple(b) for b in fb if b[0] >= 0] == d["f"] and [tuple(b) for b in tb if b[0] >= 0] == d["t"]


def _flow(table, F, T):
    """the time flow of a table row, float32 numpy (the kernel's formula)"""
    cy, cx, w, v0, v1, v2, xn, yn = (np.float32(v) for v in table)
    y, x = np.meshgrid(np.arange(F, dtype=np.float32), np.arange(T, dtype=np.float32), indexing="ij")
    r = (xn - (y * cy + x * cx) * np.float32(2)) + yn
    phi = (r * np.float32(0.5)) * np.log(np.maximum(r, np.float32(1e-10)))
    return phi * w + ((y * v0 + x * v1) + v2)


@pytest.mark.parametrize("name", _golden_cases())
def test_spline_solve_and_flow_match_reference(name):
    frames, dist = int(GOLDEN[f"{name}_meta"][0]), int(GOLDEN[f"{name}_meta"][8])
    cy, cx, w, v0, v1, v2, yn = E.solve_warp(torch.tensor(GOLDEN[f"{name}_point"]), dist, torch.tensor(GOLDEN[f"{name}_eps"]))
    gw, gv = GOLDEN[f"{name}_w"], GOLDEN[f"{name}_v"]
    assert gw[0, 0, 0] == 0 and (gv[0, :, 0] == 0).all()           # the frequency component is exactly 0
    np.testing.assert_allclose([w, v0, v1, v2], [gw[0, 0, 1], *gv[0, :, 1]], rtol=1e-6)
    table = E.warp_table([torch.tensor(GOLDEN[f"{name}_point"])], [dist], [torch.tensor(GOLDEN[f"{name}_eps"])], 128, frames)[0].numpy()
    ref = GOLDEN[f"{name}_flow"]
    scale = float(np.abs(ref).max()) + 1.0
    assert np.abs(_flow(table, 128, frames) - ref).max() <= 1e-5 * scale * 100


def test_lr_schedule():
    lr, ws = 1e-3, 200
    assert E.epic_warm_lr(0, lr, ws) == pytest.approx(lr * 0.01)
    assert E.epic_warm_lr(ws - 1, lr, ws) == pytest.approx(lr * 0.01 + (ws - 1) * (lr - lr * 0.01) / ws)
    assert E.epic_warm_lr(ws, lr, ws) == lr and E.epic_warm_lr(10 * ws, lr, ws) == lr
    assert [E.epic_lr_factor(e) for e in (0, 9, 10, 19, 20, 50)] == [1.0, 1.0, 0.05, 0.05, 0.01, 0.01]
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=E.epic_lr_factor)
    seen = []
    for _ in range(22):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert seen[9] == pytest.approx(lr) and seen[10] == pytest.approx(0.05 * lr) and seen[20] == pytest.approx(0.01 * lr)


def test_struct_layouts(tmp_path):
    hdr = os.path.join(ROOT, "include", "aum_hip.h")
    probes = {"AumStftArgs": (aum_hip.StftArgs, ["wave", "n_valid", "out", "wave_bs", "out_bs", "batch", "n_fft", "target_length", "eps", "reserved"]),
              "AumTimeWarpArgs": (aum_hip.TimeWarpArgs, ["in", "table", "out", "in_bs", "out_bs", "batch", "frames", "num_mel", "reserved"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void){"]
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    (tmp_path / "p.c").write_text("\n".join(lines))
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang", str(tmp_path / "p.c"), "-o", str(tmp_path / "p")])
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([str(tmp_path / "p")], text=True).splitlines())
    for cname, (cls, fields) in probes.items():
        assert int(got[cname]) == __import__("ctypes").sizeof(cls), cname
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, "in_" if f == "in" else f).offset, (cname, f)
    assert "aum_stft_logmel_fwd" in aum_hip.EXPORTS and "aum_spec_time_warp" in aum_hip.EXPORTS


@pytest.fixture(scope="module")
def emu():
    from tests.emu import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


def test_emu_logmel_vs_oracle(emu):
    tab = E.StftTables("cpu")
    rng = np.random.default_rng(7)
    T = 40
    ns = [1, 119, 2000, 4799, 4800, 6000]
    x = np.zeros((len(ns), 4800), np.float32)
    for i, n in enumerate(ns[1:], 1):
        m = min(n, 4800)
        x[i, :m] = np.sin(2 * np.pi * 440.0 / 24000 * np.arange(m)) if i == 2 else rng.standard_normal(m) * 0.3
    out = aum_hip.stft_logmel_fwd(torch.tensor(x), torch.tensor(ns, dtype=torch.int32), tab.tables, T, 1e-6, lib=emu).numpy()
    for i, n in enumerate(ns):
        EO.check_logmel(out[i], x[i], min(n, 4800), tab.mel, T)


@pytest.mark.parametrize("name", _golden_cases())
def test_emu_time_warp_and_masks_vs_golden(emu, name):
    from make_golden_epic import spectrogram
    frames, nseed = int(GOLDEN[f"{name}_meta"][0]), int(GOLDEN[f"{name}_meta"][1])
    dist = int(GOLDEN[f"{name}_meta"][8])
    spec = spectrogram(nseed, frames)
    table = E.warp_table([torch.tensor(GOLDEN[f"{name}_point"])], [dist], [torch.tensor(GOLDEN[f"{name}_eps"])], 128, frames)
    # two clips in one launch (the second a copy), so that waves cross a clip boundary
    x = torch.tensor(np.stack([spec.T, spec.T]).copy())
    warped = aum_hip.spec_time_warp(x, torch.cat([table, table]).contiguous(), lib=emu)
    slope = float(np.abs(np.diff(spec, axis=1)).max())
    for b in range(2):
        assert np.abs(warped[b].numpy() - GOLDEN[f"{name}_warped"].T).max() <= 1e-5 + 1e-4 * slope
    fb = torch.tensor(np.maximum(GOLDEN[f"{name}_f_bands"], 0))[None]
    tb = torch.tensor(np.maximum(GOLDEN[f"{name}_t_bands"], 0))[None]
    out = E.apply_masks(warped[:1], fb, tb)
    assert np.abs(out[0].numpy() - GOLDEN[f"{name}_out"].T).max() <= 1e-4 + 1e-4 * slope


def test_launcher_accepts_epic_sounds(tmp_path):
    from aum.train import build_parser, check_scope, epic_config
    args = build_parser().parse_args(["--dataset", "epic_sounds", "--n_class", "44", "--loss", "CE", "--metrics", "acc",
                                      "--epic_annotations_dir", str(tmp_path), "--epic_audio", str(tmp_path), "--timem", "192",
                                      "--freqm", "48", "--audio_length", "1024"])
    check_scope(args)
    cfg = epic_config(args)
    assert (cfg["T_MASK"], cfg["F_MASK"], cfg["CLIP_SECS"], cfg["NUM_FRAMES"], cfg["T_WARP"]) == (192, 48, 10, 1024, 5)
    (tmp_path / "c.yaml").write_text("AUDIO_DATA:\n  SAMPLING_RATE: 24000\nEPICSOUNDS:\n  ANNOTATIONS_DIR: /a\n  AUDIO_DATA_FILE: /b.hdf5\n"
                                     "  TRAIN_LIST: tr.pkl\n  VAL_LIST: va.pkl\n")
    args = build_parser().parse_args(["--dataset", "epic_sounds", "--epic_config", str(tmp_path / "c.yaml"), "--timem", "96",
                                      "--audio_length", "512"])
    cfg = epic_config(args)
    assert (cfg["ANNOTATIONS_DIR"], cfg["AUDIO_DATA_FILE"], cfg["VAL_LIST"], cfg["T_MASK"], cfg["CLIP_SECS"]) == ("/a", "/b.hdf5", "va.pkl", 48, 5)
    r = subprocess.run([sys.executable, "-m", "aum.train", "--dataset", "epic_sounds", "--help"], cwd=PKG, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT])))
    assert r.returncode == 0 and "--epic_audio" in r.stdout


def test_launcher_epic_scope():
    """--dataset epic_sounds passes the scope check once its data source is named; without one (the reference's built-in default
    config) it stays refused"""
    from aum import train as T
    parse = T.build_parser().parse_args
    with pytest.raises(NotImplementedError):
        T.check_scope(parse(["--dataset", "epic_sounds"]))
    with pytest.raises(NotImplementedError):
        T.check_scope(parse(["--dataset", "epic_sounds", "--epic_audio", "/a"]))
    T.check_scope(parse(["--dataset", "epic_sounds", "--epic_annotations_dir", "/a", "--epic_audio", "/b"]))
    T.check_scope(parse(["--dataset", "epic_sounds", "--epic_config", "/c.yaml"]))
    for extra in (["--model", "ast"], ["--flexible_training", "True"], ["--aum_drop_path", "0.1"]):
        with pytest.raises(NotImplementedError):
            T.check_scope(parse(extra + ["--dataset", "epic_sounds", "--epic_config", "/c.yaml"]))
