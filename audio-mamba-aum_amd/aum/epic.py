"""EPIC-Sounds: annotations, audio, clip selection and the GPU frontend of the reference's EPIC recipe
(/root/reference/src/epic_sounds/epic_data: epicsounds.py, epicsounds_record.py, audio_loader_epicsounds.py = "AL",
spec_augment.py = "SA"; the overrides of run.py:139-158).

The reference computes a librosa log-mel per clip on CPU DataLoader workers and SpecAugments it there.  Here the workers only read
and cut waveforms; the log-mel (aum_stft_logmel_fwd) and the time warp (aum_spec_time_warp) are HIP kernels, the four mean-filled
masks are one reduction and one select per mask on the device.  The random draws stay on the host, with Python `random`, in the
reference's call order per clip (time warp, two frequency masks, two time masks); the time warp's spline coefficients are solved on
the host in float32 with the reference's own sequence of torch operations.
"""
import math
import os
import random
import time
from datetime import timedelta

import numpy as np
import torch
from torch.utils.data import Dataset

import aum_hip

EPIC_CLASSES = 44
SAMPLE_RATE = 24000


# ---------------------------------------------------------------------------------------------------------------------------------------
# annotations and audio
# ---------------------------------------------------------------------------------------------------------------------------------------
def timestamp_to_sec(ts):
    """'HH:MM:SS.fff' -> seconds (epicsounds_record.py:4-11)"""
    x = time.strptime(ts, "%H:%M:%S.%f")
    return float(timedelta(hours=x.tm_hour, minutes=x.tm_min, seconds=x.tm_sec).total_seconds()) + float(ts.split(".")[-1]) / 1000


def read_annotations(path, sample_rate=SAMPLE_RATE):
    """one record per row of the pandas pickle: dict(video_id, annotation_id, start, stop (samples), label)"""
    import pandas as pd
    out = []
    for _, row in pd.read_pickle(path).iterrows():
        out.append(dict(video_id=row["video_id"], annotation_id=row["annotation_id"],
                        start=int(timestamp_to_sec(row["start_timestamp"]) * sample_rate),
                        stop=int(timestamp_to_sec(row["stop_timestamp"]) * sample_rate),
                        label=int(row["class_id"]) if "class_id" in row else 0))
    if not out:
        raise ValueError(f"{path}: no annotations")
    return out


class AudioSource:
    """Audio of whole videos by video id: an HDF5 file (the reference's AUDIO_DATA_FILE, read with h5py when it imports; only the slice a
    clip needs is read) or a directory of <video_id>.npy float arrays (memory-mapped).  Integer audio is refused, as librosa refuses it."""

    def __init__(self, path):
        self.path = path
        self.h5 = None
        if os.path.isdir(path):
            self.kind = "npy"
        else:
            try:
                import h5py  # noqa: F401
            except ImportError as e:
                raise ImportError(f"{path}: reading an HDF5 audio file needs h5py; a directory of <video_id>.npy arrays works without") from e
            self.kind = "h5"

    def _video(self, video_id):
        if self.kind == "npy":
            return np.load(os.path.join(self.path, f"{video_id}.npy"), mmap_mode="r")
        if self.h5 is None:                 # opened lazily: one handle per loader worker
            import h5py
            self.h5 = h5py.File(self.path, "r")
        return self.h5[video_id]

    def read(self, video_id, lo, hi):
        v = self._video(video_id)
        if not np.issubdtype(v.dtype, np.floating):
            raise ValueError(f"{video_id}: audio must be floating-point (got {v.dtype}), as librosa requires")
        lo = max(lo, 0)
        return np.asarray(v[lo:max(hi, lo)], dtype=np.float32).reshape(-1)


def clip_bounds(start, stop, clip):
    """[lo, hi) samples of one clip (AL:24-67): a uniformly placed window of clip - 1 samples inside the annotation, or the whole annotation
    when it is shorter than `clip`.  One random.uniform draw either way, as the reference."""
    n_ann = stop - start
    delta = max(n_ann - clip, 0)
    u = random.uniform(0, delta)
    if n_ann < clip:
        return start, stop
    return int(start + u), int(start + u + clip - 1)


def samples_needed(target_length, hop, n_fft, win):
    """samples from the clip start that frames 0 .. target_length - 1 read"""
    return (target_length - 1) * hop - n_fft // 2 + (n_fft - win) // 2 + win


class EpicSoundsDataset(Dataset):
    """item -> (waveform (ship,) fp32 zero-padded, n valid samples of the clip, one-hot label (44,), annotation_id).  `ship` = the samples the
    kept frames read; n can exceed it (the frame count 1 + n // hop is what decides the edge padding)."""

    def __init__(self, annotations, audio, clip_secs, target_length, sample_rate=SAMPLE_RATE, hop=120, n_fft=2048, win=240):
        self.records = read_annotations(annotations, sample_rate) if isinstance(annotations, str) else list(annotations)
        self.audio = audio if isinstance(audio, AudioSource) else AudioSource(audio)
        self.clip = int(round(sample_rate * clip_secs))
        self.ship = samples_needed(target_length, hop, n_fft, win)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, index):
        r = self.records[index]
        lo, hi = clip_bounds(r["start"], r["stop"], self.clip)
        n = hi - lo
        x = self.audio.read(r["video_id"], lo, min(hi, lo + self.ship))
        n = min(n, len(x)) if len(x) < min(n, self.ship) else n        # a video shorter than its annotation: what is there
        buf = np.zeros(self.ship, np.float32)
        buf[:len(x)] = x
        label = np.zeros(EPIC_CLASSES, np.float32)
        label[r["label"]] = 1.0
        return torch.from_numpy(buf), n, torch.from_numpy(label), str(r["annotation_id"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# log-mel tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def htk_mel_matrix(sample_rate=SAMPLE_RATE, n_fft=2048, n_mels=128, fmin=0.0, fmax=None):
    """(n_mels, 1 + n_fft // 2) float32 triangles on the HTK mel scale, no area normalisation (librosa.filters.mel(htk=True, norm=None))"""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    fft_f = np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz_htk(np.linspace(hz_to_mel_htk(fmin), hz_to_mel_htk(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2), np.float32)
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w


class StftTables:
    """window, twiddles and the sparse mel filterbank of aum_stft_logmel_fwd, built once per configuration (AL:94-129: n_fft 2048, periodic
    Hann of round(10 ms * sr) samples, hop round(5 ms * sr), 128 HTK bands from 0 to sr / 2)"""

    def __init__(self, device, sample_rate=SAMPLE_RATE, n_fft=2048, window_ms=10, hop_ms=5, n_mels=128):
        win = int(round(window_ms * sample_rate / 1e3))
        hop = int(round(hop_ms * sample_rate / 1e3))
        j = np.arange(win, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * math.pi * j / win)                # periodic Hann (scipy get_window, fftbins=True)
        k = np.arange(n_fft // 2, dtype=np.float64)
        tw = np.stack([np.cos(2.0 * math.pi * k / n_fft), -np.sin(2.0 * math.pi * k / n_fft)], axis=1)
        mel = htk_mel_matrix(sample_rate, n_fft, n_mels)
        start = np.zeros(n_mels, np.float32)
        count = np.zeros(n_mels, np.float32)
        rows = []
        for i in range(n_mels):
            nz = np.nonzero(mel[i])[0]
            if len(nz):
                start[i], count[i] = nz[0], nz[-1] - nz[0] + 1
                rows.append(mel[i, nz[0]:nz[-1] + 1])
            else:
                rows.append(np.zeros(0, np.float32))
        stride = max(1, int(count.max()))
        mel_w = np.zeros((n_mels, stride), np.float32)
        for i, r in enumerate(rows):
            mel_w[i, :len(r)] = r
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
        self.mel = mel
        self.tables = dict(window=t(window), twiddle=t(tw), mel_start_f=t(start), mel_count_f=t(count), mel_w=t(mel_w),
                           win=win, hop=hop, n_fft=n_fft)


def logmel(wave, n_valid, tables, target_length, eps=1e-6):
    """(batch, n) fp32 waveforms + (batch,) valid counts -> (batch, target_length, n_mels) log-mel (AL:94-156)"""
    n_valid = torch.as_tensor(n_valid).to(device=wave.device, dtype=torch.int32).contiguous()
    return aum_hip.stft_logmel_fwd(wave.contiguous(), n_valid, tables.tables, target_length, eps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# SpecAugment (SA:346-413)
# ---------------------------------------------------------------------------------------------------------------------------------------
def epic_lr_factor(epoch):
    """the LambdaLR factor of the EPIC recipe (traintest.py:63-72)"""
    return 1.0 if epoch < 10 else (0.05 if epoch < 20 else 0.01)


def epic_warm_lr(step, lr, warm_steps):
    """the LR of step `step` under --warmup (traintest.py:99-112): linear from lr / 100 over warm_steps steps, then lr on every step"""
    if step < warm_steps:
        return lr * 0.01 + step * (lr - lr * 0.01) / warm_steps
    return lr


def draw_specaug(n_frames, n_mels, t_mask, f_mask, warp, rng=random):
    """one clip's draws, in the reference's call order: time_warp (frame of the control value, shift), freq_mask x 2, time_mask x 2.
    -> dict(pos, dist, f=[(lo, hi)...], t=[(lo, hi)...]); a width draw of 0 ends that kind of mask (SA:371-373, 390-392)."""
    pos = rng.randrange(warp, n_frames - warp)
    dist = rng.randrange(-warp, warp)
    bands = {}
    for kind, width, size in (("f", f_mask, n_mels), ("t", t_mask, n_frames)):
        bands[kind] = []
        if width <= 0:
            continue
        for _ in range(2):
            w = rng.randrange(0, width)
            zero = rng.randrange(0, size - w)
            if w == 0:
                break
            bands[kind].append((zero, rng.randrange(zero, zero + w)))
    return dict(pos=pos, dist=dist, f=bands["f"], t=bands["t"])


_GRID_SQ = {}


def grid_square_sum(n_mels, n_frames):
    """the reference's x_norm_squared: ONE float32 torch.sum over the squares of every (mel, frame) grid point (SA:52-56, 140-141), summed the
    way a single-threaded loader worker sums it"""
    key = (n_mels, n_frames)
    if key not in _GRID_SQ:
        y = torch.linspace(0, n_mels - 1, n_mels)
        x = torch.linspace(0, n_frames - 1, n_frames)
        gy, gx = torch.meshgrid(y, x, indexing="ij")
        q = torch.stack((gy, gx), -1).reshape([n_mels * n_frames, 2]).unsqueeze(0).float()
        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            _GRID_SQ[key] = float(torch.sum(torch.mul(q, q)))
        finally:
            torch.set_num_threads(nt)
    return _GRID_SQ[key]


def _phi2(r):
    return 0.5 * r * torch.log(torch.max(r, torch.tensor(1e-10)))


def solve_warp(point, dist, eps_block, y=64):
    """the one-centre polyharmonic spline of time_warp (SA:62-117, 346-360), float32 on the host with the reference's operations:
    control point (y, point + dist) with flow (0, (point + dist) - point); eps_block = the (1, 3, 3) randn * 1e-7 block of its solve.
    -> (cy, cx, w, v0, v1, v2, yn) of the time component (the frequency component is exactly 0)"""
    point = torch.as_tensor(point, dtype=torch.float32)
    src = torch.stack([torch.tensor(float(y)), point]).reshape(1, 1, 2)
    dst = torch.stack([torch.tensor(float(y)), point + dist]).reshape(1, 1, 2)
    c, f = dst, (dst - src).float()
    n = 1
    sq = torch.sum(torch.mul(c, c)) - 2 * torch.matmul(c.squeeze(0), c.squeeze(0).transpose(0, 1)) + torch.sum(torch.mul(c, c))
    matrix_a = _phi2(sq.float()).unsqueeze(0)
    matrix_b = torch.cat((c, torch.ones(n, dtype=c.dtype).view([-1, n, 1])), 2).float()
    left = torch.cat((matrix_a, torch.transpose(matrix_b, 2, 1)), 1)
    right = torch.cat((matrix_b, eps_block), 1)
    lhs = torch.cat((left, right), 2)
    rhs = torch.cat((f, torch.zeros((1, 3, 2), dtype=c.dtype).float()), 1)
    try:
        X = torch.linalg.solve(lhs, rhs)
    except Exception:              # the reference's fallback (SA:111-114)
        X = torch.matmul(torch.linalg.pinv(lhs), rhs)
    w, v = X[0, :n, 1], X[0, n:, 1]
    yn = torch.sum(torch.mul(c, c))
    return (float(c[0, 0, 0]), float(c[0, 0, 1]), float(w[0]), float(v[0]), float(v[1]), float(v[2]), float(yn))


def warp_table(points, dists, eps_blocks, n_mels, n_frames, y=64):
    """(batch, 8) fp32 host table of aum_spec_time_warp"""
    xn = grid_square_sum(n_mels, n_frames)
    rows = []
    for p, d, e in zip(points, dists, eps_blocks):
        cy, cx, w, v0, v1, v2, yn = solve_warp(p, d, e, y)
        rows.append([cy, cx, w, v0, v1, v2, xn, yn])
    return torch.tensor(rows, dtype=torch.float32)


def apply_masks(spec, f_bands, t_bands):
    """the four mean-filled masks (SA:363-409) on (batch, frames, n_mels): f_bands / t_bands (batch, 2, 2) int64 [lo, hi) per mask (empty when
    lo >= hi), applied in order f0, f1, t0, t1; each mask fills with the mean of the whole (already masked) spectrogram of its clip"""
    B, T, F = spec.shape
    fi = torch.arange(F, device=spec.device).view(1, 1, F)
    ti = torch.arange(T, device=spec.device).view(1, T, 1)
    for bands, idx in ((f_bands, fi), (t_bands, ti)):
        for k in range(2):
            lo, hi = bands[:, k, 0].view(B, 1, 1), bands[:, k, 1].view(B, 1, 1)
            mean = spec.mean(dim=(1, 2)).view(B, 1, 1)
            spec = torch.where((idx >= lo) & (idx < hi), mean, spec)
    return spec


class EpicFrontend:
    """waveform batch on the device -> (log-mel (batch, target_length, n_mels), None): the shape of Frontend's unfused output in aum.train.
    train=True adds the recipe's SpecAugment (time warp W, two frequency masks of width < f_mask, two time masks of width < t_mask)."""

    def __init__(self, device, target_length, train, t_mask=0, f_mask=0, warp=5, seed=0, sample_rate=SAMPLE_RATE):
        self.tables = StftTables(device, sample_rate)
        self.target_length, self.train = target_length, train
        self.t_mask, self.f_mask, self.warp = t_mask, f_mask, warp
        self.gen = torch.Generator().manual_seed(seed)          # the eps blocks of the spline solve (the reference: torch's global generator)
        self.last_draws = None

    def spectrogram(self, wave, n_valid):
        return logmel(wave, n_valid, self.tables, self.target_length)

    def augment(self, spec, draws=None, eps_blocks=None):
        B, T, F = spec.shape
        if draws is None:
            draws = [draw_specaug(T, F, self.t_mask, self.f_mask, self.warp) for _ in range(B)]
        if eps_blocks is None:
            eps_blocks = [torch.randn((1, 3, 3), generator=self.gen) * 1e-7 for _ in range(B)]
        y = F // 2
        pos = torch.tensor([d["pos"] for d in draws], device=spec.device)
        points = spec[torch.arange(B, device=spec.device), pos, y].cpu()            # the control point's time value: one small copy per batch
        table = warp_table(points, [d["dist"] for d in draws], eps_blocks, F, T, y).to(spec.device)
        spec = aum_hip.spec_time_warp(spec, table)
        fb = torch.zeros((B, 2, 2), dtype=torch.int64)
        tb = torch.zeros((B, 2, 2), dtype=torch.int64)
        for i, d in enumerate(draws):
            for k, band in enumerate(d["f"]):
                fb[i, k] = torch.tensor(band)
            for k, band in enumerate(d["t"]):
                tb[i, k] = torch.tensor(band)
        self.last_draws = (draws, eps_blocks, table)
        return apply_masks(spec, fb.to(spec.device), tb.to(spec.device))

    def __call__(self, wave, n_valid, fused=False):
        spec = self.spectrogram(wave, n_valid)
        if self.train:
            spec = self.augment(spec)
        return spec, None
