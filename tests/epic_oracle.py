"""fp64 numpy restatement of the EPIC-Sounds log-mel of the reference (src/epic_sounds/epic_data/audio_loader_epicsounds.py:94-156:
librosa.stft(n_fft=2048, hann(240) centred in the frame, hop 120, center=True, zero padding) -> |X| -> HTK mel (norm=None, float32
filters) -> log(x + 1e-6) -> transpose -> edge-pad / crop to the target length), written as a direct DFT of each frame's win non-zero
samples.  No librosa: it is not available here, so parity with librosa itself is not pinned (as for the Kaldi fbank)."""
import math

import numpy as np


def hann_periodic(win):
    return 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(win) / win)


def frame_count(n, hop=120):
    """librosa center=True: 1 + n // hop frames"""
    return 1 + n // hop


def frame_start(t, hop=120, n_fft=2048, win=240):
    """first sample of the window's support in frame t (the clip is padded by n_fft // 2 zeros; the window sits (n_fft - win) // 2 in)"""
    return t * hop - n_fft // 2 + (n_fft - win) // 2


def magnitudes(x, n, frames, hop=120, n_fft=2048, win=240):
    """(len(frames), 1 + n_fft // 2) |X| in fp64: frames of x[:n] by a direct DFT of their win samples (phase-aligned with librosa)"""
    x = np.asarray(x, np.float64)[:n]
    w = hann_periodic(win)
    lpad = (n_fft - win) // 2
    seg = np.zeros((len(frames), win))
    for i, t in enumerate(frames):
        s = frame_start(t, hop, n_fft, win)
        lo, hi = max(s, 0), min(s + win, n)
        if hi > lo:
            seg[i, lo - s:hi - s] = x[lo:hi]
    seg *= w
    k = np.arange(1 + n_fft // 2)
    ang = -2.0 * math.pi * np.outer(np.arange(win) + lpad, k) / n_fft
    re, im = seg @ np.cos(ang), seg @ np.sin(ang)
    return np.sqrt(re * re + im * im)


def mel_energies(x, n, mel, target_length, hop=120, n_fft=2048, win=240):
    """(target_length, n_mels) fp64 mel energies (before the log), edge-padded / cropped"""
    nf = frame_count(n, hop)
    frames = [min(t, nf - 1) for t in range(target_length)]
    mag = magnitudes(x, n, frames, hop, n_fft, win)
    return mag @ np.asarray(mel, np.float32).astype(np.float64).T


def logmel(x, n, mel, target_length, eps=1e-6, **kw):
    return np.log(mel_energies(x, n, mel, target_length, **kw) + eps)


def check_logmel(got, x, n, mel, target_length, eps=1e-6, log_tol=1e-3, rel_floor=1e-4, mel_tol=1e-5, **kw):
    """the pass bar: |log| within log_tol wherever the fp64 mel energy is >= rel_floor of that frame's largest; elsewhere the mel energies
    (exp(log) - eps) within mel_tol of the frame's largest, absolute.  -> (worst log error where it applies, worst scaled mel error)"""
    e = mel_energies(x, n, mel, target_length, **kw)
    ref = np.log(e + eps)
    got = np.asarray(got, np.float64)
    top = e.max(axis=1, keepdims=True)
    big = e >= rel_floor * top
    d_log = np.abs(got - ref)
    worst_log = float(d_log[big].max()) if big.any() else 0.0
    d_mel = np.abs((np.exp(got) - eps) - e) / np.maximum(top, 1e-30)
    worst_mel = float(d_mel[~big].max()) if (~big).any() else 0.0
    silent = top[:, 0] == 0.0                     # an all-zero frame: exactly log(eps) everywhere
    if silent.any():
        worst_mel = max(worst_mel, float(np.abs(got[silent] - math.log(eps)).max()))
    assert worst_log <= log_tol and worst_mel <= mel_tol, (worst_log, worst_mel)
    return worst_log, worst_mel
