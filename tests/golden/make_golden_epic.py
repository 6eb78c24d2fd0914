#!/usr/bin/env python3
"""Generate tests/golden/epic_specaug.npz: the REFERENCE's own SpecAugment of the EPIC-Sounds recipe
(src/epic_sounds/epic_data/spec_augment.py = "SA": combined_transforms = time_warp(W=5) -> freq_mask x 2 -> time_mask x 2, SA:346-413),
run on the CPU on small seeded spectrograms.  Runs only where the reference is present (no-op elsewhere).  SA imports only torch and
random; it is loaded from its file and nothing of it is copied.

Per case (spectrogram (1, 128, T) from a numpy seed, Python `random` seed, torch seed, mask widths):
  pos / point / dist   the time warp's draws: the frame of the control value, that value (row 64), the shift
  f_bands / t_bands    [lo, hi) of each mask that ran (the draw sequence recorded through SA's `random`), -1 rows for masks that did not
  eps                  the (1, 3, 3) randn * 1e-7 block of solve_interpolation (torch's global generator after the torch seed)
  w, v                 solve_interpolation's coefficients (1, 1, 2), (1, 3, 2)
  flow                 the dense time flow (128, T) (the frequency flow is checked to be exactly 0 here)
  warped / out         time_warp's output and the whole chain's output, (128, T)
torch runs single-threaded, as in a DataLoader worker (the grid sum of SA:140 is one float32 reduction)."""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SA_PATH = os.path.join(REF, "src", "epic_sounds", "epic_data", "spec_augment.py")

# (name, frames, numpy seed, python seed, torch seed, F_MASK, T_MASK)
CASES = [
    ("t96", 96, 11, 101, 1001, 48, 30),
    ("t80", 80, 12, 7, 2002, 48, 20),
    ("t64", 64, 13, 4242, 3003, 20, 12),
]
W = 5


def spectrogram(seed, frames):
    """log-mel-like values: a smooth random field around -8 (so that the bilinear samples of a warp move by small amounts)"""
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.standard_normal((128, frames)) * 0.3, axis=1)
    base += np.cumsum(rng.standard_normal((128, 1)) * 0.5, axis=0)
    return (base - 8.0).astype(np.float32)


class _Rec:
    """SA's `random`, recording randrange draws"""

    def __init__(self):
        self.calls = []

    def randrange(self, *a):
        r = random.randrange(*a)
        self.calls.append((a, r))
        return r

    def uniform(self, *a):
        return random.uniform(*a)


class _Cfg:
    def __init__(self, f, t):
        self.F_MASK, self.T_MASK, self.T_WARP = f, t, W


def main():
    if not os.path.exists(SA_PATH):
        print("reference not present: nothing to do")
        return
    import torch
    torch.set_num_threads(1)
    spec_ = importlib.util.spec_from_file_location("ref_spec_augment", SA_PATH)
    sa = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(sa)
    out = {}
    for name, frames, nseed, pseed, tseed, fm, tm in CASES:
        x = torch.tensor(spectrogram(nseed, frames)).unsqueeze(0)
        # the whole chain, draws recorded
        rec = _Rec()
        sa.random = rec
        random.seed(pseed)
        torch.manual_seed(tseed)
        full = sa.combined_transforms(x.clone(), _Cfg(fm, tm))
        sa.random = random
        calls = rec.calls
        pos, dist = calls[0][1], calls[1][1]
        bands = {"f": [], "t": []}
        i = 2
        for kind in ("f", "t"):
            for _ in range(2):
                wdt, zero = calls[i][1], calls[i + 1][1]
                i += 2
                if wdt == 0:
                    break
                bands[kind].append((zero, calls[i][1]))
                i += 1
        assert i == len(calls), (name, calls)
        # the time warp again, step by step (SA:346-360), for its intermediate values
        random.seed(pseed)
        torch.manual_seed(tseed)
        y = x.shape[1] // 2
        p = random.randrange(W, frames - W)
        point = x[0][y][p]
        d = random.randrange(-W, W)
        assert (p, d) == (pos, dist)
        src, dst = torch.tensor([[[y, point]]]), torch.tensor([[[y, point + d]]])
        st = torch.get_rng_state()
        eps = torch.randn((1, 3, 3)) * 1e-7
        torch.set_rng_state(st)
        w, v = sa.solve_interpolation(dst, dst - src, 2, 0.0)
        torch.set_rng_state(st)
        warped, flows = sa.sparse_image_warp(x.clone(), src, dst)
        warped = warped.squeeze(3)
        torch.set_rng_state(st)
        random.seed(pseed)
        assert torch.equal(warped, sa.time_warp(x.clone(), W=W))
        assert float(flows[..., 0].abs().max()) == 0.0
        random.seed(pseed)
        random.randrange(W, frames - W), random.randrange(-W, W)
        assert torch.equal(full, sa.time_mask(sa.freq_mask(warped, F=fm, num_masks=2), T=tm, num_masks=2))
        fb = np.full((2, 2), -1, np.int64)
        tb = np.full((2, 2), -1, np.int64)
        for k, b in enumerate(bands["f"]):
            fb[k] = b
        for k, b in enumerate(bands["t"]):
            tb[k] = b
        meta = np.array([frames, nseed, pseed, tseed, fm, tm, W, pos, dist], np.int64)
        out[f"{name}_meta"] = meta
        out[f"{name}_point"] = np.float32(point)
        out[f"{name}_f_bands"], out[f"{name}_t_bands"] = fb, tb
        out[f"{name}_eps"] = eps.numpy()
        out[f"{name}_w"], out[f"{name}_v"] = w.numpy(), v.numpy()
        out[f"{name}_flow"] = flows[0, :, :, 1].numpy()
        out[f"{name}_warped"] = warped[0].numpy()
        out[f"{name}_out"] = full[0].numpy()
        print(name, "pos", pos, "dist", dist, "bands", bands, "flow range", float(flows[..., 1].min()), float(flows[..., 1].max()))
    out["case_names"] = np.array([c[0] for c in CASES])
    np.savez(os.path.join(HERE, "epic_specaug.npz"), **out)


if __name__ == "__main__":
    main()
