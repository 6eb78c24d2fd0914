"""Synthetic stand-in for the EPIC-Sounds data (there is no dataset in this image): `videos` float32 audio tracks at 24 kHz saved as
<video_id>.npy (the directory form `--epic_audio` reads), and EPIC_Sounds_train.pkl / EPIC_Sounds_validation.pkl annotation pickles
with the columns the reference reads (video_id, annotation_id, start_timestamp / stop_timestamp as HH:MM:SS.fff, class_id in 0..43).
Annotations are a mix of short (< 10 s) and long events; each class has its own tone.  Used to exercise `python -m aum.train --dataset
epic_sounds` end to end."""
import argparse
import os

import numpy as np


def stamp(sec):
    ms = int(round(sec * 1000))
    return f"{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d}.{ms % 1000:03d}"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--video-secs", type=float, default=60.0)
    ap.add_argument("--train", type=int, default=48)
    ap.add_argument("--val", type=int, default=16)
    ap.add_argument("--classes", type=int, default=44)
    a = ap.parse_args(argv)
    import pandas as pd
    sr = 24000
    os.makedirs(os.path.join(a.out, "audio"), exist_ok=True)
    os.makedirs(os.path.join(a.out, "annotations"), exist_ok=True)
    rng = np.random.default_rng(0)
    vids = [f"P{i:02d}_{i + 1:02d}" for i in range(a.videos)]
    n = int(a.video_secs * sr)
    tracks = {v: (rng.standard_normal(n) * 0.01).astype(np.float32) for v in vids}
    for split, count, fname in (("train", a.train, "EPIC_Sounds_train.pkl"), ("val", a.val, "EPIC_Sounds_validation.pkl")):
        rows = []
        for i in range(count):
            v = vids[int(rng.integers(a.videos))]
            dur = float(rng.choice([0.004, 0.5, 2.0, 5.1, 9.99, 10.0, 12.5]))
            start = float(rng.uniform(0.0, a.video_secs - dur - 0.01))
            cls = int(rng.integers(a.classes))
            lo, hi = int(start * sr), int((start + dur) * sr)
            t = np.arange(hi - lo) / sr
            tracks[v][lo:hi] += (0.2 * np.sin(2 * np.pi * (100.0 + 200.0 * cls) * t)).astype(np.float32)
            rows.append(dict(annotation_id=f"{v}_{split}_{i}", participant_id=v[:3], video_id=v, start_timestamp=stamp(start),
                             stop_timestamp=stamp(start + dur), start_sample=lo, stop_sample=hi, description="", class_id=cls))
        pd.DataFrame(rows).set_index("annotation_id", drop=False).to_pickle(os.path.join(a.out, "annotations", fname))
    for v, x in tracks.items():
        np.save(os.path.join(a.out, "audio", f"{v}.npy"), x)
    print(a.out)


if __name__ == "__main__":
    main()
