#!/usr/bin/env python3
"""Stochastic depth A/B at the bench shape: the AuM-Base bf16 training step (bench.py's step: waveform frontend, batch 64, fwd + BCE +
bwd + fused Adam) at drop_path_rate 0 and at a rate, in ONE process, the two models taking turns in blocks of steps.

    python tools/drop_path_ab.py [--rate 0.1] [--rounds 5] [--steps 10] [--warmup 5] [--batch 64] [--depth 24]

Each round times `--steps` steps of the rate-0 model, then of the rate model (host clock around work that ends in a device synchronise).
Prints one line per round and a JSON summary: per-arm median ms/step, the spread of each arm over the rounds, the difference.  The rate-0
arm launches the unscaled add + norm kernels only (asserted on the binding's launch names); the rate arm launches the scaled pair for
every block with a residual and for the final norm."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mamba-aum_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--size", default="base")
    args = ap.parse_args()
    from aum import tunable
    tunable.enable(0)              # GEMM solution selection as in bench.py, before torch issues any GEMM
    import torch
    import aum_hip
    from aum.frontend import FbankTables, WaveInput, prepare_wave
    from aum.model import build_aum
    if not torch.cuda.is_available():
        raise SystemExit("drop_path_ab.py measures on a GPU: none found")
    aum_hip.get()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    tabs = FbankTables(dev)
    wave = (torch.randn(args.batch, 160000, device=dev, generator=g) * 0.1).clamp_(-1, 1)
    fe = WaveInput(tabs, 1024)
    y = torch.zeros(args.batch, 527, device=dev)
    y.scatter_(1, torch.randint(0, 527, (args.batch, 2), device=dev, generator=g), 1.0)
    loss_fn = torch.nn.BCEWithLogitsLoss()

    def arm(rate):
        torch.manual_seed(3949)
        model = build_aum(args.size, depth=args.depth, num_classes=527, bimamba_type="v1", drop_path_rate=rate).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-7, betas=(0.95, 0.999), eps=1e-8, fused=True)

        def step():
            xin = prepare_wave(wave, None, tabs)[0]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = loss_fn(model(xin, frontend=fe).float(), y)
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            return loss
        return step

    arms = {"rate0": arm(0.0), f"rate{args.rate}": arm(args.rate)}
    names = {}
    real = aum_hip._launch
    current = [None]

    def counting(fn, a, t, lib, name, meta=None):
        names[current[0]][name] = names[current[0]].get(name, 0) + 1
        return real(fn, a, t, lib, name, meta)
    aum_hip._launch = counting
    for k, step in arms.items():
        current[0], names[k] = k, {}
        for _ in range(args.warmup):
            loss = step()
        assert torch.isfinite(loss).item(), k
    aum_hip._launch = real
    drop = {k: {n: c // args.warmup for n, c in v.items() if "rmsnorm" in n} for k, v in names.items()}
    assert not any("drop" in n for n in drop["rate0"]), drop
    times = {k: [] for k in arms}
    for r in range(args.rounds):
        for k, step in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        print(f"round {r}: " + "  ".join(f"{k} {times[k][-1]:.3f} ms/step" for k in arms), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    a, b = list(arms)
    print(json.dumps({"shape": {"size": args.size, "depth": args.depth, "batch": args.batch, "tokens": 513, "autocast": "bf16"},
                      "steps_per_block": args.steps, "rounds": args.rounds, "ms_per_step": {k: [round(t, 3) for t in v] for k, v in times.items()},
                      "median_ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
                      "rate_minus_rate0_ms": round(med[b] - med[a], 3), "norm_launches_per_step": drop}))


if __name__ == "__main__":
    main()
