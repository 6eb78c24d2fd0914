#!/usr/bin/env python3
"""Wall time of ONE 8-token hop (one time column of 16 x 16 patches on 128 mel bins) through a causal AuM, two ways, alternating in one
process: (a) eight rounds of the per-token Mamba.step through all blocks, (b) one AudioMamba.stream_push (Mamba.step_chunk).  HIP events
around each call, warm hops discarded, medians; the spread of (a) is the range of the medians of its repeat groups.

    python tools/stream_hop_bench.py [--size base] [--depth 24] [--batch 1 8] [--warm 20] [--hops 120] [--groups 4]
    python tools/stream_hop_bench.py --count-only a|b     (a few hops of one path only: for a kernel trace that counts launches per hop)

--pool S: S sessions at DIFFERENT positions, one hop each, three ways alternating in one process (same method):
  (a) S stream_push calls on S batch-1 caches -- the only way to serve staggered sessions without stream_push_many;
  (b) one stream_push_many for the S sessions at staggered offsets, one column each;
  (c) the same with ragged hops, k_i cycling through 1, 2, 1, 4 columns;
  and for reference the lockstep batch-S stream_push (all sessions at one position).
Arms (b) and (c) are skipped on a tree without stream_push_many, so the file also measures (a) on an older commit.

    python tools/stream_hop_bench.py --pool 8
    python tools/stream_hop_bench.py --pool 8 --count-only pa|pb|pc|lock

--fused-ab: stream_push (with --pool S: stream_push_many, staggered and ragged) with every block's conv, x/dt projections and scan as
three launches (aum_hip.debug.stream_fused off: the path before aum_stream_block_tm) against the one launch, alternating in one process.

    python tools/stream_hop_bench.py --fused-ab [--batch 1 8]        (--count-only a: three launches, b: one)
    python tools/stream_hop_bench.py --fused-ab --pool 8             (--count-only pb0|pc0: three launches, pb|pc: one)

--peek: "push, then tell me what you hear" two ways, same model, same hop, alternating in one process: (a) stream_push followed by
stream_read (a second pass of the cls row through all blocks), (b) one stream_push(read=True) (the cls row rides behind the hop's
tokens as a peek row); stream_push alone is timed as the third arm, so the cost of the read is visible in both forms.

    python tools/stream_hop_bench.py --peek [--batch 1 8]            (--count-only a: push + read, b: push(read=True))

--prefill COLS: a BACKLOG of COLS time columns (8 COLS tokens) into an empty session two ways, same model, same columns, alternating in
one process: (a) one stream_push (Mamba.step_chunk: the one-launch middle up to 128 tokens, else the three-launch ladder), (b) one
stream_prefill (Mamba.prefill_chunk: the time-parallel conv and the token-major scan with state in / state out).  The clip is made
long enough for the backlog (--prefill 512: 8192 frames, L = 4097).

    python tools/stream_hop_bench.py --prefill 31 [--batch 1]        (--count-only a: stream_push, b: stream_prefill)

--prefill-pool S --prefill COLS: S sessions JOIN WITH RAGGED BACKLOGS of COLS, COLS / 2, COLS / 4, ... columns (at least 1 each) into
empty rows of a pool, two ways alternating in one process, each arm on a pool of its own: (a) stream_prefill_many(packed=False), the host
loop of S batch-1 passes, (b) stream_prefill_many(packed=True), one packed pass.  Same method: HIP events around each call, warm calls
discarded, medians of all calls and of the groups, min / max.

    python tools/stream_hop_bench.py --prefill-pool 8 --prefill 64   (--count-only a: the loop, b: the packed pass)

--timeline COLS: the logits after EVERY one of COLS time columns of a new session two ways, same model, same columns, alternating in one
process: (a) the loop of COLS single-column stream_push(read=True) calls (one pass per column), (b) one stream_timeline of the COLS
columns (one pass over COLS x 9 rows, the cls row behind every column as a peek row).  One timed call is the whole clip piece in both
arms.  Same method: HIP events around each call, warm calls discarded, medians of all calls and of the groups, min / max.

    python tools/stream_hop_bench.py --timeline 64 [--batch 1]       (--count-only a: the per-column loop, b: stream_timeline)

--park N: N sessions of a pool of 2 N rows taken off the pool and brought back into other rows, with their sample tails, two ways
alternating in one process: (a) by hand -- per layer an index_select of conv_state and of ssm_state and one of the WaveStream tails
into held copies, then as many index_copy_ back: 2 (2 depth + 1) indexed copies; (b) one stream_park and one stream_resume (one launch
each).  One timed call is park + resume.  Same method: HIP events around each call, warm calls discarded, medians of all calls and of
the groups, min / max.

    python tools/stream_hop_bench.py --park 8 --hops 100             (--count-only a: by hand, b: stream_park + stream_resume)

--stack: stream_push (with --pool S: stream_push_many, staggered, one column each) without and with stack=model.stream_stack() -- the loop
over the layers against ONE aum_stream_layers call -- alternating in one process, each arm on caches of its own.  Same method: HIP events
around each call, warm hops discarded, medians of all hops and of the groups.  Next to each arm's time its HOST time: the wall clock from
entering the call to its return, before any synchronisation -- the Python, the checks and the enqueueing of the launches; a hop whose
host time is its whole time is bound by the host, one whose host time is a fraction of it waits for the kernels.

    python tools/stream_hop_bench.py --stack [--batch 1 8]           (--count-only a: the loop, b: stack=)
    python tools/stream_hop_bench.py --stack --pool 8                (--count-only a | b)
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mamba-aum_amd"))

from aum.model import AUM_SIZES, AudioMamba  # noqa: E402
from mamba_ssm.ops.triton.layernorm import rms_norm_fn  # noqa: E402


def make(size, depth, dev, frames=1024):
    torch.manual_seed(0)
    m = AudioMamba(spectrogram_size=(128, frames), depth=depth, embed_dim=AUM_SIZES[size], num_classes=527, bimamba_type="none",
                   use_middle_cls_token=False, use_end_cls_token=True, transpose_token_sequence=True)
    return m.eval().to(dev).to(torch.bfloat16)


def embed(model, spec, c0):
    """the 8 tokens of time column c0 (what stream_push builds before the blocks)"""
    nf, nt = model.patch_grid_size
    x = model.patch_embed(spec.unsqueeze(1).transpose(2, 3))
    pe = model.pos_embed.pos_embed[:, 1:].reshape(1, nf, nt, -1)[:, :, c0:c0 + 1]
    return (x.reshape(x.shape[0], nf, 1, -1) + pe).transpose(1, 2).reshape(x.shape[0], nf, -1)


def hop_steps(model, spec, cache):
    """path (a): the hop's tokens one at a time through every block's step()"""
    x = embed(model, spec, cache["columns"])
    for t in range(x.shape[1]):
        hidden, residual = x[:, t:t + 1], None
        for i, layer in enumerate(model.layers):
            hidden, residual = rms_norm_fn(hidden, layer.norm.weight, layer.norm.bias, residual=residual, prenorm=True, residual_in_fp32=True,
                                           eps=layer.norm.eps)
            hidden, _, _ = layer.mixer.step(hidden, *cache["layers"][i])
    cache["columns"] += 1


def hop_push(model, spec, cache):
    model.stream_push(spec, cache)


@contextlib.contextmanager
def stream_fused(on):
    """aum_hip.debug.stream_fused set for the block and put back to what it was (what AUM_DEBUG=1 AUM_STREAM_FUSED=0 sets for a process)"""
    import aum_hip
    was = aum_hip.debug.stream_fused
    aum_hip.debug.stream_fused = on
    try:
        yield
    finally:
        aum_hip.debug.stream_fused = was


def hop_push_unfused(model, spec, cache):
    """the path before aum_stream_block_tm: conv, x/dt projections and scan as three launches per block"""
    with stream_fused(False):
        model.stream_push(spec, cache)


def hop_push_fused(model, spec, cache):
    with stream_fused(True):
        model.stream_push(spec, cache)


def fused_ab(model, args, dev):
    """--fused-ab: one 8-token hop with the block's middle as three launches (a) against one launch (b), the arms alternating"""
    for B in args.batch:
        spec = torch.randn(B, 16, 128, device=dev, dtype=torch.bfloat16)
        ca, cb = model.allocate_inference_cache(B), model.allocate_inference_cache(B)
        if args.count_only:
            fn, c = (hop_push_unfused, ca) if args.count_only == "a" else (hop_push_fused, cb)
            for _ in range(args.count_hops):
                fn(model, spec, c)
            torch.cuda.synchronize()
            print(json.dumps({"path": "fused-ab " + args.count_only, "batch": B, "hops": args.count_hops}))
            continue
        for _ in range(args.warm):
            timed(hop_push_unfused, model, spec, ca)
            timed(hop_push_fused, model, spec, cb)
        ta, tb = [], []
        for _ in range(args.hops):
            ta.append(timed(hop_push_unfused, model, spec, ca))
            tb.append(timed(hop_push_fused, model, spec, cb))
        g = max(len(ta) // args.groups, 1)
        med = lambda t: [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
        print(json.dumps({"model": f"aum-{args.size} causal depth {args.depth} bf16", "batch": B, "hop_tokens": 8, "hops": args.hops, "warm": args.warm,
                          "three_launch_ms_median": round(statistics.median(ta), 4), "three_launch_ms_group_medians": med(ta),
                          "fused_ms_median": round(statistics.median(tb), 4), "fused_ms_group_medians": med(tb),
                          "ratio_three_over_fused": round(statistics.median(ta) / statistics.median(tb), 3)}), flush=True)


def stack_ab(model, args, dev):
    """--stack: one hop through the loop over the layers (a) against one aum_stream_layers call (b), the arms alternating"""
    stack = model.stream_stack()
    nt = model.patch_grid_size[1]
    cases = []
    if args.pool:
        S = args.pool
        specs = [torch.randn(16, 128, device=dev, dtype=torch.bfloat16) for _ in range(S)]
        pools = [model.allocate_stream_pool(S) for _ in range(2)]
        for p in pools:
            p["columns"] = [(7 * i) % (nt - 8) for i in range(S)]

        def many(i, st):
            def run():
                for j in range(S):
                    if pools[i]["columns"][j] + 1 > nt:
                        pools[i]["columns"][j] = 0        # a new clip: the caches' values do not matter for timing
                model.stream_push_many(specs, pools[i], range(S), stack=st)
            return run
        cases.append(({"sessions": S}, (("loop", many(0, None)), ("stack", many(1, stack)))))
    else:
        for B in args.batch:
            spec = torch.randn(B, 16, 128, device=dev, dtype=torch.bfloat16)
            caches = [model.allocate_inference_cache(B) for _ in range(2)]

            def push(i, st, spec=spec, caches=caches):
                def run():
                    if caches[i]["columns"] + 1 > nt:
                        caches[i]["columns"] = 0
                    model.stream_push(spec, caches[i], stack=st)
                return run
            cases.append(({"batch": B}, (("loop", push(0, None)), ("stack", push(1, stack)))))
    for tag, arms in cases:
        if args.count_only:
            name, fn = arms[0 if args.count_only == "a" else 1]
            for _ in range(args.count_hops):
                fn()
            torch.cuda.synchronize()
            print(json.dumps(dict(tag, path="stack " + name, hops=args.count_hops)))
            continue
        def timed_host(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            return a.elapsed_time(b), (t1 - t0) * 1e3

        for _ in range(args.warm):
            for _, fn in arms:
                timed_call(fn)
        times, host = [[] for _ in arms], [[] for _ in arms]
        for _ in range(args.hops):
            for t, h, (_, fn) in zip(times, host, arms):
                ms, hms = timed_host(fn)
                t.append(ms)
                h.append(hms)
        g = max(args.hops // args.groups, 1)
        out = dict(tag, model=f"aum-{args.size} causal depth {args.depth} bf16", hop_tokens=8, hops=args.hops, warm=args.warm)
        for (name, _), t, h in zip(arms, times, host):
            out[name + "_host_ms_median"] = round(statistics.median(h), 4)
            out[name + "_ms_median"] = round(statistics.median(t), 4)
            out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
            out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        out["ratio_loop_over_stack"] = round(out["loop_ms_median"] / out["stack_ms_median"], 3)
        print(json.dumps(out), flush=True)


def hop_push_then_read(model, spec, cache):
    model.stream_push(spec, cache)
    return model.stream_read(cache)


def hop_push_read(model, spec, cache):
    return model.stream_push(spec, cache, read=True)[1]


def peek_ab(model, args, dev):
    """--peek: one 8-token hop with its logits as push + stream_read (a) against one stream_push(read=True) (b); the plain push as (c)"""
    arms = (("push_then_read", hop_push_then_read), ("push_read_one_pass", hop_push_read), ("push_only", hop_push))
    for B in args.batch:
        spec = torch.randn(B, 16, 128, device=dev, dtype=torch.bfloat16)
        caches = [model.allocate_inference_cache(B) for _ in arms]
        if args.count_only:
            i = 0 if args.count_only == "a" else 1
            for _ in range(args.count_hops):
                arms[i][1](model, spec, caches[i])
            torch.cuda.synchronize()
            print(json.dumps({"path": "peek " + arms[i][0], "batch": B, "hops": args.count_hops}))
            continue
        for _ in range(args.warm):
            for (_, fn), c in zip(arms, caches):
                timed(fn, model, spec, c)
        times = [[] for _ in arms]
        for _ in range(args.hops):
            for t, (_, fn), c in zip(times, arms, caches):
                t.append(timed(fn, model, spec, c))
        g = max(args.hops // args.groups, 1)
        out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "batch": B, "hop_tokens": 8, "hops": args.hops, "warm": args.warm}
        for (name, _), t in zip(arms, times):
            out[name + "_ms_median"] = round(statistics.median(t), 4)
            out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
        out["ratio_two_pass_over_one_pass"] = round(out["push_then_read_ms_median"] / out["push_read_one_pass_ms_median"], 3)
        print(json.dumps(out), flush=True)


def backlog_push(model, spec, cache):
    cache["columns"] = 0                          # a new session every call: the caches' values do not matter for timing
    model.stream_push(spec, cache)


def backlog_prefill(model, spec, cache):
    cache["columns"] = 0
    model.stream_prefill(spec, cache)


def prefill_ab(model, args, dev):
    """--prefill COLS: a backlog of COLS columns as one stream_push (a) against one stream_prefill (b), the arms alternating"""
    arms = (("push", backlog_push), ("prefill", backlog_prefill))
    for B in args.batch:
        spec = torch.randn(B, 16 * args.prefill, 128, device=dev, dtype=torch.bfloat16)
        caches = [model.allocate_inference_cache(B) for _ in arms]
        if args.count_only:
            i = 0 if args.count_only == "a" else 1
            for _ in range(args.count_hops):
                arms[i][1](model, spec, caches[i])
            torch.cuda.synchronize()
            print(json.dumps({"path": "prefill " + arms[i][0], "batch": B, "columns": args.prefill, "hops": args.count_hops}))
            continue
        for _ in range(args.warm):
            for (_, fn), c in zip(arms, caches):
                timed(fn, model, spec, c)
        times = [[] for _ in arms]
        for _ in range(args.hops):
            for t, (_, fn), c in zip(times, arms, caches):
                t.append(timed(fn, model, spec, c))
        g = max(args.hops // args.groups, 1)
        out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "batch": B, "columns": args.prefill, "tokens": 8 * args.prefill,
               "clip_columns": model.patch_grid_size[1], "hops": args.hops, "warm": args.warm}
        for (name, _), t in zip(arms, times):
            out[name + "_ms_median"] = round(statistics.median(t), 4)
            out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
            out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        out["ratio_push_over_prefill"] = round(out["push_ms_median"] / out["prefill_ms_median"], 3)
        print(json.dumps(out), flush=True)


def timeline_loop(model, spec, cache):
    cache["columns"] = 0                          # a new session every call: the caches' values do not matter for timing
    return [model.stream_push(spec[:, 16 * j:16 * (j + 1)], cache, read=True)[1] for j in range(spec.shape[1] // 16)]


def timeline_one_pass(model, spec, cache):
    cache["columns"] = 0
    return model.stream_timeline(spec, cache)[1]


def timeline_ab(model, args, dev):
    """--timeline COLS: the logits after every one of COLS columns as COLS stream_push(read=True) calls (a) against one stream_timeline (b)"""
    arms = (("loop", timeline_loop), ("timeline", timeline_one_pass))
    for B in args.batch:
        spec = torch.randn(B, 16 * args.timeline, 128, device=dev, dtype=torch.bfloat16)
        caches = [model.allocate_inference_cache(B) for _ in arms]
        if args.count_only:
            i = 0 if args.count_only == "a" else 1
            for _ in range(args.count_hops):
                arms[i][1](model, spec, caches[i])
            torch.cuda.synchronize()
            print(json.dumps({"path": "timeline " + arms[i][0], "batch": B, "columns": args.timeline, "hops": args.count_hops}))
            continue
        for _ in range(args.warm):
            for (_, fn), c in zip(arms, caches):
                timed(fn, model, spec, c)
        times = [[] for _ in arms]
        for _ in range(args.hops):
            for t, (_, fn), c in zip(times, arms, caches):
                t.append(timed(fn, model, spec, c))
        g = max(args.hops // args.groups, 1)
        out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "batch": B, "columns": args.timeline, "rows_one_pass": 9 * args.timeline,
               "clip_columns": model.patch_grid_size[1], "hops": args.hops, "warm": args.warm}
        for (name, _), t in zip(arms, times):
            out[name + "_ms_median"] = round(statistics.median(t), 4)
            out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
            out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        out["ratio_loop_over_timeline"] = round(out["loop_ms_median"] / out["timeline_ms_median"], 3)
        print(json.dumps(out), flush=True)


def wave_ab(model, args, dev):
    """--wave: 8 sessions, one hop of 2560 samples (one column) each per call -- by hand (a: per session the carried 240 samples and the hop
    concatenated on the host side, fbank_fwd on the assembled buffer, then stream_push_many) against one stream_push_wave_many (b)"""
    import aum_hip
    from aum.frontend import FbankTables, WaveInput
    S, hop = 8, 2560
    fe = WaveInput(FbankTables(dev), target_length=16 * model.patch_grid_size[1])
    pools = [model.allocate_stream_pool(S), model.allocate_stream_pool(S)]
    ws = model.allocate_wave_stream(S, fe)
    pcm = [torch.randn(hop, device=dev) * 0.1 for _ in range(S)]
    held = [torch.zeros(240, device=dev) for _ in range(S)]
    model.stream_push_wave_many(held, pools[1], ws, range(S))                 # both arms start with the 240 samples frames share

    def by_hand():
        if pools[0]["columns"][0] >= model.patch_grid_size[1]:
            pools[0]["columns"] = [0] * S             # new clips: the caches' values do not matter for timing
        specs = []
        for i in range(S):
            buf = torch.cat((held[i], pcm[i]))
            specs.append(aum_hip.fbank_fwd(buf[None], fe.tables.tables, 16, fe.norm_mean, fe.norm_std)[0].to(torch.bfloat16))
            held[i] = buf[-240:]
        model.stream_push_many(specs, pools[0], range(S))

    def one_call():
        if pools[1]["columns"][0] >= model.patch_grid_size[1]:
            pools[1]["columns"] = [0] * S
            ws.reset(range(S))
            model.stream_push_wave_many([h[:240] for h in pcm], pools[1], ws, range(S))
        model.stream_push_wave_many(pcm, pools[1], ws, range(S))

    arms = (("by_hand", by_hand), ("push_wave_many", one_call))
    for _ in range(args.warm):
        for _, fn in arms:
            timed_call(fn)
    times = [[] for _ in arms]
    for _ in range(args.hops):
        for t, (_, fn) in zip(times, arms):
            t.append(timed_call(fn))
    g = max(args.hops // args.groups, 1)
    out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "sessions": S, "hop_samples": hop, "hops": args.hops, "warm": args.warm}
    for (name, _), t in zip(arms, times):
        out[name + "_ms_median"] = round(statistics.median(t), 4)
        out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
        out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    out["ratio_by_hand_over_push_wave_many"] = round(out["by_hand_ms_median"] / out["push_wave_many_ms_median"], 3)
    print(json.dumps(out), flush=True)


def park_ab(model, args, dev):
    """--park N: park + resume of N sessions (with sample tails) as 2 (2 depth + 1) indexed copies (a) against one launch each way (b)"""
    from aum.frontend import FbankTables, WaveInput
    N = args.park
    fe = WaveInput(FbankTables(dev), target_length=16 * model.patch_grid_size[1])
    pool, ws = model.allocate_stream_pool(2 * N), model.allocate_wave_stream(2 * N, fe)
    for c, s in pool["layers"].values():
        c.normal_(), s.normal_()
    src, dst = list(range(0, 2 * N, 2)), list(range(1, 2 * N, 2))
    i_src, i_dst = torch.tensor(src, device=dev), torch.tensor(dst, device=dev)
    tensors = model._park_tensors(pool, ws)

    def by_hand():
        held = [t.index_select(0, i_src) for t in tensors]
        for t, h in zip(tensors, held):
            t.index_copy_(0, i_dst, h)

    def one_launch_each():
        model.stream_resume(model.stream_park(pool, src, wave_stream=ws), pool, dst, wave_stream=ws)

    arms = (("by_hand", by_hand), ("park_resume", one_launch_each))
    if args.count_only:
        i = 0 if args.count_only == "a" else 1
        for _ in range(args.count_hops):
            arms[i][1]()
        torch.cuda.synchronize()
        print(json.dumps({"path": "park " + arms[i][0], "sessions": N, "hops": args.count_hops}))
        return
    for _ in range(args.warm):
        for _, fn in arms:
            timed_call(fn)
    times = [[] for _ in arms]
    for _ in range(args.hops):
        for t, (_, fn) in zip(times, arms):
            t.append(timed_call(fn))
    g = max(args.hops // args.groups, 1)
    import aum_hip
    out = {"model": f"aum-{args.size} causal depth {args.depth}", "sessions": N, "pool_rows": 2 * N, "pool_tensors": len(tensors),
           "record_bytes": aum_hip.stream_park_layout(tensors).record, "indexed_copies_by_hand": 2 * len(tensors), "hops": args.hops, "warm": args.warm}
    for (name, _), t in zip(arms, times):
        out[name + "_ms_median"] = round(statistics.median(t), 4)
        out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
        out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    out["ratio_by_hand_over_park_resume"] = round(out["by_hand_ms_median"] / out["park_resume_ms_median"], 3)
    print(json.dumps(out), flush=True)


def prefill_pool_ab(model, args, dev):
    """--prefill-pool S --prefill COLS: S ragged backlogs into empty pool rows, the host loop (a) against one packed pass (b)"""
    S = args.prefill_pool
    ks = [max(args.prefill >> i, 1) for i in range(S)]
    specs = [torch.randn(16 * k, 128, device=dev, dtype=torch.bfloat16) for k in ks]
    arms = (("loop", False), ("packed", True))
    pools = [model.allocate_stream_pool(S) for _ in arms]

    def call(i):
        pools[i]["columns"] = [0] * S             # new sessions every call: the caches' values do not matter for timing
        model.stream_prefill_many(specs, pools[i], range(S), packed=arms[i][1])

    if args.count_only:
        i = 0 if args.count_only == "a" else 1
        for _ in range(args.count_hops):
            call(i)
        torch.cuda.synchronize()
        print(json.dumps({"path": "prefill-pool " + arms[i][0], "sessions": S, "columns": ks, "hops": args.count_hops}))
        return
    for _ in range(args.warm):
        for i in range(len(arms)):
            timed_call(lambda: call(i))
    times = [[] for _ in arms]
    for _ in range(args.hops):
        for i, t in enumerate(times):
            t.append(timed_call(lambda: call(i)))
    g = max(args.hops // args.groups, 1)
    out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "sessions": S, "columns": ks, "tokens": 8 * sum(ks),
           "clip_columns": model.patch_grid_size[1], "hops": args.hops, "warm": args.warm}
    for (name, _), t in zip(arms, times):
        out[name + "_ms_median"] = round(statistics.median(t), 4)
        out[name + "_ms_group_medians"] = [round(statistics.median(t[i:i + g]), 4) for i in range(0, g * args.groups, g)]
        out[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    out["ratio_loop_over_packed"] = round(out["loop_ms_median"] / out["packed_ms_median"], 3)
    print(json.dumps(out), flush=True)


def timed(fn, model, spec, cache):
    if cache["columns"] >= model.patch_grid_size[1]:
        cache["columns"] = 0                      # a new clip: the caches' values do not matter for timing
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(model, spec, cache)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


RAGGED = (1, 2, 1, 4)


def pool_arms(model, S, dev):
    """-> {arm: (callable doing one hop of all S sessions, columns served per hop)}"""
    nt = model.patch_grid_size[1]
    piece = lambda k: torch.randn(16 * k, 128, device=dev, dtype=torch.bfloat16)
    start = [(7 * i) % (nt - 8) for i in range(S)]                  # staggered offsets into the clips
    solo = [model.allocate_inference_cache(1) for _ in range(S)]
    for c, c0 in zip(solo, start):
        c["columns"] = c0
    one = [piece(1) for _ in range(S)]

    def wrap(columns, i, k):
        if columns[i] + k > nt:
            columns[i] = 0                                          # a new clip: the caches' values do not matter for timing

    def arm_a():
        for c, sp in zip(solo, one):
            if c["columns"] + 1 > nt:
                c["columns"] = 0
            model.stream_push(sp.unsqueeze(0), c)

    lock_cache = model.allocate_inference_cache(S)
    lock_spec = torch.randn(S, 16, 128, device=dev, dtype=torch.bfloat16)

    def arm_lock():
        if lock_cache["columns"] + 1 > nt:
            lock_cache["columns"] = 0
        model.stream_push(lock_spec, lock_cache)

    arms = {"a_solo_pushes": (arm_a, S), "lockstep_batch_push": (arm_lock, S)}
    if hasattr(model, "stream_push_many"):
        pools = {}
        for name, ks in (("b_push_many", [1] * S), ("c_push_many_ragged", [RAGGED[i % len(RAGGED)] for i in range(S)])):
            pool = model.allocate_stream_pool(S)
            pool["columns"] = list(start)
            pools[name] = (pool, ks, [piece(k) for k in ks])

        def many(name):
            pool, ks, specs = pools[name]
            for i, k in enumerate(ks):
                wrap(pool["columns"], i, k)
            model.stream_push_many(specs, pool, range(S))

        arms["b_push_many"] = (lambda: many("b_push_many"), S)
        arms["c_push_many_ragged"] = (lambda: many("c_push_many_ragged"), sum(pools["c_push_many_ragged"][1]))
    return arms


def timed_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pool_fused_arms(model, S, dev):
    """--fused-ab --pool S: stream_push_many, staggered and ragged, with the block's middle as three launches against one launch; every
    arm advances a pool of its own"""
    sets = {"three_launch": (False, pool_arms(model, S, dev)), "fused": (True, pool_arms(model, S, dev))}

    def under(on, fn):
        def run():
            with stream_fused(on):
                fn()
        return run

    arms = {}
    for k in ("b_push_many", "c_push_many_ragged"):
        for tag, (on, base) in sets.items():
            arms[f"{k}_{tag}"] = (under(on, base[k][0]), base[k][1])
    return arms


COUNT_ARMS = {"pa": "a_solo_pushes", "pb": "b_push_many", "pc": "c_push_many_ragged", "lock": "lockstep_batch_push"}
COUNT_ARMS_FUSED_AB = {"pb0": "b_push_many_three_launch", "pb": "b_push_many_fused", "pc0": "c_push_many_ragged_three_launch",
                       "pc": "c_push_many_ragged_fused"}


def pool_main(model, args, dev):
    S = args.pool
    arms = pool_fused_arms(model, S, dev) if args.fused_ab else pool_arms(model, S, dev)
    if args.count_only:
        name = (COUNT_ARMS_FUSED_AB if args.fused_ab else COUNT_ARMS)[args.count_only]
        for _ in range(args.count_hops):
            arms[name][0]()
        torch.cuda.synchronize()
        print(json.dumps({"path": name, "sessions": S, "hops": args.count_hops}))
        return
    for _ in range(args.warm):
        for fn, _ in arms.values():
            timed_call(fn)
    times = {k: [] for k in arms}
    for _ in range(args.hops):
        for k, (fn, _) in arms.items():
            times[k].append(timed_call(fn))
    g = max(args.hops // args.groups, 1)
    out = {"model": f"aum-{args.size} causal depth {args.depth} bf16", "sessions": S, "hops": args.hops, "warm": args.warm}
    for k, v in times.items():
        out[k] = {"ms_median": round(statistics.median(v), 4), "columns_per_hop": arms[k][1],
                  "ms_group_medians": [round(statistics.median(v[i:i + g]), 4) for i in range(0, g * args.groups, g)]}
    for k in ("b_push_many", "c_push_many_ragged"):
        if k + "_fused" in out:
            out[f"ratio_{k}_three_over_fused"] = round(out[k + "_three_launch"]["ms_median"] / out[k + "_fused"]["ms_median"], 3)
    if "b_push_many" in out:
        out["ratio_a_over_b"] = round(out["a_solo_pushes"]["ms_median"] / out["b_push_many"]["ms_median"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--hops", type=int, default=120)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--pool", type=int, default=0, help="S sessions at different positions: S stream_push calls vs one stream_push_many")
    ap.add_argument("--count-only", choices=["a", "b", "pa", "pb", "pc", "lock", "pb0", "pc0"])
    ap.add_argument("--count-hops", type=int, default=4)
    ap.add_argument("--fused-ab", action="store_true", help="stream_push with the block's middle as three launches vs aum_stream_block_tm")
    ap.add_argument("--peek", action="store_true", help="stream_push + stream_read vs one stream_push(read=True)")
    ap.add_argument("--prefill", type=int, default=0, metavar="COLS", help="a backlog of COLS columns: one stream_push vs one stream_prefill")
    ap.add_argument("--prefill-pool", type=int, default=0, metavar="S",
                    help="with --prefill COLS: S sessions with backlogs of COLS, COLS / 2, ... columns, stream_prefill_many as a host loop vs packed")
    ap.add_argument("--timeline", type=int, default=0, metavar="COLS",
                    help="the logits after every one of COLS columns: COLS stream_push(read=True) calls vs one stream_timeline")
    ap.add_argument("--wave", action="store_true",
                    help="raw audio: 8 sessions by hand (tail + hop on the host side, fbank_fwd, stream_push_many) vs one stream_push_wave_many")
    ap.add_argument("--park", type=int, default=0, metavar="N",
                    help="N sessions off a pool and back into other rows: 2 (2 depth + 1) indexed copies vs one stream_park + one stream_resume")
    ap.add_argument("--stack", action="store_true", help="stream_push / stream_push_many without and with stack=model.stream_stack()")
    args = ap.parse_args()
    dev = "cuda:0"
    model = make(args.size, args.depth, dev, max(1024, 16 * args.prefill, 16 * args.timeline))
    if args.stack:
        with torch.no_grad():
            stack_ab(model, args, dev)
        return
    if args.park:
        with torch.no_grad():
            park_ab(model, args, dev)
        return
    if args.wave:
        with torch.no_grad():
            wave_ab(model, args, dev)
        return
    if args.timeline:
        with torch.no_grad():
            timeline_ab(model, args, dev)
        return
    if args.prefill_pool:
        if not args.prefill:
            ap.error("--prefill-pool S needs --prefill COLS")
        with torch.no_grad():
            prefill_pool_ab(model, args, dev)
        return
    if args.prefill:
        with torch.no_grad():
            prefill_ab(model, args, dev)
        return
    if args.pool:
        with torch.no_grad():
            pool_main(model, args, dev)
        return
    if args.fused_ab:
        with torch.no_grad():
            fused_ab(model, args, dev)
        return
    if args.peek:
        with torch.no_grad():
            peek_ab(model, args, dev)
        return
    with torch.no_grad():
        for B in args.batch:
            spec = torch.randn(B, 16, 128, device=dev, dtype=torch.bfloat16)
            ca, cb = model.allocate_inference_cache(B), model.allocate_inference_cache(B)
            if args.count_only:
                fn, c = (hop_steps, ca) if args.count_only == "a" else (hop_push, cb)
                for _ in range(args.count_hops):
                    fn(model, spec, c)
                torch.cuda.synchronize()
                print(json.dumps({"path": args.count_only, "batch": B, "hops": args.count_hops}))
                continue
            for _ in range(args.warm):
                timed(hop_steps, model, spec, ca)
                timed(hop_push, model, spec, cb)
            ta, tb = [], []
            for _ in range(args.hops):
                ta.append(timed(hop_steps, model, spec, ca))
                tb.append(timed(hop_push, model, spec, cb))
            g = max(len(ta) // args.groups, 1)
            meds_a = [statistics.median(ta[i:i + g]) for i in range(0, g * args.groups, g)]
            meds_b = [statistics.median(tb[i:i + g]) for i in range(0, g * args.groups, g)]
            ma, mb = statistics.median(ta), statistics.median(tb)
            print(json.dumps({"model": f"aum-{args.size} causal depth {args.depth} bf16", "batch": B, "hop_tokens": 8, "hops": args.hops, "warm": args.warm,
                              "steps_ms_median": round(ma, 4), "steps_ms_group_medians": [round(v, 4) for v in meds_a],
                              "push_ms_median": round(mb, 4), "push_ms_group_medians": [round(v, 4) for v in meds_b],
                              "ratio_steps_over_push": round(ma / mb, 3)}), flush=True)


if __name__ == "__main__":
    main()
