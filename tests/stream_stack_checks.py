"""A streaming hop through all blocks in one library call: aum_stream_in_tm (add + RMSNorm + in_proj), aum_stream_out_tm (out_proj),
aum_stream_layers (the C loop over the blocks) and AudioMamba.stream_stack / stack=.  Shared by tests/test_stream_stack.py (the lane-array
build of the kernel sources, host tensors) and tests/test_gpu_stream_stack.py (the device library).

Shapes: the three (d_model, d_inner) pairs the kernels are built for; total in {1, 9, 16, 17, 33, 73} -- below one MFMA tile of 16 rows, one
tile, one tile + 1, several tiles, 8 sessions x 9 rows + 1; depth 3 for the chain.

  1 norm prologue     W_in = [identity ; 0]: xz[:, :d_model] is the normed row itself, bit for bit aum_hip.rmsnorm_fwd's, residual_out its
                      residual; with and without residual_in
  2 exact inputs      Part A of gemm_exact_checks (integers times a power of two, sum |a||b| < 2^24 quanta): stream_out with the gemm_tn
                      recipes; stream_in with rows of hidden + residual of constant magnitude 2^j (j per row) and integer norm weights in
                      [-15, 15], so that the normed row is exactly +-w_norm (asserted on the fp64 reference first).  Conditions 1 and 2
                      (exact sums, finite, no subnormals) are asserted per total; conditions 3 and 4 (the shares of inexact results and
                      of ties, ties in both directions, what the other rounding modes change) are shares: a single row at total = 1 has
                      too few elements to hold them, so they are asserted per total from 9 rows on AND over the rows of all six totals
                      together (pooled_conditions), the total = 1 row among them
  3 random inputs     Part B: rn(ref - e) <= out <= rn(ref + e), e = k 2^-23 (|a| @ |b|^T); stream_in's operand a is the kernel's own
                      normed row (the bit-pinned one of check 1)
  4 partition         the rows of one call cut at (1, 7, 8, 16, 1) of 33 and reordered: every row's bits are the same
  5 chain             aum_stream_layers at depth 3 == the Python loop stream_in -> stream_block -> stream_out, bit for bit: hidden,
                      residual, every pool row; rows the map does not name keep their poison
  6 refusals          return the code, write nothing; stream_layers_supported agrees
  7 model             stack arm and default arm against model(spec) (2e-2, the bar of stream_block_checks), the stack arm's error at most
                      twice the default arm's; one hop of 4 columns == 4 hops of 1 column; stream_read(stack=) leaves the caches alone
  8 one call per hop  one stream_push(stack=) is one aum_stream_layers and no aum_rmsnorm_fwd / aum_stream_block_tm from Python
  9 stack cache       a no_grad write and a load_state_dict rebuild it; unsupported models raise with the reason
"""
import contextlib

import numpy as np
import pytest
import torch

import aum_hip
import gemm_exact_checks as gx
import stream_block_checks as sb
import stream_checks as sc
from conftest import rel_err
from stream_prefill_checks import product_lib

BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = (BF16, FP16)
WIDTHS = aum_hip.STREAM_STACK_WIDTHS
TOTALS = (1, 9, 16, 17, 33, 73)
XDT = {384: (48, 16), 768: (56, 24), 1536: (80, 48)}          # d_inner -> (x_dbl columns, rank) of AuM-Tiny / -Small / -Base
EPS = 1e-5
POISON = -7.25


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
def norm_operands(widths, dtype, total, device, with_res, seed=0):
    dm, dim = widths
    g = gx._gen("stack norm", widths, gx.DT_ID[dtype], total, with_res, seed)
    hidden = torch.randn(total, dm, generator=g).to(dtype).to(device)
    res = (torch.randn(total, dm, generator=g) * 3).to(device) if with_res else None
    w_norm = (1 + 0.1 * torch.randn(dm, generator=g)).to(device)
    return hidden, res, w_norm


def check_norm_prologue(lib, device, widths, dtype, total, with_res):
    dm, dim = widths
    hidden, res, w_norm = norm_operands(widths, dtype, total, device, with_res)
    w_in = torch.zeros(2 * dim, dm, dtype=dtype, device=device)
    w_in[:dm] = torch.eye(dm, dtype=dtype, device=device)
    xz, res_out = aum_hip.stream_in(hidden, w_norm, w_in, residual=res, eps=EPS, lib=lib)
    y, _, r = aum_hip.rmsnorm_fwd(hidden, w_norm, residual=res, eps=EPS, residual_dtype=torch.float32, lib=lib)
    _sync(device)
    gx.assert_bits(("norm prologue residual", widths, total), res_out, r)
    gx.assert_bits(("norm prologue normed row", widths, total), xz[:, :dm].contiguous(), y)
    assert not xz[:, dm:].any()
    return y


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
def out_operands(widths, dtype, total, exact):
    dm, dim = widths
    return gx.gemm_operands((total, dm, dim, 0, 0), dtype, exact)


def out_conditions(widths, dtype, total):
    o = out_operands(widths, dtype, total, True)
    if total < 9:           # the shares of a single row are not statistics: conditions 1 and 2 only
        return gx.check_conditions(("stream_out", widths, total), dtype, o["ref"], o["absum"], o["q"], rounded=False)
    return gx.check_conditions(("stream_out", widths, gx.DT_ID[dtype], total), dtype, o["ref"], o["absum"], o["q"])


def pooled_conditions(widths, dtype):
    """conditions 1 - 4 of Part A over the rows of ALL totals together, for both products: no total is exempt from the shares"""
    outs = [out_operands(widths, dtype, t, True) for t in TOTALS]
    ins = [in_exact_operands(widths, dtype, t) for t in TOTALS]
    cat = lambda os, k: torch.cat([o[k] for o in os], dim=0)
    a = gx.check_conditions(("stream_out pooled", widths, gx.DT_ID[dtype]), dtype, cat(outs, "ref"), cat(outs, "absum"), outs[0]["q"])
    b = gx.check_conditions(("stream_in pooled", widths, gx.DT_ID[dtype]), dtype, cat(ins, "ref"), cat(ins, "absum"), ins[0]["q"])
    return a, b


def check_out_exact(lib, device, widths, dtype, total):
    o = out_operands(widths, dtype, total, True)
    out = aum_hip.stream_out(o["a"].to(dtype).to(device), o["b"].to(dtype).to(device), lib=lib)
    _sync(device)
    gx.assert_bits(("stream_out exact", widths, gx.DT_ID[dtype], total), out, gx.rn16(o["ref"], dtype))


def in_exact_operands(widths, dtype, total):
    """hidden + residual = +-2^j per row (hidden +-2^j or 0 where the residual carries the entry), w_norm integers in [-15, 15]: mean square
    4^j, rstd = 1 / sqrt(4^j + eps) rounds v * rstd to +-1 times (1 - 2.5e-6 4^-j): times w_norm and rounded to 8 / 11 bits it is w_norm
    exactly for j >= 0 (asserted in in_conditions).  W_in by the gemm_tn recipe."""
    dm, dim = widths
    g = gx._gen("stack in exact", widths, gx.DT_ID[dtype], total)
    j = torch.randint(0, 4, (total, 1), generator=g).double()
    sign = torch.randint(0, 2, (total, dm), generator=g).double() * 2 - 1
    v = sign * 2.0 ** j
    from_res = torch.randint(0, 2, (total, dm), generator=g).bool()
    hidden, res = torch.where(from_res, torch.zeros_like(v), v), torch.where(from_res, v, torch.zeros_like(v))
    w_norm = torch.randint(-15, 16, (dm,), generator=g).double()
    _, rb, _ = gx.recipe("gemm", dtype, dm)
    w_in = gx.ints(g, (2 * dim, dm), *rb)
    normed = sign * w_norm
    return dict(hidden=hidden, res=res, v=v, w_norm=w_norm, w_in=w_in, normed=normed, ref=normed @ w_in.t(), absum=normed.abs() @ w_in.abs().t(),
                q=gx.quantum((15, 0), rb))


def in_conditions(widths, dtype, total):
    """on the fp64 reference alone: the reference normed rows ARE the integers (computed as the kernel does, in fp32 steps, and in fp64),
    and the product obeys Part A's conditions"""
    o = in_exact_operands(widths, dtype, total)
    v32 = o["v"].float()
    ms = (v32 * v32).sum(dim=1, keepdim=True) / v32.shape[1]
    rstd = 1.0 / torch.sqrt(ms + torch.tensor(EPS, dtype=torch.float32))
    y32 = (v32 * rstd * o["w_norm"].float()).to(dtype).double()
    assert torch.equal(y32, o["normed"]), "the fp32 normed row is not the integer row"
    y64 = (o["v"] / torch.sqrt((o["v"] ** 2).mean(dim=1, keepdim=True) + EPS) * o["w_norm"])
    assert torch.equal(gx.rn16(y64, dtype).double(), o["normed"]), "the fp64 normed row does not round to the integer row"
    assert torch.equal(o["hidden"].to(dtype).double(), o["hidden"])
    if total < 9:           # the shares of a single row of 2 dim elements are not statistics: conditions 1 and 2 only
        return gx.check_conditions(("stream_in", widths, total), dtype, o["ref"], o["absum"], o["q"], rounded=False)
    return gx.check_conditions(("stream_in", widths, gx.DT_ID[dtype], total), dtype, o["ref"], o["absum"], o["q"])


def check_in_exact(lib, device, widths, dtype, total):
    o = in_exact_operands(widths, dtype, total)
    xz, res_out = aum_hip.stream_in(o["hidden"].to(dtype).to(device), o["w_norm"].float().to(device), o["w_in"].to(dtype).to(device),
                                    residual=o["res"].float().to(device), eps=EPS, lib=lib)
    _sync(device)
    gx.assert_bits(("stream_in exact residual", widths, total), res_out, o["v"].float())
    gx.assert_bits(("stream_in exact", widths, gx.DT_ID[dtype], total), xz, gx.rn16(o["ref"], dtype))


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
def check_out_interval(lib, device, widths, dtype, total):
    o = out_operands(widths, dtype, total, False)
    out = aum_hip.stream_out(o["a"].to(dtype).to(device), o["b"].to(dtype).to(device), lib=lib)
    _sync(device)
    gx.assert_interval(("stream_out interval", widths, gx.DT_ID[dtype], total), out, o["ref"], widths[1] * 2.0 ** -23 * o["absum"], "stream_out")


def check_in_interval(lib, device, widths, dtype, total):
    dm, dim = widths
    hidden, res, w_norm = norm_operands(widths, dtype, total, device, True, seed=3)
    g = gx._gen("stack in interval", widths, gx.DT_ID[dtype], total)
    w_in = (torch.randn(2 * dim, dm, generator=g) / dm ** 0.5).to(dtype)
    xz, _ = aum_hip.stream_in(hidden, w_norm, w_in.to(device), residual=res, eps=EPS, lib=lib)
    a, _, _ = aum_hip.rmsnorm_fwd(hidden, w_norm, residual=res, eps=EPS, residual_dtype=torch.float32, lib=lib)     # the bit-pinned row of check 1
    _sync(device)
    a, b = a.cpu().double(), w_in.double()
    gx.assert_interval(("stream_in interval", widths, gx.DT_ID[dtype], total), xz, a @ b.t(), dm * 2.0 ** -23 * (a.abs() @ b.abs().t()), "stream_in")


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
def check_partition(lib, device, widths, dtype):
    dm, dim = widths
    total = 33
    hidden, res, w_norm = norm_operands(widths, dtype, total, device, True, seed=4)
    g = gx._gen("stack partition", widths, gx.DT_ID[dtype])
    w_in = (torch.randn(2 * dim, dm, generator=g) / dm ** 0.5).to(dtype).to(device)
    w_out = (torch.randn(dm, dim, generator=g) / dim ** 0.5).to(dtype).to(device)
    y = torch.randn(total, dim, generator=g).to(dtype).to(device)
    xz, ro = aum_hip.stream_in(hidden, w_norm, w_in, residual=res, eps=EPS, lib=lib)
    out = aum_hip.stream_out(y, w_out, lib=lib)
    at = 0
    for n in (1, 7, 8, 16, 1):
        sl = slice(at, at + n)
        xz_p, ro_p = aum_hip.stream_in(hidden[sl], w_norm, w_in, residual=res[sl], eps=EPS, lib=lib)
        out_p = aum_hip.stream_out(y[sl], w_out, lib=lib)
        _sync(device)
        gx.assert_bits(("partition xz", widths, at, n), xz_p, xz[sl])
        gx.assert_bits(("partition residual", widths, at, n), ro_p, ro[sl])
        gx.assert_bits(("partition out", widths, at, n), out_p, out[sl])
        at += n
    assert at == total
    perm = torch.randperm(total, generator=g).to(device)
    xz_r, ro_r = aum_hip.stream_in(hidden[perm].contiguous(), w_norm, w_in, residual=res[perm].contiguous(), eps=EPS, lib=lib)
    out_r = aum_hip.stream_out(y[perm].contiguous(), w_out, lib=lib)
    _sync(device)
    gx.assert_bits(("reordered xz", widths), xz_r, xz[perm])
    gx.assert_bits(("reordered residual", widths), ro_r, ro[perm])
    gx.assert_bits(("reordered out", widths), out_r, out[perm])


# ---- 5, 6 ----------------------------------------------------------------------------------------------------------------------------------
MAPS = {"one": ((None,), None, 1), "ragged": ((3, 0, 17), (2, 0, 3), 4), "eight": ((9,) * 8, tuple(range(8)), 8)}     # lens, rows, pool rows


def chain_operands(widths, dtype, total, nrows, device, depth=3):
    dm, dim = widths
    ncols, rank = XDT[dim]
    g = gx._gen("stack chain", widths, gx.DT_ID[dtype], total, nrows)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    layers = []
    for _ in range(depth):
        layers.append({
            "norm_weight": (1 + 0.1 * r(dm)).to(device), "w_in": r(2 * dim, dm, scale=dm ** -0.5).to(dtype).to(device),
            "conv_weight": r(dim, 4, scale=0.5).to(device), "conv_bias": r(dim, scale=0.1).to(device),
            "wx": r(ncols, dim, scale=dim ** -0.5).to(dtype).to(device), "wdt": r(dim, rank, scale=rank ** -0.5).to(dtype).to(device),
            "A": (-torch.exp(r(dim, 16, scale=0.5))).to(device), "D": r(dim).to(device), "delta_bias": (r(dim, scale=0.5) - 2.0).to(device),
            "w_out": r(dm, dim, scale=dim ** -0.5).to(dtype).to(device),
            "conv_state": r(nrows, dim, 4).to(device), "state": r(nrows, dim, 16, scale=0.3).to(device)})
    hidden = r(total, dm).to(dtype).to(device)
    return layers, hidden, dict(dim=dim, rank=rank, ncols=ncols, ldwx=dim, ldwdt=rank, eps=EPS)


def poison_unnamed(layers, rows):
    for L in layers:
        for r in range(L["conv_state"].shape[0]):
            if r not in rows:
                L["conv_state"][r] = POISON
                L["state"][r] = POISON


def python_loop(layers, hidden, smap, kw, lib, commit=True, peek=False):
    """the composition the C loop must equal: stream_in -> stream_block -> stream_out per layer"""
    residual = None
    for L in layers:
        xz, residual = aum_hip.stream_in(hidden, L["norm_weight"], L["w_in"], residual=residual, eps=kw["eps"], lib=lib)
        plan = sb.Plan(L["conv_weight"], L["conv_bias"], L["A"], L["D"], L["delta_bias"], L["wx"], L["wdt"], hidden.dtype)
        y = aum_hip.stream_block(xz[:, :kw["dim"]], xz[:, kw["dim"]:], L["conv_state"], L["state"], plan, seq_map=smap, commit=commit, peek=peek, lib=lib)
        hidden = aum_hip.stream_out(y, L["w_out"], lib=lib)
    return hidden, residual


def clone_layers(layers):
    return [{k: (v.clone() if k in ("conv_state", "state") else v) for k, v in L.items()} for L in layers]


def check_chain(lib, device, widths, dtype, map_name, mode):
    lens, rows, nrows = MAPS[map_name]
    if lens == (None,):
        lens = (17,)
    total = sum(lens)
    layers, hidden, kw = chain_operands(widths, dtype, total, nrows, device)
    named = set(range(len(lens)) if rows is None else [r for r, n in zip(rows, lens) if n > 0])
    poison_unnamed(layers, named)
    twin = clone_layers(layers)
    before = clone_layers(layers)
    smap = aum_hip.seq_map(lens, rows, device=device)
    commit, peek = mode != "no_commit", mode == "peek"
    h_ref, r_ref = python_loop(twin, hidden, smap, kw, lib, commit=commit, peek=peek)
    table = aum_hip.stream_layers_table(layers)
    h, r = aum_hip.stream_layers(hidden, table, len(layers), layers[0]["conv_state"], smap, commit=commit, peek=peek, lib=lib, **kw)
    _sync(device)
    gx.assert_bits(("chain hidden", widths, map_name, mode), h, h_ref)
    gx.assert_bits(("chain residual", widths, map_name, mode), r, r_ref)
    for l, (L, T, B) in enumerate(zip(layers, twin, before)):
        for k in ("conv_state", "state"):
            gx.assert_bits(("chain pool", k, l, widths, map_name, mode), L[k], T[k])
            if not commit:
                gx.assert_bits(("NO_COMMIT pool", k, l), L[k], B[k])
            for row in range(nrows):
                if row not in named:
                    assert bool((L[k][row] == POISON).all()), ("poison", k, l, row)
    if commit and not (peek and max(lens) == 1):
        assert any(not torch.equal(L["state"], B["state"]) for L, B in zip(layers, before))


def call_layers(a, lib, t):
    return lib.c.aum_stream_layers(aum_hip.C_byref(a), lib.stream(t))


def check_refusals(lib, device):
    widths, dtype, lens, rows, nrows = WIDTHS[0], BF16, (3, 0, 6), (2, 0, 3), 4
    total = sum(lens)
    ptr = aum_hip._ptr

    def fresh():
        layers, hidden, kw = chain_operands(widths, dtype, total, nrows, device)
        smap = aum_hip.seq_map(lens, rows, device=device)
        ws = torch.full((aum_hip.stream_layers_scratch_layout(total, widths[0], kw["dim"], kw["ncols"])[2] + 16,), 0x5A, dtype=torch.uint8, device=device)
        h_out = torch.full((total, widths[0]), 3.0, dtype=dtype, device=device)
        r_out = torch.full((total, widths[0]), 3.0, device=device)
        res_in = torch.randn(total, widths[0]).to(device)
        table = aum_hip.stream_layers_table(layers)
        a = aum_hip.stream_layers_args(hidden, table, len(layers), layers[0]["conv_state"], smap, ws[:-16], h_out, r_out, residual=res_in, **kw)
        return dict(layers=layers, table=table, a=a, ws=ws, h_out=h_out, r_out=r_out, keep=(hidden, smap, res_in))

    def refused(c, code):
        snap = [t.clone() for L in c["layers"] for t in (L["conv_state"], L["state"])] + [c["ws"].clone()]
        assert not aum_hip.stream_layers_supported(c["a"], c["table"])
        assert call_layers(c["a"], lib, c["h_out"]) == code, code
        _sync(device)
        now = [t for L in c["layers"] for t in (L["conv_state"], L["state"])] + [c["ws"]]
        assert all(torch.equal(x, y) for x, y in zip(now, snap)), "a refused call wrote a pool or the workspace"
        assert bool((c["h_out"] == 3.0).all()) and bool((c["r_out"] == 3.0).all()), "a refused call wrote an output"

    c = fresh()
    assert aum_hip.stream_layers_supported(c["a"], c["table"])
    c["table"][2].w_out = None                                         # the LAST layer's record: a NULL pointer
    refused(c, -1)
    c = fresh()
    c["a"].dtype = aum_hip.AUM_F32                                     # a wrong dtype
    refused(c, -3)
    c = fresh()
    c["table"][2].state = ptr(c["layers"][2]["state"]) + 4             # the LAST layer's pool pointer, misaligned
    refused(c, -4)
    c = fresh()
    c["a"].workspace_bytes = c["a"].workspace_bytes - 1                # one byte short
    refused(c, -5)
    c = fresh()
    c["a"].residual_in = c["a"].residual_out                           # read by all workgroups while one writes
    refused(c, -4)
    c = fresh()
    c["a"].max_len = aum_hip.STREAM_BLOCK_MAX_T + 1
    refused(c, -4)
    c = fresh()                                                        # and the unaltered call is taken
    assert call_layers(c["a"], lib, c["h_out"]) == 0
    _sync(device)
    assert not bool((c["h_out"] == 3.0).all())
    # the two kernels on their own
    hidden, res, w_norm = norm_operands(widths, dtype, 5, device, True)
    w_in = torch.zeros(2 * widths[1], widths[0], dtype=dtype, device=device)
    for bad in (lambda: aum_hip.stream_in(hidden.float(), w_norm, w_in.float(), lib=lib), lambda: aum_hip.stream_in(hidden[:, :128], w_norm[:128], w_in[:, :128], lib=lib),
                lambda: aum_hip.stream_out(hidden, w_in[:widths[0] * 2, :], lib=lib)):
        with pytest.raises(RuntimeError):
            bad()


# ---- 7, 8, 9: the model --------------------------------------------------------------------------------------------------------------------
def make_model(device, embed_dim=384, depth=4, dtype=BF16, **over):
    return sc.make_causal_aum(embed_dim, device, depth=depth, **over).to(dtype)


def _pools(cache):
    return [t for i in sorted(cache["layers"]) for t in cache["layers"][i]]


def check_model_arms(lib, device, embed_dim=384):
    """a staggered, ragged stream_push_many sequence with read=True through both arms; figures printed for the profile"""
    names = ("aum_stream_layers", "aum_stream_block_tm", "aum_rmsnorm_fwd")
    with torch.no_grad(), product_lib(lib), count_entries(lib, names) as calls:
        errs, finals = {}, {}
        for arm in ("default", "stack"):
            before, passes = dict(calls), 0
            model = make_model(device, embed_dim)
            nt = model.patch_grid_size[1]
            torch.manual_seed(2)
            spec = torch.randn(3, nt * 16, 128).to(device).to(BF16)
            stack = model.stream_stack() if arm == "stack" else None
            pool = model.allocate_stream_pool(4)
            rows = [3, 0, 2]
            plan = [((1, 2, 1), (0, 1, 2)), ((3, 1), (0, 2)), ((4, 5, 6), (0, 1, 2)), ((8, 8, 8), (0, 1, 2)), ((1,), (2,))]
            done = [0, 0, 0]
            logits = {}
            for ks, who in plan:
                ks = [min(k, nt - done[w]) for k, w in zip(ks, who)]
                go = [(k, w) for k, w in zip(ks, who) if k > 0]
                if not go:
                    continue
                pieces = [spec[w, done[w] * 16:(done[w] + k) * 16] for k, w in go]
                _, out = model.stream_push_many(pieces, pool, [rows[w] for _, w in go], read=True, stack=stack)
                passes += 1
                for (k, w), o in zip(go, out):
                    done[w] += k
                    logits[w] = o
            while min(done) < nt:
                go = [(min(8, nt - done[w]), w) for w in range(3) if done[w] < nt]
                _, out = model.stream_push_many([spec[w, done[w] * 16:(done[w] + k) * 16] for k, w in go], pool, [rows[w] for _, w in go], read=True,
                                                stack=stack)
                passes += 1
                for (k, w), o in zip(go, out):
                    done[w] += k
                    logits[w] = o
            snap = [t.clone() for t in _pools(pool)]
            final = model.stream_read(pool, sessions=rows, stack=stack)
            assert all(torch.equal(a, b) for a, b in zip(_pools(pool), snap)), "stream_read wrote a cache"
            # the arm took the path it is named after: every push and the read one aum_stream_layers call and no block launch from Python,
            # or none of the former (a silent fallback would compare the default arm with itself)
            took = {k: calls[k] - before[k] for k in names}
            if arm == "stack":
                # (aum_rmsnorm_fwd: the head's final norm once per pass on the device, none from the blocks)
                assert took["aum_stream_layers"] == passes + 1 and took["aum_stream_block_tm"] == 0 and passes >= 5, (took, passes)
                assert took["aum_rmsnorm_fwd"] in (0, passes + 1), (took, passes)
            else:
                assert took["aum_stream_layers"] == 0 and (device == "cpu" or took["aum_stream_block_tm"] == 4 * (passes + 1)), (took, passes)
            ref = model(spec).float().cpu().numpy()
            e_push = rel_err(torch.stack([logits[w] for w in range(3)]).float().cpu().numpy(), ref)
            e_read = rel_err(final.float().cpu().numpy(), ref)
            errs[arm] = max(e_push, e_read)
            print(f"stream stack model arms, d_model {embed_dim}, {arm}: last push logits {e_push:.3e}, final read {e_read:.3e} vs model(spec) (bar 2e-2)")
            assert e_push < 2e-2 and e_read < 2e-2, (arm, e_push, e_read)
        print(f"stream stack model arms, d_model {embed_dim}: stack {errs['stack']:.3e} vs default {errs['default']:.3e} (allowed: twice)")
        assert errs["stack"] <= 2 * errs["default"], errs
        return errs


def check_hop_cut(lib, device):
    """the stack arm pushed as one hop of 4 columns and as 4 hops of 1 column: the same caches and logits, bit for bit"""
    with torch.no_grad(), product_lib(lib):
        model = make_model(device)
        stack = model.stream_stack()
        torch.manual_seed(4)
        spec = torch.randn(2, 64, 128).to(device).to(BF16)
        a, b = model.allocate_inference_cache(2), model.allocate_inference_cache(2)
        _, la = model.stream_push(spec, a, read=True, stack=stack)
        for c in range(4):
            _, lb = model.stream_push(spec[:, c * 16:(c + 1) * 16], b, read=True, stack=stack)
        assert all(torch.equal(x, y) for x, y in zip(_pools(a), _pools(b))) and torch.equal(la, lb)
        snap = [t.clone() for t in _pools(a)]
        r = model.stream_read(a, stack=stack)
        assert all(torch.equal(x, y) for x, y in zip(_pools(a), snap)) and torch.equal(r, la)


@contextlib.contextmanager
def count_entries(lib, names):
    n = {k: 0 for k in names}
    real = {k: getattr(lib.c, k) for k in names}

    def wrap(k):
        def f(*a):
            n[k] += 1
            return real[k](*a)
        return f
    for k in names:
        setattr(lib.c, k, wrap(k))
    try:
        yield n
    finally:
        for k in names:
            setattr(lib.c, k, real[k])


def check_one_call(lib, device):
    names = ("aum_stream_layers", "aum_rmsnorm_fwd", "aum_stream_block_tm", "aum_stream_in_tm", "aum_stream_out_tm")
    with torch.no_grad(), product_lib(lib):
        model = make_model(device)
        stack = model.stream_stack()
        torch.manual_seed(5)
        spec = torch.randn(1, 32, 128).to(device).to(BF16)
        cache = model.allocate_inference_cache(1)
        model.stream_push(spec[:, :16], cache, stack=stack)              # builds what is built once
        with count_entries(lib, names) as n:
            model.stream_push(spec[:, 16:], cache, stack=stack)
        assert n == {"aum_stream_layers": 1, "aum_rmsnorm_fwd": 0, "aum_stream_block_tm": 0, "aum_stream_in_tm": 0, "aum_stream_out_tm": 0}, n
        assert stack.takes(8, 8) and stack.takes(288, 9) and not stack.takes(8, 129) and not stack.takes(stack.MAX_TOTAL + 1, 8)
        cache2 = model.allocate_inference_cache(1)
        model.stream_push(spec[:, :16], cache2)
        with count_entries(lib, names) as n:
            model.stream_push(spec[:, 16:], cache2)
        assert n["aum_stream_layers"] == 0 and n["aum_stream_in_tm"] == 0 and n["aum_stream_out_tm"] == 0, n
        if device != "cpu":                                              # today's counts: one norm and one block launch per layer
            assert n["aum_rmsnorm_fwd"] == 4 and n["aum_stream_block_tm"] == 4, n


def check_stack_cache(lib, device):
    with torch.no_grad(), product_lib(lib):
        model = make_model(device)
        stack = model.stream_stack()
        assert model.stream_stack() is stack
        torch.manual_seed(6)
        spec = torch.randn(1, 16, 128).to(device).to(BF16)

        def logits(st):
            return model.stream_push(spec, model.allocate_inference_cache(1), read=True, stack=st)[1]
        l0 = logits(stack)
        model.layers[1].mixer.in_proj.weight.mul_(0.5)
        s1 = model.stream_stack()
        assert s1 is not stack
        l1 = logits(stack)                                               # the stale handle: the push rebuilds
        assert not torch.equal(l0, l1) and torch.equal(l1, logits(s1))
        ref = logits(None)
        assert rel_err(l1.float().cpu().numpy(), ref.float().cpu().numpy()) < 2e-2
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        sd["layers.1.mixer.in_proj.weight"] = sd["layers.1.mixer.in_proj.weight"] * 2.0
        model.load_state_dict(sd)
        s2 = model.stream_stack()
        assert s2 is not s1
        assert torch.equal(logits(s2), l0)                               # 0.5 * 2: the first values again, exactly (powers of two)
        # a write through .data moves no _version: Mamba.invalidate_stream_params() is the remedy, and it reaches the stack too
        model.layers[2].mixer.D.data.mul_(3.0)
        assert model.stream_stack() is s2 and torch.equal(logits(s2), l0)          # stale, as documented
        model.layers[2].mixer.invalidate_stream_params()
        s3 = model.stream_stack()
        l3 = logits(s2)                                                      # the stale handle: rebuilt
        assert s3 is not s2 and model.stream_stack() is s3 and not torch.equal(l3, l0)
        assert rel_err(l3.float().cpu().numpy(), logits(None).float().cpu().numpy()) < 2e-2
    with pytest.raises(ValueError, match="bias"):
        make_model(device, depth=2, ssm_cfg={"bias": True}).stream_stack()
    with pytest.raises(ValueError, match="bimamba_type"):
        sc.make_causal_aum(384, device, depth=2, bimamba_type="v1").to(BF16).stream_stack()
    with pytest.raises(ValueError, match="bf16 or fp16"):
        sc.make_causal_aum(384, device, depth=2).stream_stack()
