"""Checks of TIMELINE TRAINING -- aum_scan_tm_peeks_fwd_ckpt / aum_scan_tm_peeks_bwd / aum_conv1d_tm_peeks_bwd, their bindings, the autograd
functions selective_scan_peeks_fn / causal_conv1d_peeks_fn, Mamba.forward(peek_every=) and AudioMamba.forward_timeline -- shared by
tests/test_timeline_train.py (CPU, lane-array library) and tests/test_gpu_timeline_train.py (device library).

Shapes are those of stream_timeline_checks (DIMS, PERIODS, pack_lengths(P) in a shuffled pack, the operand variants of ScanOp / ConvOp).
The oracle is the pure-torch twin (selective_scan_peeks_ref / causal_conv1d_peeks_ref) run in float64 on the same rounded inputs with a
random dout.  Bars: per-token gradients OUT_BAR of stream_checks (1e-4 fp32, 1e-2 for 16-bit I/O: one rounding of the stored gradient);
parameter sums 1e-4 for every dtype through conftest.rel_err_by (they are accumulated and stored in fp32 from the same rounded inputs, so
the 16-bit cases get no wider bar); module and model 1e-4 in fp32 and 2e-2 under bf16 autocast (the project's model bars)."""
import contextlib

import numpy as np
import pytest
import torch

import aum_hip
from causal_conv1d import causal_conv1d_peeks_fn, causal_conv1d_peeks_ref
from conftest import rel_err, rel_err_by
from mamba_ssm.ops import selective_scan_interface as ssi
from stream_checks import DT, OUT_BAR, make_causal_aum
from stream_timeline_checks import DIMS, PERIODS, SENTINEL, ConvOp, ScanOp, _is_peek, _np, _sync, pack_lengths

PARAM_BAR = 1e-4


def layout(P):
    """the lengths of pack_lengths(P) in a shuffled order"""
    rng = np.random.default_rng(17 + P)
    return [pack_lengths(P)[i] for i in rng.permutation(len(pack_lengths(P)))]


def _dout(o_like, seed, device):
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randn(o_like.shape, generator=g).to(o_like.dtype).to(device)


# ---- the two operators behind one interface: fwd, bwd (named gradients), the float64 oracle -------------------------------------------------
class Scan:
    name, op = "scan", ScanOp
    TOKEN, PARAM = ("du", "ddelta", "dz", "dB", "dC"), ("dA", "dD", "ddelta_bias")

    @staticmethod
    def operands(dt, dim, total, device, kind, seed, inputs=None):
        """inputs: a dict with the keys of cases.scan_inputs, batch 1 and `total` steps, to pack instead of the seeded values (and
        "softplus" / "activated": the form delta is in; scan_domain_checks.py)"""
        if inputs is None:
            return ScanOp.operands(dt, dim, total, 1, (), device, kind=kind, seed=seed)
        tm = lambda k, t=None: None if inputs[k] is None else torch.tensor(np.ascontiguousarray(inputs[k][0].T)).to(t or DT[dt]).to(device)
        par = lambda k: None if inputs[k] is None else torch.tensor(inputs[k], dtype=torch.float32).to(device)
        assert inputs["u"].shape == (1, dim, total)
        xz = torch.cat((tm("u"), tm("z") if inputs["z"] is not None else tm("u")), dim=1)      # u, z as the halves of one xz row
        bcm = torch.cat((tm("B"), tm("C")), dim=1)
        return {"dt": dt, "dim": dim, "u": xz[:, :dim], "z": xz[:, dim:] if inputs["z"] is not None else None, "delta": tm("delta"),
                "B": bcm[:, :16], "C": bcm[:, 16:], "A": par("A"), "D": par("D"), "bias": par("delta_bias"),
                "sp": bool(inputs.get("softplus", True)), "act": bool(inputs.get("activated", False)), "pool": None}

    @staticmethod
    def rows(o):
        return o["u"]

    @staticmethod
    def take(o, idx):
        t = lambda a: None if a is None else a.index_select(0, idx)
        return dict(o, u=t(o["u"]), z=t(o["z"]), delta=t(o["delta"]), B=t(o["B"]), C=t(o["C"]))

    @staticmethod
    def fwd(o, smap, P, lib):
        return aum_hip.scan_tm_peeks_fwd(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"], o["act"], smap, P, lib)

    @staticmethod
    def infer(o, smap, P, lib):
        pool = torch.zeros(len(smap.lens), o["dim"], 16, device=o["u"].device)
        return aum_hip.scan_tm_chunk_peeks(pool, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"], o["act"],
                                           seq_map=smap, lib=lib, peek_every=P)

    @staticmethod
    def bwd(o, dout, smap, P, lib):
        _, ck = Scan.fwd(o, smap, P, lib)
        du, dd, dz, dA, dB, dC, dD, db = aum_hip.scan_tm_peeks_bwd(dout, ck, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"],
                                                                   o["sp"], o["act"], smap, P, lib)
        return {"du": du, "ddelta": dd, "dz": dz, "dB": dB, "dC": dC, "dA": dA, "dD": dD, "ddelta_bias": db if (o["bias"] is not None or o["act"]) else None}

    @staticmethod
    def parts(o, dout, smap, P, lib, fill):
        _, ck = Scan.fwd(o, smap, P, lib)
        du, dd, dz, parts = aum_hip.scan_tm_peeks_bwd_parts(dout, ck, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"],
                                                            o["act"], smap, P, lib, fill=fill)
        return [du, dd] + ([] if dz is None else [dz]), parts[0].transpose(0, 1), list(parts[1:])

    @staticmethod
    def oracle(o, dout, lens, P):
        f = lambda t: None if t is None else t.detach().double().cpu().requires_grad_(True)
        u, dl, A, B, C, D, z, bias = f(o["u"]), f(o["delta"]), f(o["A"]), f(o["B"]), f(o["C"]), f(o["D"]), f(o["z"]), f(o["bias"])
        smap = aum_hip.seq_map(lens, device="cpu")
        out = ssi.selective_scan_peeks_ref(u, dl, A, B, C, D, z, bias, o["sp"], P, smap)      # an activated delta is a plain delta here
        out.backward(dout.double().cpu())
        ddelta = dl.grad
        if o["act"]:                        # the kernel returns raw space: times the softplus derivative 1 - exp(-dl)
            ddelta = ddelta * (1.0 - torch.exp(-dl.detach()))
        g = {"du": u.grad, "ddelta": ddelta, "dz": None if z is None else z.grad, "dB": B.grad, "dC": C.grad, "dA": A.grad,
             "dD": None if D is None else D.grad, "ddelta_bias": bias.grad if bias is not None else (ddelta.sum(0) if o["act"] else None)}
        return out.detach(), g


class Conv:
    name, op = "conv", ConvOp
    TOKEN, PARAM = ("dx",), ("dw", "db")

    @staticmethod
    def operands(dt, dim, total, device, kind, seed):
        return ConvOp.operands(dt, dim, total, 1, (), device, kind=kind, seed=seed)

    @staticmethod
    def rows(o):
        return o["x"]

    @staticmethod
    def take(o, idx):
        return dict(o, x=o["x"].index_select(0, idx))

    @staticmethod
    def fwd(o, smap, P, lib):
        return aum_hip.conv1d_tm_peeks_fwd(o["x"], o["w"], o["b"], o["silu"], smap, P, lib), None

    infer = None

    @staticmethod
    def bwd(o, dout, smap, P, lib):
        dx, dw, db = aum_hip.conv1d_tm_peeks_bwd(dout, o["x"], o["w"], o["b"], o["silu"], smap, P, lib)
        return {"dx": dx, "dw": dw, "db": db}

    @staticmethod
    def parts(o, dout, smap, P, lib, fill):
        dx, parts = aum_hip.conv1d_tm_peeks_bwd_parts(dout, o["x"], o["w"], o["b"], o["silu"], smap, P, lib, fill=fill)
        return [dx], None, list(parts) if o["b"] is not None else [parts[0]]

    @staticmethod
    def oracle(o, dout, lens, P):
        f = lambda t: None if t is None else t.detach().double().cpu().requires_grad_(True)
        x, w, b = f(o["x"]), f(o["w"]), f(o["b"])
        out = causal_conv1d_peeks_ref(x, w, b, "silu" if o["silu"] else None, P, aum_hip.seq_map(lens, device="cpu"))
        out.backward(dout.double().cpu())
        return out.detach(), {"dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}


OPS = {"scan": Scan, "conv": Conv}


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. forward identity -----------------------------------------------------------------------------------------------------------------
def check_forward_identity(dt, dim, P, lib, device, kind=0):
    lens = layout(P)
    o = Scan.operands(dt, dim, sum(lens), device, kind, P)
    smap = aum_hip.seq_map(lens, device=device)
    out, ck = Scan.fwd(o, smap, P, lib)
    ref = Scan.infer(o, smap, P, lib)
    _sync(device)
    assert out.dtype == DT[dt] and torch.equal(out, ref), f"scan_tm_peeks_fwd {dt} dim {dim} P {P}: out differs from scan_tm_chunk_peeks on a zeroed pool"
    assert ck.numel() == (sum(lens) // 8 + len(lens)) * dim * 16


# ---- 2. gradients against float64 ----------------------------------------------------------------------------------------------------------
def check_gradients(opname, dt, dim, P, lib, device, kind=0):
    op = OPS[opname]
    lens = layout(P)
    o = op.operands(dt, dim, sum(lens), device, kind, P)
    dout = _dout(op.rows(o), P, device)
    got = op.bwd(o, dout, aum_hip.seq_map(lens, device=device), P, lib)
    _sync(device)
    out_ref, want = op.oracle(o, dout, lens, P)
    e_out = rel_err(_np(op.fwd(o, aum_hip.seq_map(lens, device=device), P, lib)[0]), out_ref.numpy())
    print(f"{opname} peeks training {dt} dim {dim} P {P} kind {kind}: forward {e_out:.3e} (bar {OUT_BAR[dt]:.0e})")
    assert e_out < OUT_BAR[dt]
    for k in op.TOKEN + op.PARAM:
        if want[k] is None:
            assert got[k] is None, k
            continue
        a, b = _np(got[k]).astype(np.float64), want[k].numpy()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k in op.TOKEN:
            assert got[k].dtype == (torch.float32 if k in ("dB", "dC") else DT[dt]), k
            e, bar = rel_err(a, b), OUT_BAR[dt]
        else:
            assert got[k].dtype == torch.float32, k
            e, bar = (rel_err_by(a, b, 1) if a.ndim == 2 else rel_err(a, b)), PARAM_BAR
        print(f"    {k}: {e:.3e} (bar {bar:.0e})")
        assert e < bar, (opname, dt, dim, P, k, e)


# ---- 3. peek rows do not leak ----------------------------------------------------------------------------------------------------------------
def check_peek_rows_do_not_leak(opname, dt, dim, P, lib, device, kind=0):
    op = OPS[opname]
    lens = layout(P)
    total = sum(lens)
    o = op.operands(dt, dim, total, device, kind, 50 + P)
    starts = np.cumsum([0] + lens[:-1])
    peek = torch.tensor([_is_peek(j, P) for n in lens for j in range(n)], device=device)
    keep = torch.nonzero(~peek).flatten()
    dout = _dout(op.rows(o), 60 + P, device)
    # dout zero on the peek rows = the sequences without their peek rows (no row of which is a peek row at a period past every length)
    d0 = dout.clone()
    d0[peek] = 0
    g = op.bwd(o, d0, aum_hip.seq_map(lens, device=device), P, lib)
    big = max(lens) + 1
    g2 = op.bwd(op.take(o, keep), d0.index_select(0, keep), aum_hip.seq_map([n - n // (P + 1) for n in lens], device=device), big, lib)
    _sync(device)
    for k in op.TOKEN:
        if g[k] is None:
            continue
        assert torch.equal(g[k].index_select(0, keep), g2[k]), f"{opname} {k}: committed rows differ from the call without peek rows"
        assert not g[k][peek].any(), f"{opname} {k}: a peek row with dout = 0 has a gradient"
    for k in op.PARAM:
        assert (g[k] is None and g2[k] is None) or torch.equal(g[k], g2[k]), f"{opname} {k}: differs from the call without peek rows"
    # dout zero on the committed rows: the peek rows still reach the committed rows in front of them
    d1 = dout.clone()
    d1[~peek] = 0
    g = op.bwd(o, d1, aum_hip.seq_map(lens, device=device), P, lib)
    _sync(device)
    k = op.TOKEN[0]
    for n, at in zip(lens, starts):
        if n >= P + 1:              # the scan's peek row sees every committed row in front of it, the conv's the last three
            lo = max(0, P - 3) if opname == "conv" else 0
            assert bool(g[k][at + lo:at + P].any(dim=1).all()), f"{opname} {k}: no gradient on the committed rows in front of the first peek row"
        else:
            assert not g[k][at:at + n].any()


# ---- 4. repeatability and isolation ------------------------------------------------------------------------------------------------------------
def check_repeatable_and_isolated(opname, dt, dim, P, lib, device, kind=0):
    op = OPS[opname]
    lens = layout(P)
    total = sum(lens)
    o = op.operands(dt, dim, total + 5, device, kind, 70 + P)             # five rows behind the pack belong to no sequence
    dout = _dout(op.rows(o), 80 + P, device)
    smap = aum_hip.SeqMap(tuple(lens), tuple(range(len(lens))), total + 5, aum_hip.seq_map(lens, device=device).cu, None)
    rows1, bc1, parts1 = op.parts(o, dout, smap, P, lib, SENTINEL)
    rows2, bc2, parts2 = op.parts(o, dout, smap, P, lib, SENTINEL)
    _sync(device)
    assert _equal(rows1, rows2) and _equal(parts1, parts2) and (bc1 is None or torch.equal(bc1, bc2)), f"{opname}: two launches differ"
    for t in rows1 + ([] if bc1 is None else [bc1]):
        assert bool((t[total:] == SENTINEL).all()), f"{opname}: rows behind the pack were written"
        assert not bool((t[:total] == SENTINEL).all(dim=-1).any()), f"{opname}: a row of a sequence was not written"
    for i, n in enumerate(lens):
        for t in parts1:
            assert bool((t[i] == SENTINEL).all()) == (n == 0), f"{opname}: partial row of sequence {i} (length {n})"
    # every sequence alone, at the front of a pack of its own
    at = 0
    for i, n in enumerate(lens):
        if n:
            idx = torch.arange(at, at + n, device=device)
            r, bc, parts = op.parts(op.take(o, idx), dout.index_select(0, idx), aum_hip.seq_map([n], device=device), P, lib, SENTINEL)
            _sync(device)
            assert _equal([t[at:at + n] for t in rows1], r), f"{opname}: sequence {i} depends on its neighbours"
            assert bc is None or torch.equal(bc1[at:at + n], bc)
            assert _equal([t[i] for t in parts1], [t[0] for t in parts])
        at += n


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, device):
    lens, P, dim = (5, 3), 2, 128
    total = sum(lens)
    smap = aum_hip.seq_map(lens, device=device)
    o = Scan.operands("bf16", dim, total, device, 0, 5)
    out, ck = Scan.fwd(o, smap, P, lib)
    dout = _dout(o["u"], 6, device)
    new = lambda *shape, dt=torch.float32: torch.full(shape, SENTINEL, dtype=dt, device=device)
    held = []

    def base(a, out_t):
        _, h = aum_hip._scan_peeks_base(a, "test", lib, o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], o["sp"], o["act"], out_t, smap)
        held.append(h)

    def refused(fn, pa, bufs, cases):
        good = {k: getattr(pa, k) for k in ("peek_every",) + tuple(c[0] for c in cases)}
        flags = pa.base.flags if hasattr(pa, "base") else pa.flags
        for field, bad in cases + (("flags", None),):
            if field == "flags":
                for bit in (aum_hip.SCAN_PEEK_LAST, aum_hip.CONV_PEEK_LAST, 1 << 20):
                    if hasattr(pa, "base"):
                        pa.base.flags = flags | bit
                    else:
                        pa.flags = flags | bit
                    assert fn(aum_hip.C_byref(pa), lib.stream(out)) != 0, ("flags", bit)
                if hasattr(pa, "base"):
                    pa.base.flags = flags
                else:
                    pa.flags = flags
            else:
                setattr(pa, field, bad)
                assert fn(aum_hip.C_byref(pa), lib.stream(out)) != 0, (field, bad)
                setattr(pa, field, good[field])
            _sync(device)
            for b in bufs:
                assert bool((b == SENTINEL).all()), f"a refused call ({field}) wrote a buffer"
        assert fn(aum_hip.C_byref(pa), lib.stream(out)) == 0
        _sync(device)

    # forward: peek_every < 1, a PEEK_LAST bit, a short checkpoint buffer
    pa = aum_hip.ScanTmPeeksFwdArgs()
    y, ck2 = new(total, dim, dt=DT["bf16"]), new(ck.numel())
    base(pa.base, y)
    pa.ckpt, pa.ckpt_bytes, pa.peek_every = ck2.data_ptr(), ck2.numel() * 4, P
    refused(lib.c.aum_scan_tm_peeks_fwd_ckpt, pa, (y, ck2), (("peek_every", 0), ("peek_every", -3), ("ckpt_bytes", ck2.numel() * 4 - 4)))
    assert torch.equal(y, out)              # (slots no block of the pack reaches keep the sentinel; the backward below reads ck2)
    # backward: the same, and a short workspace
    pb = aum_hip.ScanTmPeeksBwdArgs()
    du, dd, dz = (new(total, dim, dt=DT["bf16"]) for _ in range(3))
    ws = new(int(lib.c.aum_scan_tm_peeks_bwd_workspace_bytes(total, len(lens), dim, 16)) // 4)
    base(pb.base, dout)
    pb.ckpt, pb.ckpt_bytes, pb.du, pb.ddelta, pb.dz, pb.workspace, pb.workspace_bytes = ck2.data_ptr(), ck2.numel() * 4, du.data_ptr(), dd.data_ptr(), dz.data_ptr(), ws.data_ptr(), ws.numel() * 4
    pb.du_ts = pb.ddelta_ts = pb.dz_ts = dim
    pb.peek_every = P
    refused(lib.c.aum_scan_tm_peeks_bwd, pb, (du, dd, dz, ws), (("peek_every", 0), ("ckpt_bytes", ck.numel() * 4 - 4), ("workspace_bytes", ws.numel() * 4 - 4),
                                                               ("du_ts", (1 << 31) // 8)))
    want = Scan.bwd(o, dout, smap, P, lib)
    assert torch.equal(du, want["du"]) and torch.equal(dd, want["ddelta"]) and torch.equal(dz, want["dz"])
    # conv backward
    c = Conv.operands("bf16", dim, total, device, 0, 7)
    pc = aum_hip.ConvTmPeeksBwdArgs()
    dx, wsc = new(total, dim, dt=DT["bf16"]), new(int(lib.c.aum_conv1d_tm_peeks_bwd_workspace_bytes(len(lens), dim, 4)) // 4)
    dy = _dout(c["x"], 8, device)
    w, b = c["w"].contiguous(), c["b"].contiguous()
    pc.x, pc.dy, pc.weight, pc.bias, pc.dx, pc.workspace, pc.cu_seqlens = c["x"].data_ptr(), dy.data_ptr(), w.data_ptr(), b.data_ptr(), dx.data_ptr(), wsc.data_ptr(), smap.cu.data_ptr()
    pc.workspace_bytes, pc.x_ts, pc.dy_ts, pc.dx_ts = wsc.numel() * 4, c["x"].stride(0), dim, dim
    pc.total, pc.nseq, pc.dim, pc.width, pc.dtype, pc.flags, pc.peek_every = total, len(lens), dim, 4, aum_hip.AUM_BF16, aum_hip.CONV_SILU, P
    refused(lib.c.aum_conv1d_tm_peeks_bwd, pc, (dx, wsc), (("peek_every", 0), ("workspace_bytes", wsc.numel() * 4 - 4), ("dx_ts", (1 << 31) // 8)))
    assert torch.equal(dx, Conv.bwd(c, dy, smap, P, lib)["dx"])
    for fn in (lambda: Scan.fwd(o, smap, 0, lib), lambda: Conv.bwd(c, dy, smap, None, lib)):
        with pytest.raises(ValueError, match="peek_every"):
            fn()


# ---- 6. module -----------------------------------------------------------------------------------------------------------------------------------
def _ctx(device, autocast_dtype):
    if autocast_dtype is None:
        return contextlib.nullcontext()
    return torch.autocast(device_type=torch.device(device).type, dtype=autocast_dtype)


def _grads(module, loss_of, inputs=()):
    for p in module.parameters():
        p.grad = None
    out = loss_of()
    out[1].backward()
    return out[0].detach(), {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}, [t.grad.detach().clone() for t in inputs]


def _compare(what, a, b, bar):
    e = rel_err(_np(a), _np(b))
    print(f"    {what}: {e:.3e} (bar {bar:.0e})")
    assert e < bar, (what, e)


def check_module(d_model, device, autocast_dtype=None, P=8, T=27):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(21)
    m = Mamba(d_model, bimamba_type="none", layer_idx=0).to(device)
    h = torch.randn(2, T, d_model, device=device, requires_grad=True)
    gout = torch.randn(2, T, d_model, device=device)
    bar = 1e-4 if autocast_dtype is None else 2e-2

    def run():
        h.grad = None
        with _ctx(device, autocast_dtype):
            out = m(h, peek_every=P)
        return out, (out.float() * gout).sum()

    out_k, gk, (hk,) = _grads(m, run, (h,))
    with ssi.peeks_on_ref():
        out_r, gr, (hr,) = _grads(m, run, (h,))
    _sync(device)
    print(f"Mamba({d_model}).forward(peek_every={P}) T {T} autocast {autocast_dtype}: kernels vs the _ref twins")
    _compare("out", out_k, out_r, bar)
    _compare("d hidden", hk, hr, bar)
    assert set(gk) == set(gr) == {n for n, _ in m.named_parameters()}
    for n in gk:
        _compare("d " + n, gk[n], gr[n], bar)
    for bt in ("v1", "v2"):
        with pytest.raises(NotImplementedError, match="causal"):
            Mamba(64, bimamba_type=bt, layer_idx=0).to(device)(h[..., :64].detach(), peek_every=P)
    with pytest.raises(ValueError, match="peek_every"):
        m(h, peek_every=0)


# ---- 7. model ------------------------------------------------------------------------------------------------------------------------------------
def check_model(embed_dim, device, autocast_dtype=None):
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(11)
    spec = torch.randn(2, 256, 128, device=device)
    bar = 1e-4 if autocast_dtype is None else 2e-2
    with torch.no_grad(), _ctx(device, autocast_dtype):
        _, want = model.stream_timeline(spec, model.allocate_inference_cache(2))
        full = model(spec)

    def run(s=spec):
        with _ctx(device, autocast_dtype):
            logits = model.forward_timeline(s)
        return logits, logits.float().square().mean()

    logits, gk, _ = _grads(model, run)
    with ssi.peeks_on_ref():
        logits_r, gr, _ = _grads(model, run)
    _sync(device)
    print(f"AudioMamba({embed_dim}).forward_timeline autocast {autocast_dtype}")
    assert logits.shape == (2, 16, 7)
    _compare("vs stream_timeline", logits, want, bar)
    _compare("last column vs model(spec)", logits[:, -1], full, bar)
    _compare("vs the _ref twins", logits, logits_r, bar)
    assert set(gk) == set(gr) == {n for n, _ in model.named_parameters()}
    for n in gk:
        _compare("d " + n, gk[n], gr[n], bar)
    with _ctx(device, autocast_dtype):
        part = model.forward_timeline(spec[:, :80])
        feats = model.forward_timeline(spec[:, :16], return_features=True)
    assert part.shape == (2, 5, 7) and feats.shape == (2, 1, embed_dim)
    _compare("5 columns vs the first 5 of 16", part, logits[:, :5], bar)
    for bad in (spec[:, :24], spec[:, :0], spec[:, :32, :64], spec[0, :32], torch.cat((spec, spec[:, :16]), dim=1)):
        with pytest.raises(ValueError, match="forward_timeline"):
            model.forward_timeline(bad)


def check_model_refuses_non_streamable(device):
    spec = torch.randn(1, 32, 128, device=device)
    for over in (dict(bimamba_type="v1"), dict(use_middle_cls_token=True, use_end_cls_token=False), dict(transpose_token_sequence=False),
                 dict(if_bidirectional=True)):
        with pytest.raises(ValueError, match="streaming"):
            make_causal_aum(64, device, depth=2, **over).forward_timeline(spec)


def check_model_frontend(device):
    """forward_timeline(wave, frontend=) is forward_timeline of the frontend's own log-mel frames, and forward(timeline=True) reaches it"""
    from aum.frontend import FbankTables, WaveInput
    model = make_causal_aum(64, device, depth=2)
    torch.manual_seed(14)
    wave = torch.randn(2, 16000 * 256 // 100 + 240, device=device) * 0.1
    wave = wave - wave.mean(dim=1, keepdim=True)
    fe = WaveInput(FbankTables(device), target_length=256)
    with torch.no_grad():
        spec = fe.spectrogram(wave)
        assert spec.shape == (2, 256, 128)
        a, b, c = model.forward_timeline(wave, frontend=fe), model.forward_timeline(spec), model(wave, frontend=fe, timeline=True)
    _sync(device)
    assert a.shape == (2, 16, 7) and torch.equal(a, b) and torch.equal(a, c)


# ---- 8. launcher -----------------------------------------------------------------------------------------------------------------------------------
def check_launcher(tmp_path, on_ref=False):
    """aum.train --timeline_loss True on the toy dataset of tools/make_toy_audioset.py: refused on a Fo-Bi model; on a causal model two
    steps on the same two clips (one per epoch, no augmentation) give finite losses, the second not above the first"""
    import os
    import subprocess
    import sys
    import aum.train as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = str(tmp_path / "toy")
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_toy_audioset.py"), data, "--clips", "2", "--val-clips", "2", "--seconds", "0.7",
                    "--classes", "4"], check=True)
    files = sorted(os.listdir(data))
    pick = lambda *keys: os.path.join(data, next(f for f in files if all(k in f for k in keys)))
    exp = str(tmp_path / "exp")
    common = ["--model", "aum", "--model_type", "tiny", "--depth", "1", "--n_class", "4", "--label-csv", pick(".csv"), "--data-train", pick("train", ".json"),
              "--data-val", pick("val", ".json"), "--audio_length", "64", "--num-workers", "0", "-b", "2", "--mixed_precision", "no", "--exp-dir", exp,
              "--n-epochs", "2", "--max-steps", "1", "--n-print-steps", "1000", "--freqm", "0", "--timem", "0", "--mixup", "0", "--lr", "1e-3",
              "--lrscheduler_start", "10", "--save_model", "False", "--timeline_loss", "True"]
    for bad in (["--aum_type", "Fo-Bi", "--use_middle_cls_token", "False", "--use_end_cls_token", "True", "--transpose_token_sequence", "True"],
                ["--aum_type", "Fo-Fo"], ["--aum_type", "Fo-Fo", "--use_middle_cls_token", "False", "--use_end_cls_token", "True"]):
        with pytest.raises(ValueError, match="timeline_loss"):
            T.main(common + bad)
    calls = []
    real = T._timeline_loss
    T._timeline_loss = lambda loss_fn, logits, labels: (calls.append(tuple(logits.shape)), real(loss_fn, logits, labels))[1]
    try:
        with (ssi.peeks_on_ref() if on_ref else contextlib.nullcontext()):
            T.main(common + ["--aum_type", "Fo-Fo", "--use_middle_cls_token", "False", "--use_end_cls_token", "True", "--transpose_token_sequence", "True"])
    finally:
        T._timeline_loss = real
    assert calls == [(2, 4, 4), (2, 4, 4)], calls                      # 64 frames = 4 time columns, 4 classes
    result = np.loadtxt(os.path.join(exp, "result.csv"), delimiter=",")
    l1, l2 = float(result[0, 5]), float(result[1, 5])
    print(f"--timeline_loss True, two steps on the same batch: train loss {l1:.6f} -> {l2:.6f}; valid loss {result[0, 6]:.6f} -> {result[1, 6]:.6f}")
    assert np.isfinite([l1, l2]).all() and np.isfinite(result[:, 6]).all() and l2 <= l1
    preds = np.loadtxt(os.path.join(exp, "predictions", "predictions_2.csv"), delimiter=",")
    assert preds.shape == (2, 4)                                            # the last column's output, one row per clip
