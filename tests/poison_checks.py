"""Poison checks of the token-major training kernels, shared by tests/test_poison.py (CPU, lane-array library) and tests/test_gpu_poison.py
(device library): what a kernel must not depend on and must not touch.

The rule is the same for every family.  Every operand of a case is a view into a larger buffer and the entry point runs twice on the same
values:

  NAN run   everything the kernel does not own is NaN: the pitch padding behind each row, the neighbouring column block of the same row
            (the z half next to x, the dt columns next to B | C, ...) and at least one tile of rows behind the last row (130 rows for
            the token-tiled kernels, 8 time steps for the scans).  The interior of every output is NaN, its surroundings (padding,
            neighbouring block, a tile of rows behind) hold the sentinel 7.0; every checkpoint, partial and scratch buffer the caller
            hands in is NaN with a sentinel tail.
  BIG run   the same layout with 3.0e4 (finite in fp16 and bf16) in the unowned input regions and -3.0e4 in the output interiors.

and then (1) every output interior of the NAN run is finite, (2) the NAN outputs are bit-equal to the BIG outputs (a NaN that a select
removes again and a finite neighbour that leaks through a max or a clamp both show here), (3) the NAN outputs meet the bar the family's
existing check holds against its existing fp64 reference (kernel_checks.py / xdt_tiny_checks.py: the same helpers, no tolerance of this
module's own), (4) every sentinel still equals 7.0, the message naming the region.  Bit-equality is between two runs of ONE layout, never
against a contiguous run: a pitch may select another vector path and so another order of the sums.

Operands the ABI gives a pitch get all three treatments; operands it takes contiguous only (weights, parameters, fp32 partial and
gradient tensors) are poisoned or guarded behind their last row only.  Each check's docstring lists which is which."""
import math

import numpy as np
import pytest
import torch

import aum_hip
import cases
import kernel_checks as KC
import xdt_tiny_checks as TC

NAN, BIG = "NAN", "BIG"
SENTINEL = KC.NORM_SENTINEL
FILL_IN = {NAN: float("nan"), BIG: 3.0e4}
FILL_OUT = {NAN: float("nan"), BIG: -3.0e4}
TOK_TILE = 130      # rows behind the last token of a token-tiled kernel: more than its largest tile (128 tokens)
SCAN_TILE = 8       # time steps behind the last step of a scan row: one block of the scans
W_ROWS = 8          # rows behind a weight matrix
PAD = 8             # pitch padding, elements: the smallest the kernels' 16-byte rows allow in every dtype

# The smallest shapes that still have the edges.
# conv (name, batch, dim, len, width, bias): a chunk seam (64 steps) + 1; more than 512 channels, one wave's worth in the 16-bit form; width 3
CONV_CASES = [c for c in cases.CONV_TM_CASES if c[0] in ("tm_l65", "tm_l70_w3")] + [("poison_l9_d520", 1, 520, 9, 4, True)]
# scans (case, segments): one step, one block + 1, the odd meeting point of a Fo-Bi pair, two batch entries x two channel groups with a ragged
# last block; the two longer ones also cut into 3 time ranges
_scan = {c[0]: c for c in cases.SCAN_TM_CASES}
SCAN_CASES = [(_scan[n], 1) for n in ("tm_l1", "tm_l9", "tm_l75", "tm_l130")] + [(_scan[n], 3) for n in ("tm_l75", "tm_l130")]
DTPROJ_CASES = [(33, 96, 24, 56), (31, 32, 16, 48), (129, 256, 48, 80), (70, 128, 64, 96)]       # (ntok, dim, rank, ncols)
XDT_CASES = [(1, 256, 8), (33, 256, 24, 56), (145, 768, 24, 56), (127, 512, 48)]                 # (ntok, dim, rank[, ncols = 80])
XDT_BWD_CASES = [(33, 256, 8), (145, 768, 16)]                                                   # (ntok, dim, pad)
GEMM_CASES = [(1, 256, 64), (257, 512, 192), (385, 512, 128), (130, 256, 448)]                   # (m, n, k); the last: the paced schedule's k
GEMM_WGRAD_CASES = [(65, 256, 256, 1), (64, 256, 48, 1, 0, 32), (513, 512, 48, 3, 8, 32), (130, 256, 80, 7)]   # (t, n, k, splits[, pad_y, pad_x])


class Frame:
    """one operand as the view buf[..., :rows, at:at + cols] of a (..., rows + behind, sum of the column blocks) buffer.  blocks: [(name,
    width)], `own` the index of the operand's block; the names of the others finish the sentence "wrote ..." in a guard's message"""

    def __init__(self, lead, rows, blocks, own, behind, dtype, dev, fill):
        self.rows, self.blocks, self.own = rows, blocks, own
        self.buf = torch.full(tuple(lead) + (rows + behind, sum(w for _, w in blocks)), fill, dtype=dtype, device=dev)
        at = sum(w for _, w in blocks[:own])
        self.view = self.buf[..., :rows, at:at + blocks[own][1]]

    @classmethod
    def inp(cls, lead, rows, blocks, own, behind, values, mode):
        """an input: `values` inside, the poison of `mode` everywhere else"""
        f = cls(lead, rows, blocks, own, behind, values.dtype, values.device, FILL_IN[mode])
        f.view.copy_(values)
        return f

    @classmethod
    def out(cls, lead, rows, blocks, own, behind, dtype, dev, mode):
        """an output: the interior pre-filled for `mode`, the sentinel everywhere else"""
        f = cls(lead, rows, blocks, own, behind, dtype, dev, SENTINEL)
        f.view.fill_(FILL_OUT[mode])
        return f

    def guards(self, what, last="token"):
        g, at = [], 0
        for i, (name, w) in enumerate(self.blocks):
            if i != self.own:
                g.append((f"{what}: wrote {name}", self.buf[..., :self.rows, at:at + w], SENTINEL))
            at += w
        g.append((f"{what}: wrote behind the last {last}", self.buf[..., self.rows:, :], SENTINEL))
        return g


class Flat:
    """an output or scratch tensor the ABI takes contiguous only: pre-filled for `mode`, `extra` sentinel elements behind its last row"""

    def __init__(self, shape, dev, mode, extra, dtype=torch.float32):
        n = math.prod(shape)
        self.buf = torch.full((n + extra,), SENTINEL, dtype=dtype, device=dev)
        self.buf[:n] = FILL_OUT[mode]
        self.view, self.tail = self.buf[:n].view(shape), self.buf[n:]

    def guards(self, what):
        return [(f"{what}: wrote behind its last row", self.tail, SENTINEL)]


def tail_in(values, mode, extra=64):
    """an input the ABI takes contiguous only (a weight, a parameter): its values with `extra` poison elements behind the last row"""
    if values is None:
        return None
    n = values.numel()
    buf = torch.full((n + extra,), FILL_IN[mode], dtype=values.dtype, device=values.device)
    buf[:n] = values.reshape(-1)
    return buf[:n].view(values.shape)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _holds(region, value):
    return bool(torch.isnan(region).all()) if value != value else bool((region == value).all())


def run_pair(tag, run, dev):
    """run(mode) -> ({name: output interior}, [(message, region, value it must still hold)]) for NAN and BIG: assertions 4, 1 and 2 of the
    module's rule.  Returns the NAN run's outputs for assertion 3."""
    got = {}
    for mode in (NAN, BIG):
        outs, guards = run(mode)
        if dev != "cpu":
            torch.cuda.synchronize()
        for msg, region, value in guards:
            assert _holds(region, value), tag + (mode, msg)
        got[mode] = outs
    assert set(got[NAN]) == set(got[BIG])
    for k, t in got[NAN].items():
        assert bool(torch.isfinite(t.float()).all()), tag + (k, "not finite: poison reached the result, or a part of it was never written")
    for k, t in got[NAN].items():
        assert torch.equal(_bits(t), _bits(got[BIG][k])), tag + (k, "differs between NaN and finite poison: it depends on memory it does not own")
    return got[NAN]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ok(rc, what):
    assert rc == 0, (what, "refused", aum_hip._ERR.get(rc, rc))


def _set3(a, name, view, prefix=None):
    """pointer and (batch, token) strides of a (batch, len, X) view"""
    prefix = prefix or name
    setattr(a, name, view.data_ptr())
    setattr(a, prefix + "_bs", view.stride(0))
    setattr(a, prefix + "_ts", view.stride(1))


# ---- token-major conv ---------------------------------------------------------------------------------------------------------------------
def check_conv_tm_poison(lib, dev, case, dtype, reverse, silu):
    """aum_conv1d_tm_fwd / _bwd.  All through the C entry points (the binding allocates y and the partial rows itself):
    x      the first half of (batch, len + 130, 2 dim + 8) rows -- z half, padding and rows behind poisoned (a layout the binding takes too)
    dy     pitch dim + 8 -- padding and rows behind poisoned
    y      pitch dim + 8, guarded: padding, rows behind
    dx     the first half of (batch, len + 130, 2 dim + 8) rows, guarded: z half, padding, rows behind
    dw_part / db_part   contiguous in the ABI: NaN pre-fill, one sentinel row behind aum_conv1d_tm_nparts(batch, len) rows
    dweight / dbias     the sums of the partial rows (aum_sum_rows into a caller's tensor): one sentinel row behind
    weight / bias       contiguous in the ABI: poison behind the last row only"""
    name, batch, dim, length, width, has_bias = case
    d, ry, rg = KC.conv_tm_reference(case, dtype, reverse, silu)
    tm = lambda a: KC.T(np.ascontiguousarray(a.transpose(0, 2, 1)), dev, dtype)
    xv, dyv, wv, bv = tm(d["x"]), tm(d["dout"]), KC.T(d["weight"], dev), KC.T(d["bias"], dev)
    nparts = int(lib.c.aum_conv1d_tm_nparts(batch, length))
    half = [("x", dim), ("into the z half", dim), ("past the row", PAD)]
    pitched = [("y", dim), ("past dim", PAD)]

    def run(mode):
        x = Frame.inp((batch,), length, half, 0, TOK_TILE, xv, mode)
        dy = Frame.inp((batch,), length, pitched, 0, TOK_TILE, dyv, mode)
        w, b = tail_in(wv, mode), tail_in(bv, mode)
        y = Frame.out((batch,), length, pitched, 0, TOK_TILE, dtype, dev, mode)
        dx = Frame.out((batch,), length, half, 0, TOK_TILE, dtype, dev, mode)
        dwp, dbp = Flat((nparts, dim, width), dev, mode, dim * width), Flat((nparts, dim), dev, mode, dim)
        dw, db = Flat((dim, width), dev, mode, width), Flat((dim,), dev, mode, PAD)
        a = aum_hip.ConvTmArgs()
        a.weight, a.bias = _ptr(w), _ptr(b)
        _set3(a, "x", x.view)
        _set3(a, "y", y.view)
        a.batch, a.dim, a.len, a.width, a.dtype = batch, dim, length, width, aum_hip._DT[dtype]
        a.flags = (aum_hip.CONV_SILU if silu else 0) | (aum_hip.CONV_REVERSE if reverse else 0)
        st = lib.stream(xv)
        _ok(lib.c.aum_conv1d_tm_fwd(aum_hip.C_byref(a), st), "aum_conv1d_tm_fwd")
        a.y = None
        a.y_bs = a.y_ts = 0
        _set3(a, "dy", dy.view)
        _set3(a, "dx", dx.view)
        a.dw_part, a.db_part = _ptr(dwp.view), _ptr(dbp.view) if b is not None else None
        _ok(lib.c.aum_conv1d_tm_bwd(aum_hip.C_byref(a), st), "aum_conv1d_tm_bwd")
        outs = dict(y=y.view, dx=dx.view, dw_part=dwp.view, dw=aum_hip.sum_rows(dwp.view, lib=lib, out=dw.view))
        guards = y.guards("y") + dx.guards("dx") + dwp.guards("dw_part") + dbp.guards("db_part") + dw.guards("dweight") + db.guards("dbias")
        if b is not None:
            outs.update(db_part=dbp.view, db=aum_hip.sum_rows(dbp.view, lib=lib, out=db.view))
        else:
            guards.append(("db_part: written without a bias", dbp.view, FILL_OUT[mode]))
        assert outs["dw"].data_ptr() == dw.view.data_ptr()
        return outs, guards

    got = run_pair((name, str(dtype), "rev" if reverse else "fwd", silu), run, dev)
    return KC.conv_tm_assert(name, dtype, got["y"], got["dx"], got["dw"], got.get("db"), ry, rg)


# ---- token-major scans ----------------------------------------------------------------------------------------------------------------------
XDBL_COLS, XDBL_R = 80, 48      # B | C are columns 48..80 of 80-column x_dbl rows


def check_scan_tm_poison(lib, dev, case, dtype, direction, segments=1):
    """aum_scan_tm_fwd / _bwd (segments > 1: aum_scan_tm_seg_fwd / _seg_bwd); direction: "fwd", "rev" or "bidir".  All through the C entry
    points (the binding allocates every output, the carries and the workspace itself); the input layouts are ones the binding takes too:
    u, delta, dout, out_pre (as the backward's input)   pitch dim + 8 -- padding and 8 time steps behind each batch entry poisoned
    z        the second half of [x | z] rows of 2 dim + 8 -- x half, padding and steps behind poisoned
    B | C    columns 48..80 of 80-column rows -- the dt columns and the steps behind poisoned
    out, out_pre, the inference form's out, du, ddelta   pitch dim + 8, guarded: padding, steps behind
    dz       the second half of [dx | dz] rows of 2 dim + 8, guarded: dx half, padding, steps behind
    dBC, dA, dA_b, dD, ddelta_bias, dA_xA, dA_b_xA       contiguous in the ABI: NaN pre-fill, sentinel rows behind
    checkpoint, segment carries, workspace                contiguous: NaN pre-fill, a sentinel tail behind the size the library asks for
    A, A_b, D, delta_bias                                 contiguous in the ABI: poison behind the last row only"""
    name, batch, dim, length, dstate, has_z, has_D, has_bias, softplus = case
    reverse, bidir = direction == "rev", direction == "bidir"
    ref = KC.scan_tm_reference(case, dtype, reverse, bidir)
    d = ref["inputs"]
    tm = lambda a: None if a is None else KC.T(a, dev, dtype).transpose(1, 2).contiguous()      # (batch, len, X)
    uv, dlv, zv, doutv = tm(d["u"]), tm(d["delta"]), tm(d["z"]), tm(d["dout"])
    bcv = torch.cat([tm(d["B"]), tm(d["C"])], dim=2)
    Av, Abv, Dv, biasv = KC.T(d["A"], dev), KC.T(ref["A_b"], dev), KC.T(d["D"], dev), KC.T(d["delta_bias"], dev)
    ndir, nck = (2 if bidir else 1), max(int(lib.c.aum_scan_tm_nck(length)), 1)
    ck_rows = int(lib.c.aum_scan_tm_ckpt_rows(aum_hip._DT[dtype]))
    if segments > 1:
        carry_bytes = int(lib.c.aum_scan_tm_seg_carry_bytes(batch, dim, length, dstate, int(bidir), segments))
        ws_bytes = int(lib.c.aum_scan_tm_seg_workspace_bytes(batch, dim, length, dstate, int(bidir), segments))
        assert carry_bytes > 0 and ws_bytes > 0, (name, segments, "segments refused for this shape")
    else:
        carry_bytes, ws_bytes = 0, int(lib.c.aum_scan_tm_workspace_bytes(batch, dim, length, dstate, int(bidir)))
    pitched = [("row", dim), ("past dim", PAD)]
    second = lambda other: [(f"into the {other} half", dim), ("row", dim), ("past the row", PAD)]
    flags = (aum_hip.SCAN_SOFTPLUS if softplus else 0) | (aum_hip.SCAN_REVERSE if reverse else 0)
    st = lib.stream(uv)

    def run(mode):
        inp = lambda v, blocks=pitched, own=0: None if v is None else Frame.inp((batch,), length, blocks, own, SCAN_TILE, v, mode)
        out_ = lambda blocks=pitched, own=0: Frame.out((batch,), length, blocks, own, SCAN_TILE, dtype, dev, mode)
        u, delta, dout, z = inp(uv), inp(dlv), inp(doutv), inp(zv, second("x"), 1)
        bc = inp(bcv, [("into the dt block", XDBL_R), ("B | C", 2 * dstate)], 1)
        A, Ab, D, bias = tail_in(Av, mode), tail_in(Abv, mode), tail_in(Dv, mode), tail_in(biasv, mode)
        guards = []

        def common(a):
            _set3(a, "u", u.view)
            _set3(a, "delta", delta.view)
            if z is not None:
                _set3(a, "z", z.view)
            _set3(a, "B", bc.view[..., :dstate])
            _set3(a, "C", bc.view[..., dstate:])
            a.A, a.A_b, a.D, a.delta_bias = _ptr(A), _ptr(Ab), _ptr(D), _ptr(bias)
            a.batch, a.dim, a.len, a.dstate, a.dtype, a.flags = batch, dim, length, dstate, aum_hip._DT[dtype], flags

        def forward(what, want_pre, ck):
            out, pre = out_(), out_() if want_pre else None
            a = aum_hip.ScanTmFwdArgs()
            common(a)
            _set3(a, "out", out.view)
            if pre is not None:
                _set3(a, "out_pre", pre.view, "pre")
            a.ckpt = _ptr(None if ck is None else ck.view)
            guards.extend(out.guards(what, "time step") + (pre.guards(what + "_pre", "time step") if pre is not None else []))
            if segments == 1:
                _ok(lib.c.aum_scan_tm_fwd(aum_hip.C_byref(a), st), "aum_scan_tm_fwd")
            else:
                carry = Flat((carry_bytes // 4,), dev, mode, 64)
                sa = aum_hip.ScanTmSegFwdArgs()
                sa.base, sa.carry, sa.carry_bytes, sa.segments = a, _ptr(carry.view), carry_bytes, segments
                _ok(lib.c.aum_scan_tm_seg_fwd(aum_hip.C_byref(sa), st), "aum_scan_tm_seg_fwd")
                guards.extend(carry.guards(what + " segment carries"))
            return out, pre

        ck = Flat((ndir, batch, nck, ck_rows, dim), dev, mode, dim)
        guards.extend(ck.guards("checkpoint"))
        out, pre = forward("out", True, ck)
        out2, _ = forward("out (inference form)", False, None)
        # backward: the forward's out_pre as an input of its own, poison around it
        pre_in = inp(pre.view) if z is not None else None
        du, ddelta, dz = out_(), out_(), out_(second("dx"), 1) if z is not None else None
        f32 = lambda shape, extra: Flat(shape, dev, mode, extra)
        dBC, dA, dA_xA = f32((batch, length, 2 * dstate), SCAN_TILE * 2 * dstate), f32((dim, dstate), dstate), f32((dim, dstate), dstate)
        dA_b, dA_b_xA = (f32((dim, dstate), dstate), f32((dim, dstate), dstate)) if bidir else (None, None)
        dD, dbias = f32((dim,), 64) if D is not None else None, f32((dim,), 64) if bias is not None else None
        ws = f32((max(ws_bytes, 4) // 4,), 64)
        b = aum_hip.ScanTmBwdArgs()
        common(b)
        _set3(b, "dout", dout.view)
        _set3(b, "du", du.view)
        _set3(b, "ddelta", ddelta.view)
        if z is not None:
            _set3(b, "out_pre", pre_in.view, "pre")
            _set3(b, "dz", dz.view)
        view = lambda f: None if f is None else f.view
        b.ckpt, b.dBC, b.dA, b.dA_b, b.dD, b.ddelta_bias = map(_ptr, map(view, (ck, dBC, dA, dA_b, dD, dbias)))
        b.dA_xA, b.dA_b_xA = _ptr(view(dA_xA)), _ptr(view(dA_b_xA))
        b.workspace, b.workspace_bytes = _ptr(ws.view), ws_bytes
        if segments == 1:
            _ok(lib.c.aum_scan_tm_bwd(aum_hip.C_byref(b), st), "aum_scan_tm_bwd")
        else:
            sb = aum_hip.ScanTmSegBwdArgs()
            sb.base, sb.segments = b, segments
            _ok(lib.c.aum_scan_tm_seg_bwd(aum_hip.C_byref(sb), st), "aum_scan_tm_seg_bwd")
        outs = dict(out=out.view, out_pre=pre.view, out_nopre=out2.view, du=du.view, ddelta=ddelta.view)
        guards.extend(du.guards("du", "time step") + ddelta.guards("ddelta", "time step") + ws.guards("workspace"))
        if dz is not None:
            outs["dz"] = dz.view
            guards.extend(dz.guards("dz", "time step"))
        for k, f in (("dBC", dBC), ("dA", dA), ("dA_xA", dA_xA), ("dA_b", dA_b), ("dA_b_xA", dA_b_xA), ("dD", dD), ("ddelta_bias", dbias)):
            if f is not None:
                outs[k] = f.view
                guards.extend(f.guards(k))
        return outs, guards

    got = run_pair((name, str(dtype), direction, segments), run, dev)
    # (check_scan_tm's own side assertion: the products d A .* A come out of the same partial-sum launch, exactly dA * A in fp32)
    assert torch.equal(got["dA_xA"], got["dA"] * Av) and (not bidir or torch.equal(got["dA_b_xA"], got["dA_b"] * Abv))
    g = {k: got.get(k) for k in ("du", "ddelta", "dz", "dBC", "dA", "dA_b", "dD", "ddelta_bias")}
    return KC.scan_tm_assert(case, dtype, reverse, bidir, None, ref, got["out"], got["out_pre"], got["out_nopre"], g)


# ---- dt projection ------------------------------------------------------------------------------------------------------------------------
def _weight(values, mode):
    """a weight matrix with a pitch in the ABI: padding behind its rows and W_ROWS rows behind the last one poisoned"""
    return Frame.inp((), values.shape[0], [("w", values.shape[1]), ("padding", PAD)], 0, W_ROWS, values, mode)


def check_dtproj_poison(lib, dev, ntok, dim, rank, ncols, dtype):
    """aum_dtproj_tm_fwd, through the C entry point (the binding allocates the output and gives it no pitch):
    x_dbl   the first `rank` columns of (ntok + 130, ncols) rows -- the B | C columns rank..ncols and the rows behind ntok poisoned (the
            binding takes this layout too)
    w       pitch rank + 8 -- padding and 8 rows behind poisoned
    out     pitch dim + 8, guarded: padding, 130 rows behind"""
    g = torch.Generator().manual_seed(ntok * 131 + dim + rank)
    xv = torch.randn(ntok, ncols, generator=g).to(dtype).to(dev)[:, :rank]
    wv = (torch.randn(dim, rank, generator=g) / rank ** 0.5).to(dtype).to(dev)

    def run(mode):
        x = Frame.inp((), ntok, [("dt", rank), ("into the B|C block", ncols - rank)], 0, TOK_TILE, xv, mode)
        w = _weight(wv, mode)
        out = Frame.out((), ntok, [("delta", dim), ("past dim", PAD)], 0, TOK_TILE, dtype, dev, mode)
        a = aum_hip.DtProjArgs()
        a.x, a.w, a.out = _ptr(x.view), _ptr(w.view), _ptr(out.view)
        a.ntok, a.dim, a.rank, a.ldx, a.ldw, a.ldo, a.dtype = ntok, dim, rank, x.view.stride(0), w.view.stride(0), out.view.stride(0), aum_hip._DT[dtype]
        _ok(lib.c.aum_dtproj_tm_fwd(aum_hip.C_byref(a), lib.stream(xv)), "aum_dtproj_tm_fwd")
        return dict(delta=out.view), out.guards("delta")

    got = run_pair(("dtproj", ntok, dim, rank, ncols, str(dtype)), run, dev)
    KC.dtproj_assert(got["delta"], xv, wv, rank, dtype)


# ---- x / dt projections ---------------------------------------------------------------------------------------------------------------------
def _xdt_pair(lib, dev, tag, uv, wxv, wdtv, dtype):
    ntok, dim = uv.shape
    ncols, rank = wxv.shape[0], wdtv.shape[1]

    def run(mode):
        u = Frame.inp((), ntok, [("x", dim), ("into the z half", dim)], 0, TOK_TILE, uv, mode)
        wx, wdt = _weight(wxv, mode), _weight(wdtv, mode)
        x_dbl = Frame.out((), ntok, [("x_dbl", ncols), ("past its last column", PAD)], 0, TOK_TILE, dtype, dev, mode)
        delta = Frame.out((), ntok, [("delta", dim), ("past dim", PAD)], 0, TOK_TILE, dtype, dev, mode)
        a = aum_hip.XdtArgs()
        a.u, a.wx, a.wdt, a.x_dbl, a.delta = map(_ptr, (u.view, wx.view, wdt.view, x_dbl.view, delta.view))
        a.ntok, a.dim, a.rank, a.ncols, a.dtype = ntok, dim, rank, ncols, aum_hip._DT[dtype]
        a.ldu, a.ldwx, a.ldwdt, a.ldx, a.ldd = (t.view.stride(0) for t in (u, wx, wdt, x_dbl, delta))
        _ok(lib.c.aum_xdt_tm_fwd(aum_hip.C_byref(a), lib.stream(uv)), "aum_xdt_tm_fwd")
        return dict(x_dbl=x_dbl.view, delta=delta.view), x_dbl.guards("x_dbl") + delta.guards("delta")

    return run_pair(tag, run, dev)


def check_xdt_poison(lib, dev, ntok, dim, rank, dtype, ncols=80):
    """aum_xdt_tm_fwd, through the C entry point (the binding allocates both outputs and gives them no pitch):
    u            the first half of (ntok + 130, 2 dim) rows -- the z half and the rows behind ntok poisoned (the binding takes this too)
    wx, wdt      pitch + 8 -- padding and 8 rows behind poisoned
    x_dbl        pitch ncols + 8, guarded: padding, 130 rows behind
    delta        pitch dim + 8, guarded: padding, 130 rows behind"""
    g = torch.Generator().manual_seed(ntok * 7 + dim + rank + ncols)
    uv = torch.randn(ntok, dim, generator=g).to(dtype).to(dev)
    wxv = (torch.randn(ncols, dim, generator=g) / dim ** 0.5).to(dtype).to(dev)
    wdtv = (torch.randn(dim, rank, generator=g) / rank ** 0.5).to(dtype).to(dev)
    got = _xdt_pair(lib, dev, ("xdt", ntok, dim, rank, ncols, str(dtype)), uv, wxv, wdtv, dtype)
    KC.xdt_assert(got["x_dbl"], got["delta"], uv, wxv, wdtv, dtype)


def check_xdt_tiny_poison(lib, dev, dt):
    """aum_xdt_tm_fwd at AuM-Tiny's padded width (48 columns, rank 16) and the smallest token count of xdt_tiny_checks.NTOKS: operands
    treated as in check_xdt_poison, held to xdt_tiny_checks' reference (the unpadded weights in fp64) and bar, pad columns exactly +0"""
    ntok = min(TC.NTOKS)
    wx44, wdt12 = TC.weights(dt, dev, seed=ntok)
    wx, wdt = TC.pad_weights(wx44, wdt12)
    uv = torch.randn(ntok, TC.DIM, generator=torch.Generator().manual_seed(ntok)).to(TC.DT[dt]).to(dev)
    got = _xdt_pair(lib, dev, ("xdt tiny", ntok, dt), uv, wx, wdt, TC.DT[dt])
    TC.assert_xdt_fwd(got["x_dbl"], got["delta"], uv, wx44, wdt12, None, dt, False)


def check_xdt_bwd_poison(lib, dev, ntok, dim, dtype, pad):
    """aum_xdt_tm_bwd, through the C entry point (the binding allocates dx_dbl and gives it no pitch):
    ddelta   pitch dim + pad -- padding and 130 rows behind poisoned (the binding takes this too)
    dbc      fp32, pitch 32 + 8 -- padding and 130 rows behind poisoned
    du       in place, pitch dim + pad: the padding holds the sentinel (check_xdt_bwd's tail guard), the 130 rows behind hold poison and
             must come back bit for bit
    wdt_t, wx_t   pitch + 8 -- padding and 8 rows behind poisoned
    dx_dbl   pitch 80 + 8, guarded: padding, 130 rows behind"""
    g = torch.Generator().manual_seed(ntok * 5 + dim)
    R, C = 48, 80
    ddv = torch.randn(ntok, dim + pad, generator=g).to(dtype).to(dev)[:, :dim]
    duv = torch.randn(ntok, dim + pad, generator=g).to(dtype).to(dev)[:, :dim]
    dbcv = torch.randn(ntok, C - R, generator=g).to(dev)
    wdtv = (torch.randn(R, dim, generator=g) / dim ** 0.5).to(dtype).to(dev)
    wxv = (torch.randn(dim, C, generator=g) / C ** 0.5).to(dtype).to(dev)

    def run(mode):
        ddelta = Frame.inp((), ntok, [("ddelta", dim), ("padding", pad)], 0, TOK_TILE, ddv, mode)
        dbc = Frame.inp((), ntok, [("dbc", C - R), ("padding", PAD)], 0, TOK_TILE, dbcv, mode)
        du = Frame.inp((), ntok, [("du", dim), ("padding", pad)], 0, TOK_TILE, duv, mode)
        du.buf[:ntok, dim:] = SENTINEL
        wdt_t, wx_t = _weight(wdtv, mode), _weight(wxv, mode)
        dx = Frame.out((), ntok, [("dx_dbl", C), ("past its last column", PAD)], 0, TOK_TILE, dtype, dev, mode)
        a = aum_hip.XdtBwdArgs()
        a.ddelta, a.dbc, a.wdt_t, a.wx_t, a.du, a.dx_dbl = map(_ptr, (ddelta.view, dbc.view, wdt_t.view, wx_t.view, du.view, dx.view))
        a.ntok, a.dim, a.rank, a.ncols, a.dtype = ntok, dim, R, C, aum_hip._DT[dtype]
        a.ldd, a.lddbc, a.ldwdt, a.ldwx, a.ldu, a.ldx = (t.view.stride(0) for t in (ddelta, dbc, wdt_t, wx_t, du, dx))
        _ok(lib.c.aum_xdt_tm_bwd(aum_hip.C_byref(a), lib.stream(ddv)), "aum_xdt_tm_bwd")
        guards = dx.guards("dx_dbl") + [("du: wrote past dim", du.buf[:ntok, dim:], SENTINEL),
                                        ("du: wrote behind the last token", du.buf[ntok:], FILL_IN[mode])]
        return dict(dx_dbl=dx.view, du=du.view), guards

    got = run_pair(("xdt_bwd", ntok, dim, pad, str(dtype)), run, dev)
    KC.xdt_bwd_assert(got["dx_dbl"], got["du"], duv.double().cpu(), ddv, dbcv, wdtv, wxv, dtype)


# ---- GEMMs ----------------------------------------------------------------------------------------------------------------------------------
def check_gemm_poison(lib, dev, m, n, k, dtype, flags=0, refused=False):
    """aum_gemm_tn, through the binding (strided a, out=):
    a   the first k columns of (m + 260, k + 64) rows -- the 64 columns behind and the 260 rows behind poisoned
    b   pitch k + 8 -- padding and 8 rows behind poisoned
    c   guarded as check_gemm guards it -- 8 columns in front, 8 behind, 260 rows behind -- plus the pre-filled interior
    refused: a schedule the shape does not admit (the paced one below k = 448) is refused and leaves all of c as it was"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(f"poison_{m}_{n}_{k}".encode()))
    av = torch.randn(m, k, generator=g).to(dtype).to(dev)
    bv = (torch.randn(n, k, generator=g) / k ** 0.5).to(dtype).to(dev)

    def run(mode):
        a = Frame.inp((), m, [("a", k), ("padding", 64)], 0, 260, av, mode)
        b = _weight(bv, mode)
        c = Frame.out((), m, [("in front of the result", PAD), ("c", n), ("past n", PAD)], 1, 260, dtype, dev, mode)
        if refused:
            with pytest.raises(RuntimeError, match="UNSUPPORTED"):
                aum_hip.gemm_tn(a.view, b.view, out=c.view, lib=lib, flags=flags)
            return {}, c.guards("c") + [("c: a refused call wrote to the result", c.view, FILL_OUT[mode])]
        out = aum_hip.gemm_tn(a.view, b.view, out=c.view, lib=lib, flags=flags)
        assert out.data_ptr() == c.view.data_ptr()
        return dict(c=c.view), c.guards("c")

    got = run_pair(("gemm_tn", m, n, k, str(dtype), flags), run, dev)
    if not refused:
        KC.gemm_assert(f"poison_{m}_{n}_{k}", got["c"], av, bv, dtype)


def check_gemm_wgrad_poison(lib, dev, t, n, k, splits, dtype, pad_y=0, pad_x=0):
    """aum_gemm_wgrad, through the C entry point (the binding allocates the partial tiles itself):
    y      columns pad_y.. of (t + 130, pad_y + n + 8) rows -- the columns in front and behind and the rows behind t poisoned
    x      the first k columns of (t + 130, k + max(pad_x, 8)) rows -- the columns behind and the rows behind t poisoned
           (both layouts the binding takes too)
    part   contiguous in the ABI: NaN pre-fill, one sentinel split behind the `splits` tiles; an empty split comes back as zeros"""
    g = torch.Generator().manual_seed(t * 7 + n + k + splits)
    yv = torch.randn(t, n + pad_y, generator=g).to(dtype).to(dev)[:, pad_y:]
    xv = torch.randn(t, k + pad_x, generator=g).to(dtype).to(dev)[:, :k]
    chunk = (((t + splits - 1) // splits) + 63) // 64 * 64

    def run(mode):
        y = Frame.inp((), t, [("front", pad_y), ("y", n), ("padding", PAD)], 1, TOK_TILE, yv, mode)
        x = Frame.inp((), t, [("x", k), ("padding", max(pad_x, PAD))], 0, TOK_TILE, xv, mode)
        part = Flat((splits, n, k), dev, mode, n * k)
        total = Flat((n, k), dev, mode, k)
        a = aum_hip.GemmWArgs()
        a.y, a.x, a.part = _ptr(y.view), _ptr(x.view), _ptr(part.view)
        a.t, a.ldy, a.ldx, a.n, a.k, a.splits, a.dtype = t, y.view.stride(0), x.view.stride(0), n, k, splits, aum_hip._DT[dtype]
        _ok(lib.c.aum_gemm_wgrad(aum_hip.C_byref(a), lib.stream(yv)), "aum_gemm_wgrad")
        outs = dict(part=part.view, total=aum_hip.sum_rows(part.view, lib=lib, out=total.view))
        assert outs["total"].data_ptr() == total.view.data_ptr()
        return outs, part.guards("part") + total.guards("the summed result")

    got = run_pair(("gemm_wgrad", t, n, k, splits, str(dtype)), run, dev)
    for s_ in range(splits):
        if min(s_ * chunk, t) == t:
            assert bool((got["part"][s_] == 0).all()), (t, n, k, splits, s_, "an empty split is not zeros")
    KC.gemm_wgrad_assert(got["part"], got["total"], yv, xv, splits)
