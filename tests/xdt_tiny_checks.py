"""Checks of AuM-Tiny's widths on the x/dt forward kernel and the one-launch streaming block, shared by tests/test_xdt_tiny.py (CPU,
lane-array library) and tests/test_gpu_xdt_tiny.py (device library).

Tiny is d_inner 384, dt_rank 12, d_state 16: x_dbl rows of 44 columns.  The kernels see the PADDED layout of Mamba.stream_params --
w_x (48, 384) = [dt 12 | 4 zero rows | B 16 | C 16], w_dt (384, 16) with zero columns 12..15, ncols 48, rank 16.  Expected values come
from the UNPADDED (44, 384) / (384, 12) weights, rounded to the 16-bit type, multiplied in fp64; bars are the project's 16-bit bar (1e-2,
stream_checks.OUT_BAR) and, for the block, the bars and the fp64 restatement of tests/stream_block_checks.py."""
import numpy as np
import torch

import aum_hip
import stream_block_checks as bc
from conftest import rel_err
from stream_checks import CACHE_BAR, DT, OUT_BAR

DIM, R, RP, N, NCOLS = 384, 12, 16, 16, 48
SENTINEL = bc.SENTINEL
NTOKS = (1, 16, 17, 16 * 8 + 1)          # one lane's worth, one fragment, a ragged second fragment, one more than a full 8-wave workgroup


def pad_weights(wx44, wdt12):
    """the layout Mamba.stream_params builds"""
    wx = wx44.new_zeros(NCOLS, DIM)
    wx[:R], wx[RP:] = wx44[:R], wx44[R:]
    wdt = wdt12.new_zeros(DIM, RP)
    wdt[:, :R] = wdt12
    return wx, wdt


def weights(dt, device, seed=0):
    g = torch.Generator().manual_seed(4400 + seed)
    wx44 = (torch.randn(R + 2 * N, DIM, generator=g) * DIM ** -0.5).to(DT[dt]).to(device)
    wdt12 = (torch.randn(DIM, R, generator=g) * R ** -0.5).to(DT[dt]).to(device)
    return wx44, wdt12


def _is_pos_zero(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


def _softplus64(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def check_xdt_fwd(lib, device, ntok, dt, softplus):
    """x_dbl and delta of the padded operands against the fp64 products of the unpadded weights; the pad columns exactly +0"""
    wx44, wdt12 = weights(dt, device, seed=ntok)
    wx, wdt = pad_weights(wx44, wdt12)
    g = torch.Generator().manual_seed(ntok)
    u = torch.randn(ntok, DIM, generator=g).to(DT[dt]).to(device)
    bias = (torch.randn(DIM, generator=g) * 0.5 - 1.0).to(device) if softplus else None
    assert aum_hip.xdt_tm_supported(u, wx, wdt)
    x_dbl, delta = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib, delta_bias=bias, delta_softplus=softplus)
    assert_xdt_fwd(x_dbl, delta, u, wx44, wdt12, bias, dt, softplus)
    return x_dbl, delta


def assert_xdt_fwd(x_dbl, delta, u, wx44, wdt12, bias, dt, softplus):
    """the bars of check_xdt_fwd on the outputs of one call (also what tests/poison_checks.py holds the padded width to)"""
    ntok = u.shape[0]
    f = lambda t: t.detach().double().cpu().numpy()
    ref_x = f(u) @ f(wx44).T                                        # (ntok, 44)
    ref_d = ref_x[:, :R] @ f(wdt12).T
    if softplus:
        ref_d = _softplus64(ref_d + f(bias)[None, :])
    assert x_dbl.shape == (ntok, NCOLS) and delta.shape == (ntok, DIM) and x_dbl.dtype == delta.dtype == DT[dt]
    e_dt, e_bc, e_d = rel_err(f(x_dbl[:, :R]), ref_x[:, :R]), rel_err(f(x_dbl[:, RP:]), ref_x[:, R:]), rel_err(f(delta), ref_d)
    print(f"xdt_tm_fwd tiny {dt} ntok={ntok} softplus={softplus}: dt block {e_dt:.3e}, B | C {e_bc:.3e}, delta {e_d:.3e} (bar {OUT_BAR[dt]:.0e})")
    assert e_dt < OUT_BAR[dt] and e_bc < OUT_BAR[dt]
    assert e_d < OUT_BAR[dt]
    assert _is_pos_zero(x_dbl[:, R:RP]), "the pad columns of x_dbl are not exactly +0"


def check_pad_columns_unread(lib, device, ntok, dt, softplus):
    """delta does not depend on w_dt's pad columns: whatever they hold meets an exact zero of x_dbl"""
    wx44, wdt12 = weights(dt, device, seed=7)
    wx, wdt = pad_weights(wx44, wdt12)
    g = torch.Generator().manual_seed(70 + ntok)
    u = torch.randn(ntok, DIM, generator=g).to(DT[dt]).to(device)
    bias = (torch.randn(DIM, generator=g) * 0.5 - 1.0).to(device) if softplus else None
    x0, d0 = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib, delta_bias=bias, delta_softplus=softplus)
    wdt2 = wdt.clone()
    wdt2[:, R:] = (torch.randn(DIM, RP - R, generator=g) * 100.0).to(DT[dt]).to(device)
    x1, d1 = aum_hip.xdt_tm_fwd(u, wx, wdt2, lib=lib, delta_bias=bias, delta_softplus=softplus)
    assert torch.equal(x0, x1) and torch.equal(d0, d1)


# ---- the one-launch block -----------------------------------------------------------------------------------------------------------
def operands(dt, total, nrows, device, seed=0):
    """stream_block_checks.operands at Tiny's shape with the padded plan; o["rank"] is the PADDED rank (the offset of B in x_dbl rows),
    which is what the shared three_launches / oracle64 of stream_block_checks index with"""
    g = torch.Generator().manual_seed(2000 + seed + total)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    xz = r(total, 2 * DIM).to(DT[dt]).to(device)
    wx44, wdt12 = r(R + 2 * N, DIM, scale=DIM ** -0.5).to(DT[dt]), r(DIM, R, scale=R ** -0.5).to(DT[dt])
    wx, wdt = pad_weights(wx44, wdt12)
    plan = bc.Plan(r(DIM, 4, scale=0.5).to(device), r(DIM, scale=0.1).to(device), (-torch.exp(r(DIM, 16, scale=0.5))).to(device), r(DIM).to(device),
                   (r(DIM, scale=0.5) - 2.0).to(device), wx.to(device), wdt.to(device), DT[dt])
    conv, state = torch.full((nrows, DIM, 4), SENTINEL), torch.full((nrows, DIM, 16), SENTINEL)
    entry = (r(nrows, DIM, 4), r(nrows, DIM, 16, scale=0.3))
    return {"xz": xz, "x": xz[:, :DIM], "z": xz[:, DIM:], "plan": plan, "conv": conv.to(device), "state": state.to(device),
            "entry": (entry[0].to(device), entry[1].to(device)), "dim": DIM, "rank": RP, "dt": dt}


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def oracle_errors(o, y, conv, state, lens, rows):
    """every session of a pack against stream_block_checks.oracle64 -- conv -> projections -> scan in fp64 from that session's own entry
    window and state and its own rows -> per session (y, exit state, exit window) rel_err"""
    n = lambda t: t.detach().float().cpu().numpy()
    out, at = [], 0
    for T, r_ in zip(lens, rows):
        one = dict(o, x=o["x"][at:at + T], z=o["z"][at:at + T], entry=(o["entry"][0][r_:r_ + 1], o["entry"][1][r_:r_ + 1]))
        ref_y, ref_h, ref_win = bc.oracle64(one, T)
        out.append((rel_err(n(y[at:at + T]), ref_y), rel_err(n(state[r_]), ref_h), rel_err(n(conv[r_]), ref_win)))
        at += T
    return out


def assert_oracle_bars(what, dt, lens, rows, errs):
    for T, r_, e in zip(lens, rows, errs):
        print(f"{what} tiny {dt} session of {T} rows on pool row {r_} vs fp64: y {e[0]:.3e} (bar {OUT_BAR[dt]:.0e}), state {e[1]:.3e} "
              f"(bar {bc.STATE_BAR[dt]:.0e}), window {e[2]:.3e} (bar {CACHE_BAR:.0e})")
        assert e[0] < OUT_BAR[dt], (T, r_)
        assert e[1] < bc.STATE_BAR[dt], (T, r_)
        assert e[2] < CACHE_BAR, (T, r_)


def check_block(dt, lens, rows, nrows, lib, device):
    """window and state start from non-zero carried values.  The one launch is bit for bit the three launches, and y and both pools are
    within the streaming bars of the fp64 restatement, session by session; commit=False leaves the pools bitwise untouched and returns
    the same rows; peek=True leaves the pools of a push of all rows but each session's last and the last row of an uncommitted read;
    pool rows no session names are bitwise unchanged"""
    total = sum(lens)
    o = operands(dt, total, nrows, device, seed=len(lens))
    bc.seed_rows(o, rows)
    smap = aum_hip.seq_map(lens, rows, device=device)
    assert aum_hip.stream_block_supported(o["x"], o["z"], o["conv"], o["state"], o["plan"], max(lens))
    c0, s0 = o["conv"].clone(), o["state"].clone()
    c3, s3 = c0.clone(), s0.clone()
    y3 = bc.three_launches(o, smap, lib, conv=c3, state=s3)
    # commit=False first, on the live pools
    y0 = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], seq_map=smap, commit=False, lib=lib)
    _sync(device)
    assert torch.equal(o["conv"], c0) and torch.equal(o["state"], s0), "commit=False wrote a pool"
    c1, s1 = c0.clone(), s0.clone()
    y = aum_hip.stream_block(o["x"], o["z"], c1, s1, o["plan"], seq_map=smap, lib=lib)
    _sync(device)
    assert torch.equal(y, y3) and torch.equal(y0, y3)
    assert torch.equal(c1, c3) and torch.equal(s1, s3)
    assert_oracle_bars("stream_block", dt, lens, rows, oracle_errors(o, y, c1, s1, lens, rows))
    idle = sorted(set(range(nrows)) - set(rows))
    for r_ in idle:
        assert torch.equal(c1[r_], c0[r_]) and torch.equal(s1[r_], s0[r_]) and bool((c1[r_] == SENTINEL).all())
    for r_ in rows:
        assert not torch.equal(s1[r_], s0[r_])
    # peek=True: the pools of a push of all rows but each session's last, the last rows those of an uncommitted read from there
    body, last, at = [], [], 0
    for n in lens:
        body += list(range(at, at + n - 1))
        last.append(at + n - 1)
        at += n
    take = lambda t, ix: t.index_select(0, torch.tensor(ix, dtype=torch.int64, device=device))
    cr, sr = c0.clone(), s0.clone()
    y_ref = torch.zeros_like(y)
    if body:
        mb = aum_hip.seq_map([n - 1 for n in lens], rows, device=device)
        y_ref[body] = aum_hip.stream_block(take(o["x"], body), take(o["z"], body), cr, sr, o["plan"], seq_map=mb, lib=lib)
    ml = aum_hip.seq_map([1] * len(lens), rows, device=device)
    y_ref[last] = aum_hip.stream_block(take(o["x"], last), take(o["z"], last), cr, sr, o["plan"], seq_map=ml, commit=False, lib=lib)
    cp, sp = c0.clone(), s0.clone()
    yp = aum_hip.stream_block(o["x"], o["z"], cp, sp, o["plan"], seq_map=smap, peek=True, lib=lib)
    _sync(device)
    assert torch.equal(yp, y_ref) and torch.equal(cp, cr) and torch.equal(sp, sr)
    for r_ in idle:
        assert torch.equal(cp[r_], c0[r_]) and torch.equal(sp[r_], s0[r_])
    return o, y


def check_block_vs_oracle(dt, T, lib, device):
    """one session on row 0 against the fp64 restatement of stream_block_checks (conv -> projections -> scan, nothing rounded between):
    its bars, and the one launch's errors EQUAL the three launches'"""
    o = operands(dt, T, 1, device, seed=3)
    bc.seed_rows(o, [0])
    smap = aum_hip.seq_map([T], device=device)
    c3, s3 = o["conv"].clone(), o["state"].clone()
    y3 = bc.three_launches(o, smap, lib, conv=c3, state=s3)
    y = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], lib=lib)
    _sync(device)
    e, e3 = oracle_errors(o, y, o["conv"], o["state"], (T,), (0,)), oracle_errors(o, y3, c3, s3, (T,), (0,))
    assert e == e3
    assert_oracle_bars("stream_block (one session)", dt, (T,), (0,), e)


def check_chunk_invariance(dt, lib, device):
    """24 rows pushed as 24, as 8 + 16 and as 1 + 23: bitwise equal y and pools"""
    T = 24
    o = operands(dt, T, 1, device, seed=9)
    bc.seed_rows(o, [0])
    c0, s0 = o["conv"].clone(), o["state"].clone()
    y = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], lib=lib)
    for cut in (8, 1):
        c, s = c0.clone(), s0.clone()
        ya = aum_hip.stream_block(o["x"][:cut], o["z"][:cut], c, s, o["plan"], lib=lib)
        yb = aum_hip.stream_block(o["x"][cut:], o["z"][cut:], c, s, o["plan"], lib=lib)
        _sync(device)
        assert torch.equal(torch.cat([ya, yb]), y), cut
        assert torch.equal(c, o["conv"]) and torch.equal(s, o["state"]), cut


def check_scratch_bytes(lib):
    """xc and delta rows of dim, x_dbl rows of the padded width, 16-bit elements"""
    assert lib.c.aum_stream_block_scratch_bytes(10, DIM, NCOLS) == 2 * 10 * (2 * DIM + NCOLS)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def tiny_block(dtype, device="cpu"):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(12)
    m = Mamba(192, bimamba_type="none", layer_idx=0).to(device).to(dtype)
    assert (m.d_inner, m.dt_rank, m.d_state) == (DIM, R, N)
    return m


def check_tiny_plan(dtype):
    """stream_params() of a Tiny block: the padded layout in 16 bits (exact copies of the casts around exact zeros), the plain casts in fp32"""
    m = tiny_block(dtype)
    p = m.stream_params()
    wx, wdt = m.x_proj.weight.detach().to(dtype), m.dt_proj.weight.detach().to(dtype)
    if dtype == torch.float32:
        assert torch.equal(p.w_x, wx) and torch.equal(p.w_dt, wdt) and p.b_off == R
        return
    assert p.w_x.shape == (NCOLS, DIM) and p.w_dt.shape == (DIM, RP) and p.b_off == RP and p.w_x.dtype == p.w_dt.dtype == dtype
    assert torch.equal(p.w_x[:R], wx[:R]) and torch.equal(p.w_x[RP:], wx[R:]) and _is_pos_zero(p.w_x[R:RP])
    assert torch.equal(p.w_dt[:, :R], wdt) and _is_pos_zero(p.w_dt[:, R:])
    assert p.w_x.data_ptr() % 16 == 0 and p.w_dt.data_ptr() % 16 == 0 and p.w_x.is_contiguous() and p.w_dt.is_contiguous()
    assert m.stream_params() is p                                   # cached under the existing key rules
    x = torch.zeros(3, DIM, dtype=dtype)
    assert aum_hip.xdt_tm_supported(x, p.w_x, p.w_dt)
    conv, state = torch.zeros(1, DIM, 4), torch.zeros(1, DIM, 16)
    assert aum_hip.stream_block_supported(x, x, conv, state, p, 3)


def check_other_plans_unpadded():
    """Base- and Small-width blocks (and a width no kernel takes): tensors bitwise equal to the unpadded casts, the original rank and offset"""
    from mamba_ssm.modules.mamba_simple import Mamba
    for d_model, rank in ((768, 48), (384, 24), (64, 4)):
        torch.manual_seed(d_model)
        m = Mamba(d_model, bimamba_type="none", layer_idx=0)
        assert m.dt_rank == rank
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            p = m.stream_params(dtype)
            assert torch.equal(p.w_x, m.x_proj.weight.detach().to(dtype)) and torch.equal(p.w_dt, m.dt_proj.weight.detach().to(dtype))
            assert p.w_x.shape == (rank + 2 * N, m.d_inner) and p.w_dt.shape == (m.d_inner, rank) and p.b_off == rank
            assert p._fields[:8] == ("conv_w", "conv_b", "A", "D", "dt_bias", "w_x", "w_dt", "dtype")         # the fields callers knew, in their order


def check_xdt_fwd_other_width(lib, device, ncols, rank, dim, ntok, dt):
    """the widths the kernel had before, at dims the relaxed rule admits (dim % 256 == 128: a last prefetch round of two steps) and at
    one it took already: x_dbl against fp64, delta against the fp64 product of the kernel's own rounded dt block"""
    g = torch.Generator().manual_seed(dim + ncols + ntok)
    u = torch.randn(ntok, dim, generator=g).to(DT[dt]).to(device)
    wx = (torch.randn(ncols, dim, generator=g) * dim ** -0.5).to(DT[dt]).to(device)
    wdt = (torch.randn(dim, rank, generator=g) * rank ** -0.5).to(DT[dt]).to(device)
    assert aum_hip.xdt_tm_supported(u, wx, wdt)
    x_dbl, delta = aum_hip.xdt_tm_fwd(u, wx, wdt, lib=lib)
    f = lambda t: t.detach().double().cpu().numpy()
    e_x = rel_err(f(x_dbl), f(u) @ f(wx).T)
    e_d = rel_err(f(delta), f(x_dbl)[:, :rank] @ f(wdt).T)
    print(f"xdt_tm_fwd ({ncols}, {rank}) dim {dim} {dt} ntok={ntok}: x_dbl {e_x:.3e}, delta {e_d:.3e} (bar {OUT_BAR[dt]:.0e})")
    assert e_x < OUT_BAR[dt] and e_d < OUT_BAR[dt]


class count_calls:
    """counts the calls of aum_hip.<name> inside the block (how the stream-block tests tell the one launch from the ladder)"""

    def __init__(self, *names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        self.orig = {k: getattr(aum_hip, k) for k in self.names}
        for k in self.names:
            def wrap(*a, _k=k, **kw):
                self.n[_k] += 1
                return self.orig[_k](*a, **kw)
            setattr(aum_hip, k, wrap)
        return self.n

    def __exit__(self, *a):
        for k, v in self.orig.items():
            setattr(aum_hip, k, v)
