"""Checks of the one-launch recurrent middle of the causal block (aum_stream_block_tm, aum_hip.stream_block, Mamba.stream_params,
Mamba.step_chunk(commit=), AudioMamba.stream_read in place), shared by tests/test_stream_block.py (CPU, lane-array library) and
tests/test_gpu_stream_block.py (device library).

The acceptance property is BIT EQUALITY with the three launches conv1d_tm_chunk_var -> xdt_tm_fwd(delta_softplus) ->
scan_tm_chunk_var(delta_activated) on the same operands: y and both pools torch.equal, untouched pool rows still at the sentinel.
Against the fp64 oracle (conv -> projections -> scan on the whole sequence in fp64 from the same rounded inputs) the bar is not a new
number: the three-launch path goes through the same comparison, the fused error must EQUAL it, and both stay under the bars
stream_pool_checks.check_var_vs_oracle uses for these dtypes (OUT_BAR 1e-2 for the 16-bit outputs, CACHE_BAR 1e-4 for the conv window,
which holds fp32 copies of the inputs; the exit state is built from 16-bit intermediates and is held to OUT_BAR, see STATE_BAR)."""
import collections

import numpy as np
import torch

import aum_hip
from conftest import rel_err
from stream_checks import CACHE_BAR, DT, OUT_BAR, make_causal_aum

SENTINEL = 7.25
MAX_T = aum_hip.STREAM_BLOCK_MAX_T
SHAPES = {"small": (256, 56, 24), "base": (1536, 80, 48)}       # dim, x_dbl width, dt_rank
# The exit state against the fp64 oracle.  The conv window holds the inputs themselves (CACHE_BAR, fp32 exactness); the state does not:
# it is accumulated in fp32, but from xc, delta, B and C as the phases hand them on, each rounded to the 16-bit dtype (8 / 11 significant
# bits), while the oracle rounds nothing between its stages.  The state is a decayed sum of delta * xc * B terms, each a product of three
# rounded factors (relative error <= 3 * 2^-9 for bf16, 3 * 2^-12 for fp16, plus the rounding of xc inside the projections' inputs),
# so it is held to the bar of the 16-bit outputs, which are built from the same rounded factors -- not to the fp32 bar.
STATE_BAR = OUT_BAR
Plan = collections.namedtuple("Plan", "conv_w conv_b A D dt_bias w_x w_dt dtype")


def operands(shape, dt, total, nrows, device, seed=0):
    """free-standing random operands: in_proj rows [x | z] (total, 2 dim), a plan, sentinel-filled pools whose live rows the caller seeds"""
    dim, ncols, rank = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 + seed + total)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    xz = r(total, 2 * dim).to(DT[dt]).to(device)
    plan = Plan(r(dim, 4, scale=0.5).to(device), r(dim, scale=0.1).to(device),
                (-torch.exp(r(dim, 16, scale=0.5))).to(device), r(dim).to(device), (r(dim, scale=0.5) - 2.0).to(device),
                r(ncols, dim, scale=dim ** -0.5).to(DT[dt]).to(device), r(dim, rank, scale=rank ** -0.5).to(DT[dt]).to(device), DT[dt])
    conv = torch.full((nrows, dim, 4), SENTINEL)
    state = torch.full((nrows, dim, 16), SENTINEL)
    entry = (r(nrows, dim, 4), r(nrows, dim, 16, scale=0.3))
    return {"xz": xz, "x": xz[:, :dim], "z": xz[:, dim:], "plan": plan, "conv": conv.to(device), "state": state.to(device),
            "entry": (entry[0].to(device), entry[1].to(device)), "dim": dim, "rank": rank, "dt": dt}


def seed_rows(o, rows):
    for r in rows:
        o["conv"][r] = o["entry"][0][r]
        o["state"][r] = o["entry"][1][r]


def three_launches(o, smap, lib, x=None, z=None, conv=None, state=None):
    """the reference path: the three existing launches on the same operands; on the host library the xdt loop has no activation, so the
    scan applies bias and softplus (what the emulated aum_stream_block_tm composes)"""
    p, R = o["plan"], o["rank"]
    x, z = (o["x"], o["z"]) if x is None else (x, z)
    conv, state = (o["conv"], o["state"]) if conv is None else (conv, state)
    xc = aum_hip.conv1d_tm_chunk_var(x, conv, p.conv_w, p.conv_b, True, seq_map=smap, lib=lib)
    if lib.host:
        proj, delta = aum_hip.xdt_tm_fwd(xc, p.w_x, p.w_dt, lib=lib)
        return aum_hip.scan_tm_chunk_var(state, xc, delta, p.A, proj[:, R:R + 16], proj[:, R + 16:R + 32], p.D, z, p.dt_bias, True, False,
                                         seq_map=smap, lib=lib)
    proj, delta = aum_hip.xdt_tm_fwd(xc, p.w_x, p.w_dt, lib=lib, delta_bias=p.dt_bias, delta_softplus=True)
    return aum_hip.scan_tm_chunk_var(state, xc, delta, p.A, proj[:, R:R + 16], proj[:, R + 16:R + 32], p.D, z, None, False, True,
                                     seq_map=smap, lib=lib)


def check_fused_equals_three(shape, dt, lens, rows, nrows, lib, device, null_idx=False):
    total = sum(lens)
    o = operands(shape, dt, total, nrows, device)
    live = list(range(len(lens))) if null_idx else rows
    seed_rows(o, live)
    smap = aum_hip.seq_map(lens, None if null_idx else rows, device=device)
    c2, s2 = o["conv"].clone(), o["state"].clone()
    y_ref = three_launches(o, smap, lib, conv=c2, state=s2)
    y = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], seq_map=smap, lib=lib)
    at = 0
    for n in lens:          # rows of empty sessions do not exist; every row of the pack belongs to a session
        assert torch.equal(y[at:at + n], y_ref[at:at + n])
        at += n
    assert torch.equal(o["conv"], c2) and torch.equal(o["state"], s2)
    for r in set(range(nrows)) - set(live):
        assert torch.equal(o["conv"][r], torch.full_like(o["conv"][r], SENTINEL))
        assert torch.equal(o["state"][r], torch.full_like(o["state"][r], SENTINEL))
    for r, n in zip(live, lens):
        if n:
            assert not torch.equal(o["state"][r], o["entry"][1][r])
    return o, y


def check_partition(shape, dt, lib, device):
    o = operands(shape, dt, MAX_T, 1, device, seed=7)
    seed_rows(o, [0])
    c0, s0 = o["conv"].clone(), o["state"].clone()
    y = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], lib=lib)
    for cut in (1, 7, 8, MAX_T - 16):
        c, s = c0.clone(), s0.clone()
        ya = aum_hip.stream_block(o["x"][:cut], o["z"][:cut], c, s, o["plan"], lib=lib)
        yb = aum_hip.stream_block(o["x"][cut:], o["z"][cut:], c, s, o["plan"], lib=lib)
        assert torch.equal(torch.cat([ya, yb]), y), cut
        assert torch.equal(c, o["conv"]) and torch.equal(s, o["state"]), cut


def oracle64(o, T):
    """one session on row 0: conv -> projections -> scan over the whole sequence in fp64 from the rounded inputs, nothing rounded between"""
    f = lambda t: t.detach().double().cpu().numpy()
    p, dim, R = o["plan"], o["dim"], o["rank"]
    x, z = f(o["x"]), f(o["z"])
    w, b, A, D, db, wx, wdt = f(p.conv_w), f(p.conv_b), f(p.A), f(p.D), f(p.dt_bias), f(p.w_x), f(p.w_dt)
    win = np.concatenate([f(o["entry"][0][0]).T, x], axis=0)              # (4 + T, dim): the window, then the new inputs
    acc = b[None, :] + sum(win[k + 1:k + 1 + T] * w[None, :, k] for k in range(4))       # y[t] = b + sum_k w[k] in[t - 3 + k]
    xc = acc / (1 + np.exp(-acc))
    proj = xc @ wx.T
    dl = proj[:, :R] @ wdt.T + db[None, :]
    dl = np.where(dl > 20, dl, np.log1p(np.exp(np.minimum(dl, 20))))
    B, C = proj[:, R:R + 16], proj[:, R + 16:R + 32]
    h = f(o["entry"][1][0])
    ys = np.zeros((T, dim))
    for t in range(T):
        h = np.exp(dl[t][:, None] * A) * h + (dl[t] * xc[t])[:, None] * B[t][None, :]
        ys[t] = (h @ C[t] + D * xc[t]) * (z[t] / (1 + np.exp(-z[t])))
    return ys, h, win[T:].T


def check_vs_oracle(shape, dt, T, lib, device):
    o = operands(shape, dt, T, 1, device, seed=3)
    seed_rows(o, [0])
    ref_y, ref_h, ref_win = oracle64(o, T)
    smap = aum_hip.seq_map([T], device=device)
    c3, s3 = o["conv"].clone(), o["state"].clone()
    y3 = three_launches(o, smap, lib, conv=c3, state=s3)
    y = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], lib=lib)
    n = lambda t: t.detach().float().cpu().numpy()
    e = [rel_err(n(y), ref_y), rel_err(n(o["state"][0]), ref_h), rel_err(n(o["conv"][0]), ref_win)]
    e3 = [rel_err(n(y3), ref_y), rel_err(n(s3[0]), ref_h), rel_err(n(c3[0]), ref_win)]
    print(f"stream_block {shape} {dt} T={T} vs fp64: y {e[0]:.3e} (three launches {e3[0]:.3e}, bar {OUT_BAR[dt]:.0e}), "
          f"state {e[1]:.3e} ({e3[1]:.3e}), window {e[2]:.3e} ({e3[2]:.3e}), bar {CACHE_BAR:.0e}")
    assert e == e3
    assert e[0] < OUT_BAR[dt]
    assert e[1] < STATE_BAR[dt]
    assert e[2] < CACHE_BAR
    return e


def check_no_commit(shape, dt, lib, device):
    lens, rows = (3, 0, 17), (2, 0, 3)
    o = operands(shape, dt, sum(lens), 4, device, seed=5)
    seed_rows(o, rows)
    smap = aum_hip.seq_map(lens, rows, device=device)
    c0, s0 = o["conv"].clone(), o["state"].clone()
    y0 = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], seq_map=smap, commit=False, lib=lib)
    assert torch.equal(o["conv"], c0) and torch.equal(o["state"], s0)
    y1 = aum_hip.stream_block(o["x"], o["z"], o["conv"], o["state"], o["plan"], seq_map=smap, commit=True, lib=lib)
    assert torch.equal(y0, y1) and not torch.equal(o["state"], s0)


def raw_args(o, smap, y, scratch, lib, max_len=None):
    p = o["plan"]
    a = aum_hip.StreamBlockArgs()
    ptr = aum_hip._ptr
    a.x, a.z, a.conv_state, a.state, a.y, a.scratch = ptr(o["x"]), ptr(o["z"]), ptr(o["conv"]), ptr(o["state"]), ptr(y), ptr(scratch)
    a.conv_weight, a.conv_bias, a.wx, a.wdt = ptr(p.conv_w), ptr(p.conv_b), ptr(p.w_x), ptr(p.w_dt)
    a.A, a.D, a.delta_bias, a.cu_seqlens, a.state_indices = ptr(p.A), ptr(p.D), ptr(p.dt_bias), ptr(smap.cu), ptr(smap.idx)
    a.x_ts = a.z_ts = o["x"].stride(0)
    a.y_ts, a.scratch_bytes = y.stride(0), scratch.numel()
    a.total, a.nseq, a.nrows = o["x"].shape[0], len(smap.lens), o["conv"].shape[0]
    a.max_len = max(smap.lens) if max_len is None else max_len
    a.dim, a.width, a.dstate, a.rank, a.ncols = o["dim"], 4, 16, o["rank"], p.w_x.shape[0]
    a.ldwx, a.ldwdt, a.dtype, a.flags = p.w_x.stride(0), p.w_dt.stride(0), aum_hip._DT[o["x"].dtype], 0
    return a


def call_raw(a, t, lib):
    return lib.c.aum_stream_block_tm(aum_hip.C_byref(a), lib.stream(t))


def check_refusals(lib, device):
    """every refusal returns an error code and touches nothing"""
    def fresh(total, dt="bf16", shape="small"):
        o = operands(shape, dt, total, 2, device, seed=9)
        seed_rows(o, [0, 1])
        y = torch.full((total, o["dim"]), 3.0, dtype=o["x"].dtype, device=device)
        scratch = torch.zeros(max(int(lib.c.aum_stream_block_scratch_bytes(total, o["dim"], o["plan"].w_x.shape[0])), 16), dtype=torch.uint8, device=device)
        return o, y, scratch

    def untouched(o, y, snap):
        if device != "cpu":
            torch.cuda.synchronize()
        assert torch.equal(o["conv"], snap[0]) and torch.equal(o["state"], snap[1]) and bool((y == 3.0).all())

    # T = MAX_T + 1
    o, y, sc = fresh(MAX_T + 1)
    snap = (o["conv"].clone(), o["state"].clone())
    assert call_raw(raw_args(o, aum_hip.seq_map([MAX_T + 1], device=device), y, sc, lib), y, lib) == -4
    untouched(o, y, snap)
    assert not aum_hip.stream_block_supported(o["x"], o["z"], o["conv"], o["state"], o["plan"], MAX_T + 1)
    # dim 320
    o, y, sc = fresh(8)
    a = raw_args(o, aum_hip.seq_map([8], device=device), y, sc, lib)
    a.dim, a.ldwx = 320, 320
    snap = (o["conv"].clone(), o["state"].clone())
    assert call_raw(a, y, lib) == -4
    untouched(o, y, snap)
    # an fp32 activation
    a = raw_args(o, aum_hip.seq_map([8], device=device), y, sc, lib)
    a.dtype = aum_hip.AUM_F32
    assert call_raw(a, y, lib) == -3
    untouched(o, y, snap)
    assert not aum_hip.stream_block_supported(o["x"].float(), o["z"].float(), o["conv"], o["state"], o["plan"], 8)
    # an index outside the pool: a no-op for that session only
    o, y, sc = fresh(8)
    snap = (o["conv"].clone(), o["state"].clone())
    smap = aum_hip.seq_map([5, 3], [1, 2], device=device)          # row 2 does not exist in a pool of 2
    ref_c, ref_s = o["conv"].clone(), o["state"].clone()
    y_ref = three_launches(o, aum_hip.seq_map([5], [1], device=device), lib, x=o["x"][:5], z=o["z"][:5], conv=ref_c, state=ref_s)
    assert call_raw(raw_args(o, smap, y, sc, lib), y, lib) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(y[:5], y_ref) and bool((y[5:] == 3.0).all())
    assert torch.equal(o["conv"], ref_c) and torch.equal(o["state"], ref_s) and torch.equal(o["conv"][0], snap[0][0])


# ---- module and model ------------------------------------------------------------------------------------------------------------
def _fused(on):
    class _Ctx:
        def __enter__(self):
            self.old = aum_hip.debug.stream_fused
            aum_hip.debug.stream_fused = on

        def __exit__(self, *a):
            aum_hip.debug.stream_fused = self.old
    return _Ctx()


def check_mamba_arms(d_model, device):
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(11)
    m = Mamba(d_model, bimamba_type="none", layer_idx=0).to(device).to(torch.bfloat16)
    h = torch.randn(2, 9, d_model, device=device).to(torch.bfloat16)
    res = {}
    for on in (False, True):
        with _fused(on), torch.no_grad():
            c, s = m.allocate_inference_cache(2, 0, dtype=torch.float32)
            c.normal_(), s.normal_(std=0.3)
            torch.manual_seed(5)
            c.copy_(torch.randn(c.shape)), s.copy_(torch.randn(s.shape) * 0.3)
            out, _, _ = m.step_chunk(h, c, s)
            pc, ps = torch.full((4, *c.shape[1:]), SENTINEL, device=device), torch.full((4, *s.shape[1:]), SENTINEL, device=device)
            pc[3], pc[1], ps[3], ps[1] = c[0], c[1], s[0], s[1]
            smap = aum_hip.seq_map([4, 0, 5], [3, 0, 1], device=device)
            outp, _, _ = m.step_chunk(h.reshape(1, 18, d_model)[:, :9], pc, ps, seq_map=smap)
            res[on] = (out, c, s, outp, pc, ps)
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)
    assert torch.equal(res[True][4][2], torch.full_like(res[True][4][2], SENTINEL))


def check_model_arms(device):
    """hops and reads of one clip, batch and pool, fused on against fused off: every read's logits equal bit for bit; the last read
    against model(spec) under the existing 2e-2 bar; stream_read leaves every cache as it was and clones none of them when fused"""
    model = make_causal_aum(768, device, depth=4).to(torch.bfloat16)
    nt = model.patch_grid_size[1]
    torch.manual_seed(2)
    spec = torch.randn(2, nt * 16, 128, device=device).to(torch.bfloat16)
    reads = {}
    for on in (False, True):
        with _fused(on), torch.no_grad():
            cache = model.allocate_inference_cache(2)
            pool = model.allocate_stream_pool(3)
            got, c0 = [], 0
            for k in (1, 1, 2, 4, 8)[:None]:
                if c0 + k > nt:
                    break
                model.stream_push(spec[:, c0 * 16:(c0 + k) * 16], cache)
                model.stream_push_many([spec[0, c0 * 16:(c0 + k) * 16], spec[1, c0 * 16:(c0 + k) * 16]], pool, [2, 0])
                c0 += k
                snap = [(c.clone(), s.clone()) for c, s in list(cache["layers"].values()) + list(pool["layers"].values())]
                clones = []          # copies of cache rows: clone (every row) and index_select (named rows), by the shape of a row
                orig, orig_sel = torch.Tensor.clone, torch.Tensor.index_select
                torch.Tensor.clone = lambda self, *a, **kw: (clones.append(tuple(self.shape[1:])), orig(self, *a, **kw))[1]
                torch.Tensor.index_select = lambda self, *a, **kw: (clones.append(tuple(self.shape[1:])), orig_sel(self, *a, **kw))[1]
                try:
                    got.append(model.stream_read(cache))
                    got.append(model.stream_read(pool, sessions=[2, 0]))
                    got.append(model.stream_read(pool))
                finally:
                    torch.Tensor.clone, torch.Tensor.index_select = orig, orig_sel
                now = list(cache["layers"].values()) + list(pool["layers"].values())
                for (c, s), (c1, s1) in zip(now, snap):
                    assert torch.equal(c, c1) and torch.equal(s, s1)
                cache_shapes = {tuple(t.shape[1:]) for pair in now for t in pair}
                copied = [sh for sh in clones if sh in cache_shapes]
                if on:
                    assert not copied, copied
                else:
                    assert len(copied) == 3 * len(now), copied          # the counter sees the copying path: every cache, each read
            reads[on] = got
            if c0 == nt:
                ref = model(spec).float()
                err = rel_err(got[-3].float().cpu().numpy(), ref.cpu().numpy())
                print(f"final stream_read vs model(spec), fused={on}: {err:.3e} (bar 2e-2)")
                assert err < 2e-2
    assert len(reads[True]) == len(reads[False]) >= 3
    for a, b in zip(reads[False], reads[True]):
        assert torch.equal(a, b)
