"""A PIN of what the token-major scan / conv bindings of aum_hip tell the library: for every launch the launch name, the timer's meta
tuple and every field of the Args struct (nested `base` structs included), held against tests/golden/binding_args.json by
tests/test_binding_pin.py (CPU, lane-array library, host tensors) and tests/test_gpu_binding_pin.py (device library, the same cases).

aum_hip._launch is wrapped the way tests/stream_timeline_checks.py wraps it: the wrapper records the launch and then still performs it.
Integer and float fields are recorded as values.  A pointer field is recorded as `null`, as `<operand>+<byte offset>` when the address
lies inside the storage of a tensor the case passed in or got back (u / z are the halves of one `xz` row, B / C column blocks of one
`bc` row, the two tensors of a seq_map live in one `map` buffer), else as `internal` (workspace, carry, converted fp32 copies) -- their
byte counts are in the `*_bytes` fields next to them.  What a call returns is recorded as shapes, strides and dtypes; a refused call as the
exception's type and full message.  Nothing recorded depends on the address space: host and device runs give the same record.

The fixture is written by `python tests/binding_pin_checks.py --record` (lane-array library); `--record NAME ...` rewrites only the
named cases.  The row families (channel-major scan, per-token updates, conv, add + RMSNorm, channel-major projections: ROW_CASES) are held
the same way against tests/golden/binding_args_rows.json, written by `--record-rows [NAME ...]`.

SEG_MIN_LEN / RANGE_MIN_LEN: the shortest rows the library takes with segments=2 / range_len=8, found on the lane-array build: 1 for
both.  aum_scan_tm_seg_fwd / _seg_bwd / aum_scan_tm_fwd_state round a range up to the 8-step block and clamp every range to the row, so
at len <= 8 the second range is empty; aum_scan_tm_fwd_state_var with range_len 8 runs one range where no session is longer than 8."""
import ctypes as C
import json
import os
import sys

import torch

if __name__ == "__main__":      # run as a script (--record): the paths tests/conftest.py sets up for pytest
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio-mamba-aum_amd"))
import aum_hip

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_args.json")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SEG_MIN_LEN = 1
RANGE_MIN_LEN = 1

# (dtype, dim, T, z, D, delta_bias, delta form): every dim, T, dtype, operand presence and delta form at least twice
SCAN_CONFIGS = (("f32", 64, 1, True, True, True, "sp"), ("f32", 128, 8, False, False, False, "raw"), ("bf16", 64, 9, True, True, True, "act"),
                ("bf16", 128, 17, True, True, False, "sp"), ("bf16", 64, 8, False, False, True, "sp"), ("f32", 128, 17, True, False, True, "raw"),
                ("bf16", 128, 1, False, True, True, "raw"), ("f32", 64, 9, False, True, False, "sp"))
# (dtype, dim, T, bias, silu)
CONV_CONFIGS = (("f32", 64, 1, True, True), ("f32", 128, 8, False, False), ("bf16", 64, 9, True, False), ("bf16", 128, 17, False, True),
                ("bf16", 64, 8, True, True), ("f32", 128, 17, True, True))
# total -> (session lengths in pack order, cache rows or None, pool rows): an empty session, a permuted map, a pool with spare rows
LAYOUTS = {1: ((0, 1), (1, 0), 2), 8: ((8,), None, 1), 9: ((4, 0, 5), (3, 0, 1), 5), 17: ((9, 8), (2, 0), 4), 0: ((0, 0), (1, 0), 3)}


# ---- recording -----------------------------------------------------------------------------------------------------------------------------
def _snap(s):
    out = {}
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = _snap(v)
        elif ctype is C.c_void_p:
            out[name] = ("ptr", int(v or 0))
        else:
            out[name] = v
    return out


def _flat(prefix, v, out):
    """the tensors of a return value by name: a tensor, a tuple or a dict of them, nested"""
    if isinstance(v, torch.Tensor):
        out.append((prefix, v))
    elif isinstance(v, dict):
        for k, x in v.items():
            _flat(k if prefix == "ret" else f"{prefix}.{k}", x, out)
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            _flat(f"{prefix}{i}" if prefix == "ret" else f"{prefix}.{i}", x, out)


def _resolve(rec, spans):
    for k, v in rec.items():
        if isinstance(v, dict):
            _resolve(v, spans)
        elif isinstance(v, tuple):
            p = v[1]
            rec[k] = "null" if p == 0 else next((f"{n}+{p - lo}" for n, lo, hi in spans if lo <= p < hi), "internal")
    return rec


def run_case(fn, lib, device):
    """one case -> {"launches": [{"name", "meta", "args"}], "returns": {name: [shape, strides, dtype]}, "error": None | [type, message]}"""
    named, call = fn(lib, device)
    launches, orig = [], aum_hip._launch

    def spy(fn_, args, t, lib_, name, meta=None):
        launches.append({"name": name, "meta": None if meta is None else [int(m) if isinstance(m, bool) else m for m in meta], "args": _snap(args)})
        return orig(fn_, args, t, lib_, name, meta)

    aum_hip._launch = spy
    ret, error = None, None
    try:
        ret = call()
    except Exception as e:              # a refusal is part of the record
        error = [type(e).__name__, str(e)]
    finally:
        aum_hip._launch = orig
    got = []
    _flat("ret", ret, got)
    spans = []
    for n, t in list(named.items()) + got:
        if t is not None and t.untyped_storage().nbytes() > 0:
            lo = t.untyped_storage().data_ptr()
            spans.append((n, lo, lo + t.untyped_storage().nbytes()))
    for l in launches:
        _resolve(l["args"], spans)
    returns = {n: [list(t.shape), list(t.stride()), str(t.dtype)] for n, t in got}
    if device != "cpu":
        torch.cuda.synchronize()
    return json.loads(json.dumps({"launches": launches, "returns": returns, "error": error}))


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
class Ops(dict):
    __getattr__ = dict.__getitem__


def scan_ops(device, dt, dim, lead, z=True, D=True, bias=True, form="sp", seed=0, bc_width=48):
    """u, z the halves of one xz row, B / C column blocks 1 and 2 of a bc row of `bc_width` columns (strides differ from widths)"""
    g = torch.Generator().manual_seed(3000 + seed)
    lead = tuple(lead)
    shape = tuple(max(n, 1) for n in lead)
    cut = (lambda t: t[:lead[0]]) if len(lead) == 1 else (lambda t: t)
    xz = cut(torch.randn(*shape, 2 * dim, generator=g).to(DT[dt]).to(device))
    bc = cut(torch.randn(*shape, bc_width, generator=g).to(DT[dt]).to(device))
    raw = torch.randn(*shape, dim, generator=g) * 0.7 - 0.5
    b = torch.randn(dim, generator=g) * 0.5
    if form == "act":
        raw = torch.nn.functional.softplus(raw.double() + b.double()).float()
    elif form == "raw":
        raw, b = raw.abs() * 0.3, b.abs()
    o = Ops(dt=dt, dim=dim, lead=lead, xz=xz, u=xz[..., :dim], z=xz[..., dim:] if z else None, delta=cut(raw.to(DT[dt]).to(device)), bc=bc,
            B=bc[..., 16:32], C=bc[..., 32:48], A=(-torch.exp(torch.randn(dim, 16, generator=g) * 0.5)).to(device),
            D=torch.randn(dim, generator=g).to(device) if D else None, bias=b.to(device) if bias else None, sp=form == "sp", act=form == "act")
    o["named"] = {"xz": xz, "delta": o.delta, "bc": bc, "A": o.A, "D": o.D, "bias": o.bias}
    return o


def conv_ops(device, dt, dim, lead, bias=True, silu=True, seed=0, width=4):
    g = torch.Generator().manual_seed(4000 + seed)
    lead = tuple(lead)
    shape = tuple(max(n, 1) for n in lead)
    xz = torch.randn(*shape, 2 * dim, generator=g).to(DT[dt]).to(device)
    if len(lead) == 1:
        xz = xz[:lead[0]]
    o = Ops(dt=dt, dim=dim, lead=lead, xz=xz, x=xz[..., :dim], w=(torch.randn(dim, width, generator=g) * 0.5).to(device),
            b=torch.randn(dim, generator=g).to(device) if bias else None, silu=silu)
    o["named"] = {"xz": xz, "w": o.w, "b": o.b}
    return o


def pool(device, rows, dim, last, seed=0):
    return (torch.randn(rows, dim, last, generator=torch.Generator().manual_seed(5000 + seed)) * 0.3).to(device)


def smap(device, total, pooled=True):
    """pooled False: the training entry points have no pool, session i is sequence i"""
    lens, rows, nrows = LAYOUTS[total]
    return aum_hip.seq_map(lens, rows if pooled else None, device=device), nrows


def rand_like(t, seed):
    return torch.randn(t.shape, generator=torch.Generator().manual_seed(6000 + seed)).to(t.dtype).to(t.device)


# ---- the cases: name -> fn(lib, device) -> (named tensors, the call to record) ---------------------------------------------------------------
CASES = {}


def case(name):
    def put(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return put


def _tag(cfg):
    return "_".join(str(int(v)) if isinstance(v, bool) else str(v) for v in cfg)


def _fwd_kw(o, lib, A_b=None, want_ckpt=True):
    batch, length = o.lead
    kw = dict(D=o.D, z=o.z, delta_bias=o.bias, delta_softplus=o.sp, delta_activated=o.act, A_b=A_b, lib=lib)
    if want_ckpt:
        kw.update(want_out_pre=o.z is not None, ckpt=aum_hip.scan_tm_ckpt(batch, length, o.dim, 16, A_b is not None, o.u.device, lib=lib, dtype=DT[o.dt]))
    return kw


def _add_fixed_scan(i, cfg, batch=2, tag=None, reverse=False, bidir=False, segments=1):
    dt, dim, T, z, D, bias, form = cfg
    tag = tag or _tag(cfg)

    def ops(device):
        o = scan_ops(device, dt, dim, (batch, T), z, D, bias, form, seed=i)
        o["A_b"] = (o.A * 1.25).contiguous() if bidir else None
        o.named["A_b"] = o.A_b
        return o

    @case(f"scan_tm_fwd/{tag}")
    def _(lib, device):
        o = ops(device)
        kw = _fwd_kw(o, lib, o.A_b, want_ckpt=i % 2 == 0 or segments > 1 or bidir)
        if "ckpt" in kw:
            o.named["ckpt"] = kw["ckpt"]
        else:
            kw["out"] = o.named["out"] = torch.empty((batch, T, dim), dtype=DT[dt], device=device)
        return o.named, lambda: aum_hip.scan_tm_fwd(o.u, o.delta, o.A, o.B, o.C, reverse=reverse, segments=segments, **kw)

    @case(f"scan_tm_bwd/{tag}")
    def _(lib, device):
        o = ops(device)
        kw = _fwd_kw(o, lib, o.A_b)
        _, out_pre = aum_hip.scan_tm_fwd(o.u, o.delta, o.A, o.B, o.C, reverse=reverse, segments=segments, **kw)
        dout = rand_like(o.delta, i)
        o.named.update(ckpt=kw["ckpt"], out_pre=out_pre, dout=dout)
        return o.named, lambda: aum_hip.scan_tm_bwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, dout, out_pre, kw["ckpt"], o.sp, reverse, o.A_b,
                                                    lib=lib, segments=segments, want_dA_xA=i % 2 == 1, delta_activated=o.act)

    if reverse or bidir:
        return

    @case(f"scan_tm_fwd_state/{tag}")
    def _(lib, device):
        o = ops(device)
        st = pool(device, batch, dim, 16, i)
        st_in, st_out = ((None, None), (st, st), (st, torch.empty_like(st)), (None, st))[i % 4]
        o.named.update(state_in=st_in, state_out=st_out)
        return o.named, lambda: aum_hip.scan_tm_fwd_state(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, st_in, st_out, segments, lib=lib)

    if segments > 1:
        return

    @case(f"scan_tm_chunk/{tag}")
    def _(lib, device):
        o = ops(device)
        o.named["state"] = pool(device, batch, dim, 16, i)
        return o.named, lambda: aum_hip.scan_tm_chunk(o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, lib=lib)


def _packed_scan(device, i, cfg, pooled=True):
    dt, dim, T, z, D, bias, form = cfg
    o = scan_ops(device, dt, dim, (T,), z, D, bias, form, seed=i)
    m, nrows = smap(device, T, pooled)
    o.named.update(map=m.cu)
    return o, m, nrows


def _add_packed_scan(i, cfg):
    tag = _tag(cfg)
    dim = cfg[1]

    @case(f"scan_tm_chunk_var/{tag}")
    def _(lib, device):
        o, m, nrows = _packed_scan(device, i, cfg)
        o.named["state"] = st = pool(device, nrows, dim, 16, i)
        return o.named, lambda: aum_hip.scan_tm_chunk_var(st, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, lib=lib, peek=i % 3 == 0)

    @case(f"scan_tm_chunk_peeks/{tag}")
    def _(lib, device):
        o, m, nrows = _packed_scan(device, i, cfg)
        o.named["state"] = st = pool(device, nrows, dim, 16, i)
        o.named["out"] = out = torch.empty_like(o.delta) if i % 2 else None
        return o.named, lambda: aum_hip.scan_tm_chunk_peeks(st, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, out=out, lib=lib,
                                                            peek_every=(1, 3)[i % 2])

    @case(f"scan_tm_fwd_state_var/{tag}")
    def _(lib, device):
        o, m, nrows = _packed_scan(device, i, cfg)
        o.named["state"] = st = pool(device, nrows, dim, 16, i)
        return o.named, lambda: aum_hip.scan_tm_fwd_state_var(st, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m,
                                                              range_len=8 if i % 2 else 0, lib=lib)

    @case(f"scan_tm_peeks_fwd/{tag}")
    def _(lib, device):
        o, m, _ = _packed_scan(device, i, cfg, pooled=False)
        return o.named, lambda: aum_hip.scan_tm_peeks_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, peek_every=(2, 1)[i % 2], lib=lib)

    @case(f"scan_tm_peeks_bwd/{tag}")
    def _(lib, device):
        o, m, _ = _packed_scan(device, i, cfg, pooled=False)
        P = (2, 1)[i % 2]
        _, ckpt = aum_hip.scan_tm_peeks_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, peek_every=P, lib=lib)
        dout = rand_like(o.delta, i)
        o.named.update(ckpt=ckpt, dout=dout)
        return o.named, lambda: aum_hip.scan_tm_peeks_bwd_parts(dout, ckpt, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m,
                                                                peek_every=P, lib=lib)


def _add_conv(i, cfg):
    dt, dim, T, bias, silu = cfg
    tag = _tag(cfg)

    def packed(device, pooled=True):
        o = conv_ops(device, dt, dim, (T,), bias, silu, seed=i)
        m, nrows = smap(device, T, pooled)
        o.named.update(map=m.cu, pool=pool(device, nrows, dim, 4, i))
        if i == 2:          # the weight as the module holds it, and as a misaligned view: it gets its own storage
            wide = torch.zeros(dim * 4 + 1, device=device)
            wide[1:] = o.w.reshape(-1)
            o["w"] = o.named["w"] = wide[1:].view(dim, 1, 4)
        return o, m

    @case(f"conv1d_tm_chunk/{tag}")
    def _(lib, device):
        o = conv_ops(device, dt, dim, (2, T), bias, silu, seed=i)
        o.named["pool"] = cs = pool(device, 2, dim, 4, i)
        return o.named, lambda: aum_hip.conv1d_tm_chunk(o.x, cs, o.w, o.b, o.silu, lib=lib)

    @case(f"conv1d_tm_chunk_var/{tag}")
    def _(lib, device):
        o, m = packed(device)
        return o.named, lambda: aum_hip.conv1d_tm_chunk_var(o.x, o.named["pool"], o.w, o.b, o.silu, seq_map=m, lib=lib, peek=i % 3 == 0)

    @case(f"conv1d_tm_chunk_peeks/{tag}")
    def _(lib, device):
        o, m = packed(device)
        o.named["out"] = out = torch.empty((T, dim), dtype=DT[dt], device=device) if i % 2 else None
        return o.named, lambda: aum_hip.conv1d_tm_chunk_peeks(o.x, o.named["pool"], o.w, o.b, o.silu, seq_map=m, out=out, lib=lib, peek_every=(1, 3)[i % 2])

    @case(f"conv1d_tm_prefill_var/{tag}")
    def _(lib, device):
        o, m = packed(device)
        return o.named, lambda: aum_hip.conv1d_tm_prefill_var(o.x, o.named["pool"], o.w, o.b, o.silu, seq_map=m, lib=lib)

    @case(f"conv1d_tm_peeks_bwd/{tag}")
    def _(lib, device):
        o, m = packed(device, pooled=False)
        o.named["dy"] = dy = rand_like(o.x, i)
        return o.named, lambda: aum_hip.conv1d_tm_peeks_bwd_parts(dy, o.x, o.w, o.b, o.silu, seq_map=m, peek_every=(2, 1)[i % 2], lib=lib)


for _i, _cfg in enumerate(SCAN_CONFIGS):
    _add_fixed_scan(_i, _cfg)
    _add_packed_scan(_i, _cfg)
for _i, _cfg in enumerate(CONV_CONFIGS):
    _add_conv(_i, _cfg)
# the offline pair: batch 1 (the batch stride of a size-1 axis is normalised), reversed time, both directions, two time segments
_add_fixed_scan(10, ("bf16", 64, 9, True, True, True, "sp"), batch=1, tag="batch1")
_add_fixed_scan(11, ("f32", 64, 9, True, True, True, "sp"), tag="reverse_f32", reverse=True)
_add_fixed_scan(12, ("bf16", 128, 8, False, True, False, "raw"), tag="reverse_bf16", reverse=True)
_add_fixed_scan(13, ("f32", 128, 17, True, True, True, "sp"), tag="bidir_f32", bidir=True)
_add_fixed_scan(14, ("bf16", 64, 8, True, False, True, "act"), tag="bidir_bf16", bidir=True)
_add_fixed_scan(15, ("bf16", 64, SEG_MIN_LEN, True, True, True, "sp"), tag="segments2_min", segments=2)
_add_fixed_scan(16, ("f32", 128, 17, False, True, True, "raw"), tag="segments2", segments=2)
_add_fixed_scan(17, ("bf16", 64, 17, True, True, True, "sp"), tag="segments2_bidir", segments=2, bidir=True)


@case("scan_tm_fwd_state_var/range8_min")
def _(lib, device):
    o, m, nrows = _packed_scan(device, 20, ("bf16", 64, RANGE_MIN_LEN, True, True, True, "sp"))
    o.named["state"] = st = pool(device, nrows, 64, 16, 20)
    return o.named, lambda: aum_hip.scan_tm_fwd_state_var(st, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, range_len=8, lib=lib)


# ---- the all-empty pack: every packed wrapper returns before it looks at anything else ---------------------------------------------------
def _add_empty():
    def scan(fn, **kw):
        def run(lib, device):
            o, m, nrows = _packed_scan(device, 30, ("bf16", 64, 0, True, True, True, "sp"))
            o.named["state"] = st = pool(device, nrows, 64, 16, 30)
            return o.named, lambda: getattr(aum_hip, fn)(st, o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, lib=lib, **kw)
        CASES[f"{fn}/all_empty"] = run

    def conv(fn, **kw):
        def run(lib, device):
            o = conv_ops(device, "bf16", 64, (0,), seed=30)
            m, nrows = smap(device, 0)
            o.named.update(map=m.cu, pool=pool(device, nrows, 64, 4, 30))
            return o.named, lambda: getattr(aum_hip, fn)(o.x, o.named["pool"], o.w, o.b, o.silu, seq_map=m, lib=lib, **kw)
        CASES[f"{fn}/all_empty"] = run

    scan("scan_tm_chunk_var")
    scan("scan_tm_chunk_peeks", peek_every=2)
    scan("scan_tm_fwd_state_var")
    conv("conv1d_tm_chunk_var")
    conv("conv1d_tm_chunk_peeks", peek_every=2)
    conv("conv1d_tm_prefill_var")


_add_empty()


# ---- refusals: one per clause of the operand rule and entry point that states it (a Python message, or the library's code) ---------------
def _breaks():
    """clause -> (scan_ops keywords, what to do to the operands afterwards)"""
    def wrong_dtype(o):
        o["delta"] = o.named["delta"] = o.delta.float()

    def misaligned(o):                  # u one element into the row: the row is no longer 16-byte aligned
        o["u"] = o.xz[..., 1:o.dim + 1]

    def odd_bc(o):                      # B / C rows of an odd stride at 16 bits
        pass

    return {"wrong_dtype": (dict(dt="bf16"), wrong_dtype), "misaligned_row": (dict(dt="f32"), misaligned),
            "odd_bc_stride": (dict(dt="bf16", bc_width=49), odd_bc), "activated_fp32": (dict(dt="f32", form="act"), lambda o: None)}


def _add_refusals():
    for clause, (kw, brk) in _breaks().items():
        # the chunk kernels read rows element by element: of the four clauses they state only the dtype one, the rest they TAKE
        verb = lambda name, clause=clause: "takes" if name in ("scan_tm_chunk", "scan_tm_chunk_var") and clause != "wrong_dtype" else "refuse"

        def ops(device, lead, kw=kw, brk=brk):
            o = scan_ops(device, kw.get("dt", "bf16"), 64, lead, True, True, True, kw.get("form", "sp"), seed=40, bc_width=kw.get("bc_width", 48))
            brk(o)
            return o

        def fixed(name, call, ops=ops):
            def run(lib, device):
                o = ops(device, (2, 9))
                o.named["state"] = pool(device, 2, 64, 16, 40)
                return o.named, lambda: call(o, lib)
            CASES[f"{name}/{verb(name)}_{clause}"] = run

        def packed(name, call, ops=ops):
            def run(lib, device):
                o = ops(device, (9,))
                m, nrows = smap(device, 9, pooled=name != "scan_tm_peeks_fwd")
                o.named.update(map=m.cu, state=pool(device, nrows, 64, 16, 40))
                return o.named, lambda: call(o, m, lib)
            CASES[f"{name}/{verb(name)}_{clause}"] = run

        fixed("scan_tm_fwd", lambda o, lib: aum_hip.scan_tm_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, delta_activated=o.act, lib=lib))
        fixed("scan_tm_fwd_state", lambda o, lib: aum_hip.scan_tm_fwd_state(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, o.named["state"],
                                                                            o.named["state"], lib=lib))
        fixed("scan_tm_chunk", lambda o, lib: aum_hip.scan_tm_chunk(o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, lib=lib))
        packed("scan_tm_chunk_var", lambda o, m, lib: aum_hip.scan_tm_chunk_var(o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act,
                                                                               seq_map=m, lib=lib))
        packed("scan_tm_fwd_state_var", lambda o, m, lib: aum_hip.scan_tm_fwd_state_var(o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp,
                                                                                       o.act, seq_map=m, lib=lib))
        if clause == "wrong_dtype":
            def bwd(lib, device, ops=ops):
                o = ops(device, (2, 9))
                ckpt = aum_hip.scan_tm_ckpt(2, 9, 64, 16, False, device, lib=lib, dtype=torch.bfloat16)
                return o.named, lambda: aum_hip.scan_tm_bwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, rand_like(o.u, 1), rand_like(o.u, 2), ckpt, o.sp,
                                                            lib=lib)
            CASES["scan_tm_bwd/refuse_wrong_dtype"] = bwd
            packed("scan_tm_peeks_fwd", lambda o, m, lib: aum_hip.scan_tm_peeks_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m,
                                                                                   peek_every=2, lib=lib))

    def scan_state(name, fixed, shape, call):
        def run(lib, device):
            o = scan_ops(device, "bf16", 64, (2, 9) if fixed else (9,), seed=41)
            m = None if fixed else smap(device, 9)[0]
            o.named["state"] = torch.zeros(shape, device=device)
            if m is not None:
                o.named["map"] = m.cu
            return o.named, lambda: call(o, m, lib)
        CASES[f"{name}/refuse_state_shape"] = run

    scan_state("scan_tm_fwd_state", True, (2, 16, 64), lambda o, m, lib: aum_hip.scan_tm_fwd_state(
        o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, o.named["state"], None, lib=lib))
    scan_state("scan_tm_chunk", True, (3, 64, 16), lambda o, m, lib: aum_hip.scan_tm_chunk(
        o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, lib=lib))
    scan_state("scan_tm_chunk_var", False, (5, 64, 8), lambda o, m, lib: aum_hip.scan_tm_chunk_var(
        o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, lib=lib))
    scan_state("scan_tm_fwd_state_var", False, (5, 16, 64), lambda o, m, lib: aum_hip.scan_tm_fwd_state_var(
        o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, lib=lib))

    # a map of another length, under every packed wrapper's own name; a map that names a row the pool does not have
    def scan_map(fn, total=17, rows=5, **kw):
        def run(lib, device):
            o = scan_ops(device, "bf16", 64, (9,), seed=42)
            m = smap(device, total)[0]
            o.named.update(map=m.cu, state=pool(device, rows, 64, 16, 42))
            return o.named, lambda: getattr(aum_hip, fn)(o.named["state"], o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, lib=lib, **kw)
        CASES[f"{fn}/refuse_map_{'length' if total != 9 else 'row'}"] = run

    def conv_map(fn, **kw):
        def run(lib, device):
            o = conv_ops(device, "bf16", 64, (9,), seed=42)
            m = smap(device, 17)[0]
            o.named.update(map=m.cu, pool=pool(device, 5, 64, 4, 42))
            return o.named, lambda: getattr(aum_hip, fn)(o.x, o.named["pool"], o.w, o.b, o.silu, seq_map=m, lib=lib, **kw)
        CASES[f"{fn}/refuse_map_length"] = run

    scan_map("scan_tm_chunk_var")
    scan_map("scan_tm_chunk_peeks", peek_every=2)
    scan_map("scan_tm_fwd_state_var")
    scan_map("scan_tm_chunk_var", total=9, rows=2)
    conv_map("conv1d_tm_chunk_var")
    conv_map("conv1d_tm_chunk_peeks", peek_every=2)
    conv_map("conv1d_tm_prefill_var")

    def peeks_map(lib, device):
        o = scan_ops(device, "bf16", 64, (9,), seed=42)
        m = smap(device, 17, pooled=False)[0]
        return o.named, lambda: aum_hip.scan_tm_peeks_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, o.act, seq_map=m, peek_every=2, lib=lib)
    CASES["scan_tm_peeks_fwd/refuse_map_length"] = peeks_map

    # the conv family: a row that is not 16-byte aligned, a pool of another width than the weight, a 16-bit pool
    def conv_bad(fn, clause, packed, **kw):
        def run(lib, device):
            o = conv_ops(device, "f32" if clause == "misaligned_row" else "bf16", 64, (9,) if packed else (2, 9), seed=43)
            m, nrows = smap(device, 9)
            cs = pool(device, nrows if packed else 2, 64, 3 if clause == "pool_width" else 4, 43)
            if clause == "misaligned_row":
                o["x"] = o.xz[..., 1:65]
            if clause == "pool_dtype":
                cs = cs.to(torch.bfloat16)
            o.named.update(map=m.cu, pool=cs)
            if packed:
                kw["seq_map"] = m
            return o.named, lambda: getattr(aum_hip, fn)(o.x, cs, o.w, o.b, o.silu, lib=lib, **kw)
        CASES[f"{fn}/refuse_{clause}"] = run

    for clause in ("misaligned_row", "pool_width", "pool_dtype"):
        conv_bad("conv1d_tm_chunk", clause, False)
        conv_bad("conv1d_tm_chunk_var", clause, True)
        conv_bad("conv1d_tm_prefill_var", clause, True)
    conv_bad("conv1d_tm_chunk_peeks", "misaligned_row", True, peek_every=2)

    # the checkpoint of the offline pair: too small, and not fp32
    def ckpt_bad(fn, small):
        def run(lib, device):
            o = scan_ops(device, "bf16", 64, (2, 9), seed=44)
            ckpt = aum_hip.scan_tm_ckpt(2, 9, 64, 16, False, device, lib=lib, dtype=torch.bfloat16)
            ckpt = ckpt.reshape(-1)[1:] if small else ckpt.double()
            o.named["ckpt"] = ckpt
            if fn == "scan_tm_fwd":
                return o.named, lambda: aum_hip.scan_tm_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.sp, want_out_pre=True, ckpt=ckpt, lib=lib)
            return o.named, lambda: aum_hip.scan_tm_bwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, rand_like(o.delta, 1), rand_like(o.delta, 2), ckpt,
                                                        o.sp, lib=lib)
        CASES[f"{fn}/refuse_ckpt_{'small' if small else 'dtype'}"] = run

    for fn in ("scan_tm_fwd", "scan_tm_bwd"):
        ckpt_bad(fn, True)
        ckpt_bad(fn, False)


_add_refusals()
GROUPS = sorted({n.split("/")[0] for n in CASES})


# ==== the row families -> tests/golden/binding_args_rows.json: channel-major scan, per-token updates, conv (token- and channel-major), ====
# ==== add + RMSNorm, channel-major projections.  Recorded on the lane-array build, which has every one of their entry points          ====
ROWS_FIXTURE = os.path.join(os.path.dirname(FIXTURE), "binding_args_rows.json")
ROW_CASES = {}
# calls whose operand is of another type, shape or device than the kernel is told: host tensors only (every such operand is LARGER than
# what the kernel reads, so the lane-array run stays in bounds where a binding launches it); a device run could fault, so there is none
ROW_HOST_ONLY = set()
DT16 = dict(DT, f16=torch.float16)


def row_case(name, host_only=False):
    def put(fn):
        assert name not in ROW_CASES, name
        ROW_CASES[name] = fn
        if host_only:
            ROW_HOST_ONLY.add(name)
        return fn
    return put


def _randn(device, dt, *shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(7000 + seed)) * scale).to(DT16[dt]).to(device)


# ---- channel-major scan: u / z the halves of one (batch, 2 dim, len) xz tensor, B / C (batch, 1, 16, len) or (batch, 16, len) ---------------
def scan_cm_ops(device, dt, dim, length, z=True, D=True, bias=True, bc4=False, bidir=False, seed=0, batch=2):
    xz = _randn(device, dt, batch, 2 * dim, length, seed=seed)
    bc = _randn(device, dt, 2, batch, 1, 16, length, seed=seed + 100)
    g = torch.Generator().manual_seed(7500 + seed)
    A = (-torch.exp(torch.randn(dim, 16, generator=g) * 0.5)).to(device)
    o = Ops(dt=dt, dim=dim, batch=batch, length=length, xz=xz, u=xz[:, :dim], z=xz[:, dim:] if z else None,
            delta=_randn(device, dt, batch, dim, length, seed=seed + 200, scale=0.3).abs(), bc=bc,
            B=bc[0] if bc4 else bc[0, :, 0], C=bc[1] if bc4 else bc[1, :, 0], A=A, A_b=(A * 1.25).contiguous() if bidir else None,
            D=torch.randn(dim, generator=g).to(device) if D else None, bias=(torch.randn(dim, generator=g) * 0.5).to(device) if bias else None)
    o["named"] = {"xz": xz, "delta": o.delta, "bc": bc, "A": A, "A_b": o.A_b, "D": o.D, "bias": o.bias}
    return o


# (tag, dtype, dim, len, z, D, delta_bias, delta_softplus, the rest): len 1 / 9 plain rows, 513 the lane checkpoint, 1025 the chunk checkpoint
SCAN_CM_CONFIGS = (
    ("plain_f32", "f32", 64, 1, True, True, True, True, dict(bc4=True)),
    ("bare_bf16", "bf16", 128, 9, False, False, False, False, {}),
    ("reverse_f32", "f32", 128, 9, True, True, False, True, dict(reverse=True)),
    ("bidir_bf16", "bf16", 64, 9, True, True, True, True, dict(bidir=True, bc4=True)),
    ("dmajor", "bf16", 64, 9, True, False, True, False, dict(dmajor=True)),
    ("generic", "f32", 64, 9, True, True, True, True, dict(generic=True)),
    ("rowpair", "bf16", 128, 9, True, True, True, True, dict(rowpair=True)),
    ("last_state_dz_view", "f32", 64, 9, True, True, True, True, dict(want_last_state=True, dz_view=True)),
    ("lane_bidir", "bf16", 64, 513, True, True, True, True, dict(bidir=True, lane=True)),
    ("lane_f32", "f32", 64, 513, False, True, True, True, dict(lane=True)),
    ("chunk_ck", "bf16", 64, 1025, True, True, True, True, dict(ck=True)),
    ("chunk_acc", "bf16", 64, 1025, True, True, True, True, dict(ck=True, acc=True)),
    ("chunk_f32", "f32", 128, 1025, False, False, True, False, {}),
    ("len1_bf16", "bf16", 128, 1, True, True, True, True, {}))


def _add_scan_cm(i, cfg):
    tag, dt, dim, length, z, D, bias, sp, x = cfg
    bidir, lane, ck, acc = x.get("bidir", False), x.get("lane", False), x.get("ck", False), x.get("acc", False)
    flags = {k: x[k] for k in ("dmajor", "generic", "rowpair") if k in x}

    def ops(device, lib):
        o = scan_cm_ops(device, dt, dim, length, z, D, bias, x.get("bc4", False), bidir, seed=i)
        o["x_ck"] = aum_hip.scan_ckpt(o.u, 16, lib=lib) if ck else None
        o["x_lane"] = aum_hip.scan_lane_ckpt(o.u, 16, bidir, lib=lib) if lane else None
        assert (o.x_ck is not None) == ck and (o.x_lane is not None) == lane
        o["A_rev"] = (o.A * 1.25).contiguous() if acc else None    # the reverse direction's A of a two-launch Fo-Bi pair
        o.named.update(x_ck=o.x_ck, x_lane=o.x_lane, A_rev=o.A_rev)
        return o

    def fwd(o, lib, reverse, A, x_ck, **kw):
        return aum_hip.scan_fwd(o.u, o.delta, A, o.B, o.C, o.D, o.z, o.bias, sp, reverse, o.A_b, want_out_pre=z, x_ck=x_ck, x_lane=o.x_lane,
                                lib=lib, **flags, **kw)

    def bwd(o, lib, reverse, A, x_ck, dout, out_pre, **kw):
        return aum_hip.scan_bwd(o.u, o.delta, A, o.B, o.C, o.D, o.z, o.bias, dout, out_pre, sp, reverse, o.A_b, x_ck=x_ck, x_lane=o.x_lane,
                                lib=lib, **flags, **kw)

    @row_case(f"scan_fwd/{tag}")
    def _(lib, device):
        o = ops(device, lib)
        if not acc:
            return o.named, lambda: fwd(o, lib, x.get("reverse", False), o.A, o.x_ck, want_last_state=x.get("want_last_state", False))
        o.named["out"] = fwd(o, lib, False, o.A, None)[0]           # the other direction's output: the reverse launch adds to it
        return o.named, lambda: fwd(o, lib, True, o.A_rev, o.x_ck, accumulate_into=o.named["out"])

    @row_case(f"scan_bwd/{tag}")
    def _(lib, device):
        o = ops(device, lib)
        dout = rand_like(o.delta, i)
        o.named["dout"] = dout
        if not acc:
            o.named["out_pre"] = out_pre = fwd(o, lib, x.get("reverse", False), o.A, o.x_ck)[1]
            kw = {}
            if x.get("dz_view"):                                    # dz as the second half of a d(xz) tensor
                o.named["dxz"] = torch.empty_like(o.xz)
                kw["dz_out"] = o.named["dxz"][:, dim:]
            return o.named, lambda: bwd(o, lib, x.get("reverse", False), o.A, o.x_ck, dout, out_pre, **kw)
        g = bwd(o, lib, False, o.A, None, dout, fwd(o, lib, False, o.A, None)[1])
        o.named["out_pre"] = out_pre = fwd(o, lib, True, o.A_rev, o.x_ck)[1]
        o.named.update({f"acc.{k}": v for k, v in g.items()})
        return o.named, lambda: bwd(o, lib, True, o.A_rev, o.x_ck, dout, out_pre, accumulate_into=g)


for _i, _cfg in enumerate(SCAN_CM_CONFIGS):
    _add_scan_cm(_i, _cfg)


def _add_scan_ckpt_shapes():
    """what scan_ckpt / scan_lane_ckpt / scan_accumulates hand out per length: a tensor's shape is recorded, None (or False) leaves no entry"""
    for length in (1, 9, 513, 1025):
        def run(lib, device, length=length):
            u = torch.empty((2, 64, length), dtype=torch.bfloat16, device=device)
            return {}, lambda: {"scan_ckpt": aum_hip.scan_ckpt(u, 16, lib=lib), "scan_lane_ckpt": aum_hip.scan_lane_ckpt(u, 16, False, lib=lib),
                                "scan_lane_ckpt_bidir": aum_hip.scan_lane_ckpt(u, 16, True, lib=lib),
                                "scan_accumulates": torch.empty((), device=device) if aum_hip.scan_accumulates(u, 16, lib=lib) else None}
        ROW_CASES[f"scan_ckpt/len{length}"] = run


_add_scan_ckpt_shapes()


# ---- one token: state_update / conv1d_update ------------------------------------------------------------------------------------------------
def _add_updates():
    # (dtype, z, D, dt_bias, dt_softplus)
    for i, (dt, z, D, bias, sp) in enumerate((("f32", True, True, True, True), ("bf16", False, False, False, False), ("bf16", True, True, True, True),
                                              ("f32", False, True, False, True))):
        @row_case(f"state_update/{_tag((dt, z, D, bias, sp))}")
        def _(lib, device, i=i, dt=dt, z=z, D=D, bias=bias, sp=sp):
            named = {"state": pool(device, 2, 64, 16, i), "x": _randn(device, dt, 2, 64, seed=i), "dt": _randn(device, dt, 2, 64, seed=i + 1, scale=0.3),
                     "A": -torch.rand(64, 16).to(device), "B": _randn(device, dt, 2, 16, seed=i + 2), "C": _randn(device, dt, 2, 16, seed=i + 3),
                     "D": torch.ones(64, device=device) if D else None, "z": _randn(device, dt, 2, 64, seed=i + 4) if z else None,
                     "dt_bias": torch.zeros(64, device=device) if bias else None}
            n = Ops(named)
            return named, lambda: aum_hip.state_update(n.state, n.x, n.dt, n.A, n.B, n.C, n.D, n.z, n.dt_bias, sp, lib=lib)

    for i, (dt, bias, silu) in enumerate((("f32", True, True), ("bf16", False, False), ("bf16", True, True))):
        @row_case(f"conv1d_update/{_tag((dt, bias, silu))}")
        def _(lib, device, i=i, dt=dt, bias=bias, silu=silu):
            named = {"x": _randn(device, dt, 2, 64, seed=i), "conv_state": pool(device, 2, 64, 4, i), "w": _randn(device, "f32", 64, 1, 4, seed=i + 1),
                     "b": _randn(device, "f32", 64, seed=i + 2) if bias else None}
            n = Ops(named)
            return named, lambda: aum_hip.conv1d_update(n.x, n.conv_state, n.w, n.b, silu, lib=lib)


_add_updates()


# ---- conv: token-major (batch, len, dim) and channel-major (batch, dim, len), x the first half of an xz tensor or a tensor of its own ----------
# (dtype, dim, len, width, bias, silu, reverse, the rest)
CONV_ROW_CONFIGS = (("f32", 64, 1, 4, True, True, False, dict(own=True)), ("bf16", 128, 3, 4, False, False, False, {}),
                    ("bf16", 64, 9, 4, True, True, True, {}), ("f32", 128, 9, 2, True, False, False, {}),
                    ("bf16", 128, 9, 4, True, True, False, dict(dx_view=True, partials=True, own=True)), ("f32", 64, 3, 4, False, True, True, {}),
                    ("bf16", 64, 9, 4, True, False, False, dict(dmajor=True, generic=True, dx_view=True)))


def _conv_row_ops(device, cfg, i, tm):
    dt, dim, T, width, bias, silu, rev, x = cfg
    o = conv_ops(device, dt, dim, (2, T), bias, silu, seed=50 + i, width=width)
    if not tm:                          # the same numbers as (batch, 2 dim, len)
        o["xz"] = o.named["xz"] = o.xz.transpose(1, 2).contiguous()
        o["x"] = o.xz[:, :dim]
    if x.get("own"):
        o["x"] = o.named["x"] = o.x.contiguous()
    o.named["dy"] = o["dy"] = rand_like(o.x.contiguous(), i)
    o["dx_out"] = None
    if x.get("dx_view"):                # dx as the first half of a d(xz) tensor
        o.named["dxz"] = torch.empty_like(o.xz)
        o["dx_out"] = o.named["dxz"][..., :dim] if tm else o.named["dxz"][:, :dim]
    return o


def _add_conv_rows(i, cfg):
    dt, dim, T, width, bias, silu, rev, x = cfg
    tag = _tag(cfg[:7]) + "".join(f"_{k}" for k in x)
    gen = {"generic": True} if x.get("generic") else {}

    if not x.get("dmajor"):
        @row_case(f"conv1d_tm_fwd/{tag}")
        def _(lib, device):
            o = _conv_row_ops(device, cfg, i, True)
            return o.named, lambda: aum_hip.conv1d_tm_fwd(o.x, o.w, o.b, silu, rev, lib=lib)

        @row_case(f"conv1d_tm_bwd/{tag}")
        def _(lib, device):
            o = _conv_row_ops(device, cfg, i, True)
            return o.named, lambda: aum_hip.conv1d_tm_bwd(o.x, o.w, o.b, o.dy, silu, rev, dx_out=o.dx_out, lib=lib, partials=x.get("partials", False))

    @row_case(f"conv1d_fwd/{tag}")
    def _(lib, device):
        o = _conv_row_ops(device, cfg, i, False)
        return o.named, lambda: aum_hip.conv1d_fwd(o.x, o.w, o.b, silu, rev, dmajor=x.get("dmajor", False), lib=lib, **gen)

    @row_case(f"conv1d_bwd/{tag}")
    def _(lib, device):
        o = _conv_row_ops(device, cfg, i, False)
        return o.named, lambda: aum_hip.conv1d_bwd(o.x, o.w, o.b, o.dy, silu, rev, dx_out=o.dx_out, lib=lib, **gen)


for _i, _cfg in enumerate(CONV_ROW_CONFIGS):
    _add_conv_rows(_i, _cfg)


def _prefill_ops(device, dt, T, width=4, pool_width=4, seed=0):
    o = conv_ops(device, dt, 64, (2, T), seed=60 + seed, width=width)
    o.named["conv_state"] = o["cs"] = pool(device, 2, 64, pool_width, seed)
    return o


for _dt, _T in (("bf16", 1), ("f32", 3), ("bf16", 9)):          # T < width: the window shifts; T >= width: it is replaced
    def _prefill(lib, device, dt=_dt, T=_T):
        o = _prefill_ops(device, dt, T, seed=T)
        return o.named, lambda: aum_hip.conv1d_tm_prefill(o.x, o.cs, o.w, o.b, o.silu, lib=lib)
    ROW_CASES[f"conv1d_tm_prefill/{_dt}_T{_T}"] = _prefill


# ---- add + RMSNorm --------------------------------------------------------------------------------------------------------------------------
# (rows, cols, x dtype, residual: None | its dtype, the rest): residual_f32 = residual_dtype=torch.float32 without a residual; x_view = x the
# first half of wider rows; bwd: dres = dresidual given, dw_out given; drop = (rows_per_scale,) -> the drop pair instead of the plain one
NORM_CONFIGS = (
    (1, 64, "f32", None, {}),
    (9, 768, "bf16", "bf16", dict(dres=True)),
    (18, 64, "bf16", "f32", dict(dw_out=True)),
    (9, 64, "bf16", None, dict(residual_f32=True)),
    (18, 768, "f32", "f32", dict(x_view=True, dres=True)),
    (9, 4096, "bf16", "bf16", {}),                          # the non-vector kernels: one partial row per grid row
    (9, 64, "bf16", "bf16", dict(generic=True)),
    (1, 768, "bf16", "f32", {}),
    (9, 64, "bf16", "bf16", dict(drop=1, dres=True)),
    (18, 768, "bf16", "f32", dict(drop=9, dw_out=True)),
    (9, 64, "f32", "f32", dict(drop=9, x_view=True)),
    (18, 4096, "bf16", "bf16", dict(drop=1, generic=True)))
ROW_SCALES = (0.0, 1.0, 1.0 / 0.9)


def _add_norm(i, cfg):
    rows, cols, dt, res, x = cfg
    drop, generic = x.get("drop"), x.get("generic", False)
    tag = _tag(cfg[:3]) + f"_{res}" + "".join(f"_{k}" if v is True else f"_{k}{v}" for k, v in x.items())

    def ops(device):
        wide = _randn(device, dt, rows, 2 * cols if x.get("x_view") else cols, seed=70 + i)
        named = {"x": wide, "w": _randn(device, "f32", cols, seed=71 + i), "residual": None if res is None else _randn(device, res, rows, cols, seed=72 + i)}
        o = Ops(x=wide[:, :cols], w=named["w"], residual=named["residual"], named=named)
        if drop:
            o["scale"] = named["row_scale"] = torch.tensor([ROW_SCALES[(k + i) % 3] for k in range(rows // drop)], dtype=torch.float32, device=device)
        return o

    def fwd(o, lib):
        if drop:
            return aum_hip.rmsnorm_drop_fwd(o.x, o.w, o.residual, o.scale, drop, 1e-5, generic=generic, lib=lib)
        return aum_hip.rmsnorm_fwd(o.x, o.w, o.residual, 1e-5, residual_dtype=torch.float32 if x.get("residual_f32") else None, generic=generic, lib=lib)

    pair = "rmsnorm_drop" if drop else "rmsnorm"

    @row_case(f"{pair}_fwd/{tag}")
    def _(lib, device):
        o = ops(device)
        return o.named, lambda: fwd(o, lib)

    @row_case(f"{pair}_bwd/{tag}")
    def _(lib, device):
        o = ops(device)
        _, rstd, saved = fwd(o, lib)
        o.named.update(x_saved=saved, rstd=rstd, dy=rand_like(o.x.contiguous(), i))
        dres = o.named["dresidual"] = rand_like(saved, i + 1) if x.get("dres") else None
        dw_out = o.named["dw_out"] = torch.empty(cols, device=device) if x.get("dw_out") else None
        kw = dict(x_dtype=DT[dt], generic=generic, lib=lib, dw_out=dw_out)

        def call():                     # the partial rows handed to sum_rows are part of the record: their count is the kernel's
            seen, orig = {}, aum_hip.sum_rows
            aum_hip.sum_rows = lambda t, *a, **k: (seen.update(dweight_partial=t), orig(t, *a, **k))[1]
            try:
                if drop:
                    ret = aum_hip.rmsnorm_drop_bwd(o.named["dy"], saved, o.w, rstd, o.scale, drop, dres, **kw)
                else:
                    ret = aum_hip.rmsnorm_bwd(o.named["dy"], saved, o.w, rstd, dres, res is not None, **kw)
            finally:
                aum_hip.sum_rows = orig
            return dict(seen, dx=ret[0], dw=ret[1], dres_in=ret[2])
        return o.named, call


for _i, _cfg in enumerate(NORM_CONFIGS):
    _add_norm(_i, _cfg)


# ---- channel-major projections ----------------------------------------------------------------------------------------------------------------
# (dtype, ntok, dt_rank, transpose_out): dstate 16, dim 64.  dt_rank 48 and 24 do NOT reach _pad_cols8's padding branch (48, 24, 80 and 56
# columns are multiples of 8); dt_rank 20 does (w_dt 20 -> 24, w_x_t 52 -> 56).  aum_proj_bwd_weight_splits gives 1 split up to 128 tokens,
# 2 at 256
PROJ_CONFIGS = (("bf16", 64, 48, False), ("f16", 128, 24, True), ("bf16", 128, 24, False), ("f16", 64, 48, True), ("bf16", 256, 20, True))


def _add_proj(i, cfg):
    dt, ntok, rank, tr = cfg
    tag, rt = _tag(cfg), rank + 32

    @row_case(f"proj_fwd/{tag}")
    def _(lib, device):
        named = {"act": _randn(device, dt, 64, ntok, seed=80 + i), "w_x": _randn(device, dt, rt, 64, seed=81 + i), "w_dt": _randn(device, dt, 64, rank, seed=82 + i)}
        return named, lambda: aum_hip.proj_fwd(named["act"], named["w_x"], named["w_dt"], 16, lib=lib)

    @row_case(f"proj_bwd_data/{tag}")
    def _(lib, device):
        named = {"ddelta": _randn(device, dt, 64, ntok, seed=83 + i), "w_dt_t": _randn(device, dt, rank, 64, seed=84 + i),
                 "w_x_t": _randn(device, dt, 64, rt, seed=85 + i), "dB": _randn(device, "f32", 2, 16, ntok // 2, seed=86 + i),
                 "dC": _randn(device, "f32", 2, 16, ntok // 2, seed=87 + i), "dconv": _randn(device, dt, 64, ntok, seed=88 + i)}
        n = Ops(named)
        return named, lambda: aum_hip.proj_bwd_data(n.ddelta, n.w_dt_t, n.w_x_t, n.dB, n.dC, n.dconv, ntok // 2, lib=lib)

    @row_case(f"proj_bwd_weight/{tag}")
    def _(lib, device):
        named = {"x": _randn(device, dt, 64, ntok, seed=89 + i), "y": _randn(device, dt, rt, ntok, seed=90 + i)}
        return named, lambda: aum_hip.proj_bwd_weight(named["x"], named["y"], tr, lib=lib)


for _i, _cfg in enumerate(PROJ_CONFIGS):
    _add_proj(_i, _cfg)


# ---- refusals the families state, and the calls they took although an operand was of another type, shape or device (ROW_HOST_ONLY) -----------
def _add_row_refusals():
    def scan(name, brk, bwd=False, host_only=False, length=9):
        @row_case(f"{'scan_bwd' if bwd else 'scan_fwd'}/{name}", host_only)
        def _(lib, device):
            o = scan_cm_ops(device, "bf16", 64, length, seed=95)
            o.update(dout=rand_like(o.delta, 1), out_pre=rand_like(o.delta, 2), kw={})
            o.named.update(dout=o.dout, out_pre=o.out_pre)
            brk(o)
            if bwd:
                return o.named, lambda: aum_hip.scan_bwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, o.dout, o.out_pre, True, lib=lib, **o.kw)
            return o.named, lambda: aum_hip.scan_fwd(o.u, o.delta, o.A, o.B, o.C, o.D, o.z, o.bias, True, lib=lib, **o.kw)

    def put(key, make, also=None):
        def brk(o):
            o[key] = make(o)
            if also:
                o.named[also] = o[key]
        return brk

    longer = lambda t: torch.cat([t, t[..., :1]], -1)           # one more step: every row the kernel reads is inside it
    for bwd in (False, True):
        scan("refuse_time_stride", put("delta", lambda o: o.delta.transpose(1, 2).contiguous().transpose(1, 2)), bwd)
        scan("refuse_two_bc_groups", put("B", lambda o: torch.cat([o.bc[0], o.bc[0]], 1)), bwd)
    scan("refuse_mixed_dtypes", put("delta", lambda o: o.delta.float(), "delta"))
    scan("refuse_shape", put("B", lambda o: longer(o.B), "B"))
    scan("takes_mixed_dtypes", put("delta", lambda o: o.delta.float(), "delta"), True, True)
    scan("takes_shape", put("B", lambda o: longer(o.B), "B"), True, True)
    scan("takes_dout_dtype", put("dout", lambda o: o.dout.float(), "dout"), True, True)
    scan("takes_dout_shape", put("dout", lambda o: longer(o.dout), "dout"), True, True)
    scan("takes_out_pre_dtype", put("out_pre", lambda o: o.out_pre.float(), "out_pre"), True, True)
    scan("takes_out_pre_shape", put("out_pre", lambda o: longer(o.out_pre), "out_pre"), True, True)
    scan("takes_delta_shape", put("delta", lambda o: longer(o.delta), "delta"), False, True)
    scan("takes_z_shape", put("z", lambda o: longer(o.z), "z"), True, True)
    scan("refuse_no_dout", put("dout", lambda o: None, "dout"), True)                 # the parent: the library's AUM_E_NULL
    scan("refuse_no_out_pre", put("out_pre", lambda o: None, "out_pre"), True)
    # a checkpoint that is not on the library's side: a `meta` tensor has a device of its own and no memory, the library is told no checkpoint
    meta = lambda *shape: torch.empty(shape, dtype=torch.float32, device="meta")
    scan("takes_x_ck_device", lambda o: o.kw.update(x_ck=meta(2, 64, 2, 16)), True, True, length=1025)
    scan("refuse_x_ck_device", lambda o: o.kw.update(x_ck=meta(2, 64, 2, 16)), False, True, length=1025)      # the message names the library
    scan("refuse_x_lane_device", lambda o: o.kw.update(x_lane=meta(2, 64, 1, 16, 64)), False, True, length=513)
    scan("refuse_x_lane_device", lambda o: o.kw.update(x_lane=meta(2, 64, 1, 16, 64)), True, True, length=513)
    for bwd in (False, True):           # a checkpoint of another shape than scan_ckpt() hands out
        scan("refuse_x_ck_shape", lambda o: o.kw.update(x_ck=torch.empty((2, 64, 1, 16), device=o.u.device)), bwd, length=1025)

    def norm(name, brk, drop=False, host_only=True, bwd=True):
        @row_case(f"rmsnorm{'_drop' if drop else ''}_{'bwd' if bwd else 'fwd'}/{name}", host_only)
        def _(lib, device):
            o = Ops(x=_randn(device, "bf16", 9, 64, seed=96), w=_randn(device, "f32", 64, seed=97), residual=_randn(device, "bf16", 9, 64, seed=98),
                    scale=torch.ones(9, device=device), rps=1, dres=None)
            o["named"] = {"x": o.x, "w": o.w, "residual": o.residual, "row_scale": o.scale}
            if bwd:
                f = aum_hip.rmsnorm_drop_fwd(o.x, o.w, o.residual, o.scale, 1, lib=lib) if drop else aum_hip.rmsnorm_fwd(o.x, o.w, o.residual, lib=lib)
                o.update(rstd=f[1], saved=f[2], dy=rand_like(o.x, 3))
                o.named.update(x_saved=o.saved, dy=o.dy)
            brk(o)
            o.named.update(rstd=o.get("rstd"), dresidual=o.dres, row_scale=o.scale)
            if not bwd:
                return o.named, lambda: aum_hip.rmsnorm_drop_fwd(o.x, o.w, o.residual, o.scale, o.rps, lib=lib)
            if drop:
                return o.named, lambda: aum_hip.rmsnorm_drop_bwd(o.dy, o.saved, o.w, o.rstd, o.scale, o.rps, o.dres, lib=lib)
            return o.named, lambda: aum_hip.rmsnorm_bwd(o.dy, o.saved, o.w, o.rstd, o.dres, True, lib=lib)

    for drop in (False, True):
        norm("takes_rstd_length", put("rstd", lambda o: longer(o.rstd)), drop)
        norm("takes_rstd_dtype", put("rstd", lambda o: o.rstd.double()), drop)
        norm("takes_rstd_strided", put("rstd", lambda o: torch.stack([o.rstd, o.rstd], 1)[:, 0]), drop)
        norm("takes_dy_shape", put("dy", lambda o: torch.cat([o.dy, o.dy[:1]])), drop)
        norm("takes_dresidual_shape", put("dres", lambda o: torch.zeros(10, 64, dtype=torch.bfloat16, device=o.x.device)), drop)
    norm("refuse_no_residual", put("residual", lambda o: None), True, False, False)
    norm("refuse_whole_samples", put("rps", lambda o: 2), True, False, False)
    norm("refuse_row_scale", put("scale", lambda o: o.scale[:3]), True, True, False)          # host only: the message names the device
    norm("refuse_row_scale", put("scale", lambda o: o.scale.double()), True, True)

    @row_case("rmsnorm_fwd/refuse_column_stride")                   # a converted assert
    def _(lib, device):
        named = {"x": _randn(device, "bf16", 9, 128, seed=96), "w": _randn(device, "f32", 64, seed=97)}
        return named, lambda: aum_hip.rmsnorm_fwd(named["x"][:, ::2], named["w"], lib=lib)

    def conv(name, brk, tm, host_only=True):
        @row_case(f"{'conv1d_tm_bwd' if tm else 'conv1d_bwd'}/{name}", host_only)
        def _(lib, device):
            o = _conv_row_ops(device, ("bf16", 64, 9, 4, True, True, False, {}), 9, tm)
            brk(o)
            o.named["dy"] = o.dy
            return o.named, lambda: (aum_hip.conv1d_tm_bwd if tm else aum_hip.conv1d_bwd)(o.x, o.w, o.b, o.dy, lib=lib)

    for tm in (True, False):
        conv("takes_dy_dtype", put("dy", lambda o: o.dy.float()), tm)
        conv("takes_dy_shape", put("dy", lambda o: torch.cat([o.dy, o.dy[:, :1]], 1)), tm)       # one more token (tm) / channel: still in bounds
    conv("refuse_time_stride", put("dy", lambda o: o.dy.transpose(1, 2).contiguous().transpose(1, 2)), False, False)

    @row_case("conv1d_tm_prefill/refuse_operands")
    def _(lib, device):
        o = _prefill_ops(device, "bf16", 9)
        return o.named, lambda: aum_hip.conv1d_tm_prefill(o.x, o.cs[:1], o.w, o.b, lib=lib)

    @row_case("conv1d_tm_prefill/refuse_width")
    def _(lib, device):
        o = _prefill_ops(device, "bf16", 9, pool_width=3)
        return o.named, lambda: aum_hip.conv1d_tm_prefill(o.x, o.cs, o.w, o.b, lib=lib)

    @row_case("proj_bwd_weight/refuse_shape")
    def _(lib, device):
        named = {"x": _randn(device, "bf16", 32, 64, seed=99), "y": _randn(device, "bf16", 80, 64, seed=99)}
        return named, lambda: aum_hip.proj_bwd_weight(named["x"], named["y"], False, lib=lib)

    @row_case("proj_bwd_weight/refuse_tokens")                      # a converted assert: y2d of another token count than x2d
    def _(lib, device):
        named = {"x": _randn(device, "bf16", 64, 64, seed=99), "y": _randn(device, "bf16", 80, 128, seed=99)}
        return named, lambda: aum_hip.proj_bwd_weight(named["x"], named["y"], False, lib=lib)

    @row_case("proj_fwd/refuse_dtype")                              # a converted assert: w_dt of another dtype than the activations
    def _(lib, device):
        named = {"act": _randn(device, "bf16", 64, 64, seed=99), "w_x": _randn(device, "bf16", 80, 64, seed=99), "w_dt": _randn(device, "f16", 64, 48, seed=99)}
        return named, lambda: aum_hip.proj_fwd(named["act"], named["w_x"], named["w_dt"], 16, lib=lib)


_add_row_refusals()
ROW_GROUPS = sorted({n.split("/")[0] for n in ROW_CASES})


# ---- compare / record ------------------------------------------------------------------------------------------------------------------------
def _diff(path, a, b, out):
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                out.append(f"{path}.{k}: {'missing' if k not in a else a[k]!r} != {'missing' if k not in b else b[k]!r}")
            else:
                _diff(f"{path}.{k}", a[k], b[k], out)
    elif isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            _diff(f"{path}[{i}]", x, y, out)
    elif a != b:
        out.append(f"{path}: {a!r} != {b!r}")


def load_fixture(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def check_group(group, lib, device, fixture, cases=CASES, skip=()):
    """every case of one entry point against the fixture, field for field"""
    names = [n for n in cases if n.split("/")[0] == group and n not in skip]
    assert names
    bad = []
    for n in names:
        assert n in fixture, f"{n}: not in the fixture"
        _diff(n, run_case(cases[n], lib, device), fixture[n], bad)
    assert not bad, "\n".join(bad)


def record(lib, only=(), path=FIXTURE, cases=CASES):
    fixture = load_fixture(path) if only else {}
    for n in (only or cases):
        fixture[n] = run_case(cases[n], lib, "cpu")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(fixture[n], sort_keys=True)}" for n in sorted(fixture)) + "\n}\n")
    return fixture


if __name__ == "__main__":
    if "--record" not in sys.argv and "--record-rows" not in sys.argv:
        sys.exit("usage: python tests/binding_pin_checks.py --record | --record-rows [CASE ...]")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    where = (ROWS_FIXTURE, ROW_CASES) if "--record-rows" in sys.argv else (FIXTURE, CASES)
    done = record(aum_hip.Lib(build_emu.build(), host=True), [a for a in sys.argv[1:] if not a.startswith("--record")], *where)
    print(f"{len(done)} cases in {where[0]}")
