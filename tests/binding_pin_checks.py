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
named cases.

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


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def check_group(group, lib, device, fixture):
    """every case of one entry point against the fixture, field for field"""
    names = [n for n in CASES if n.split("/")[0] == group]
    assert names
    bad = []
    for n in names:
        assert n in fixture, f"{n}: not in the fixture"
        _diff(n, run_case(CASES[n], lib, device), fixture[n], bad)
    assert not bad, "\n".join(bad)


def record(lib, only=()):
    fixture = load_fixture() if only else {}
    for n in (only or CASES):
        fixture[n] = run_case(CASES[n], lib, "cpu")
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(fixture[n], sort_keys=True)}" for n in sorted(fixture)) + "\n}\n")
    return fixture


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/binding_pin_checks.py --record [CASE ...]")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    done = record(aum_hip.Lib(build_emu.build(), host=True), [a for a in sys.argv[1:] if a != "--record"])
    print(f"{len(done)} cases in {FIXTURE}")
