"""CPU: the operand checks of the six streaming entry points, on the lane-array build (tests/emu) called directly through ctypes --
aum_conv1d_tm_chunk / _chunk_var / _prefill_var and aum_scan_tm_chunk / _chunk_var / aum_scan_tm_fwd_state_var.  Each case starts from
one valid argument struct (dim 64, 9 rows, dstate 16, width 4, bf16), breaks one thing -- or two, which pins the precedence of the
refusals -- and holds the returned AUM_E_* code.  The codes are the library's behaviour as recorded when the table was written: the
entries differ in small ways (which flags they refuse, whether row strides must be 16-byte), and the table keeps every one of them."""
import ctypes as C
import os
import sys

import pytest
import torch

import aum_hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

OK, E_NULL, E_SHAPE, E_DTYPE, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3, -4, -5
DIM, ROWS, DSTATE, WIDTH, LD = 64, 9, 16, 4, 128          # LD: elements per allocated row (room for the odd strides of the cases)
UNKNOWN_FLAG = 1 << 20


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


def _buffers():
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    b = {n: bf(ROWS + 7, LD) for n in ("x", "y", "u", "delta", "z", "B", "C", "out")}
    b.update(conv_state=f32(2, DIM, WIDTH), weight=f32(DIM, WIDTH), bias=f32(DIM), A=-torch.ones(DIM, DSTATE), D=f32(DIM), delta_bias=f32(DIM),
             state=f32(2, DIM, DSTATE), cu_seqlens=torch.tensor([0, 5, ROWS, 0], dtype=torch.int32), state_indices=torch.tensor([1, 0, 0, 0], dtype=torch.int32),
             carry=f32(2 * 2 * DIM * DSTATE + 64))
    return b


def _valid(entry, b):
    """(ctypes struct, held buffers) of one valid call of `entry`"""
    p = lambda n: b[n].data_ptr()
    conv, var = entry.startswith("aum_conv1d"), entry.endswith("_var")
    cls = {"aum_conv1d_tm_chunk": aum_hip.ConvTmChunkArgs, "aum_conv1d_tm_chunk_var": aum_hip.ConvTmChunkVarArgs,
           "aum_conv1d_tm_prefill_var": aum_hip.ConvTmPrefillVarArgs, "aum_scan_tm_chunk": aum_hip.ScanTmChunkArgs,
           "aum_scan_tm_chunk_var": aum_hip.ScanTmChunkVarArgs, "aum_scan_tm_fwd_state_var": aum_hip.ScanTmFwdStateVarArgs}[entry]
    a = cls()
    if conv:
        a.x, a.conv_state, a.weight, a.bias, a.y = p("x"), p("conv_state"), p("weight"), p("bias"), p("y")
        a.x_ts, a.y_ts, a.width, a.flags = LD, DIM, WIDTH, aum_hip.CONV_SILU
    else:
        for n in ("u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out"):
            setattr(a, n, p(n))
        a.u_ts = a.delta_ts = a.z_ts = a.B_ts = a.C_ts = LD
        a.out_ts, a.dstate, a.flags = DIM, DSTATE, aum_hip.SCAN_SOFTPLUS
    a.dim, a.dtype = DIM, aum_hip.AUM_BF16
    if var:
        a.cu_seqlens, a.state_indices = p("cu_seqlens"), p("state_indices")
        a.total, a.nseq, a.nrows = ROWS, 2, 2
        if hasattr(a, "max_len"):
            a.max_len = 5
    else:
        a.batch, a.len = 1, ROWS
        for n in (("x", "y") if conv else ("u", "delta", "z", "B", "C", "out")):
            setattr(a, n + "_bs", getattr(a, n + "_ts") * ROWS)
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _both(*fs):
    def f(a):
        for g in fs:
            g(a)
    return f


def _bump(field, by):
    return lambda a: setattr(a, field, getattr(a, field) + by)


def _ranges(a):          # the longest session (5 rows) cut into ranges of 8 steps: one range, a carry buffer
    a.range_len, a.carry, a.carry_bytes = 8, _BUF["carry"].data_ptr(), _BUF["carry"].numel() * 4


_BUF = _buffers()
_FLAG = lambda a: setattr(a, "flags", a.flags | UNKNOWN_FLAG)
_CONV = [
    ("valid", _set(), OK, OK, OK),
    ("null_x", _set(x=None), E_NULL, E_NULL, E_NULL),
    ("null_conv_state", _set(conv_state=None), E_NULL, E_NULL, E_NULL),
    ("dim_0", _set(dim=0), E_SHAPE, E_SHAPE, E_SHAPE),
    ("dtype_3", _set(dtype=3), E_DTYPE, E_DTYPE, E_DTYPE),
    ("width_5", _set(width=5), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("x_misaligned", _bump("x", 2), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("x_ts_68", _set(x_ts=68), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("x_is_y", lambda a: setattr(a, "y", a.x), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("x_ts_negative", _set(x_ts=-LD), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("unknown_flag", _FLAG, OK, OK, E_UNSUPPORTED),
    ("peek_flag", lambda a: setattr(a, "flags", a.flags | aum_hip.CONV_PEEK_LAST), E_UNSUPPORTED, OK, E_UNSUPPORTED),
    ("null_x+dtype_3", _set(x=None, dtype=3), E_NULL, E_NULL, E_NULL),
    ("dim_0+dtype_3", _set(dim=0, dtype=3), E_SHAPE, E_SHAPE, E_SHAPE),
    ("dtype_3+width_5", _set(dtype=3, width=5), E_DTYPE, E_DTYPE, E_DTYPE),
    ("width_5+x_is_y", _both(_set(width=5), lambda a: setattr(a, "y", a.x)), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("x_is_y+unknown_flag", _both(lambda a: setattr(a, "y", a.x), _FLAG), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
]
_SCAN = [
    ("valid", _set(), OK, OK, OK),
    ("valid_no_z", _set(z=None, z_ts=0), OK, OK, OK),
    ("valid_activated", lambda a: setattr(a, "flags", aum_hip.SCAN_DELTA_ACTIVATED), OK, OK, OK),
    ("null_u", _set(u=None), E_NULL, E_NULL, E_NULL),
    ("null_state", _set(state=None), E_NULL, E_NULL, E_NULL),
    ("dim_0", _set(dim=0), E_SHAPE, E_SHAPE, E_SHAPE),
    ("dtype_3", _set(dtype=3), E_DTYPE, E_DTYPE, E_DTYPE),
    ("dstate_8", _set(dstate=8), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("u_misaligned_2", _bump("u", 2), OK, OK, E_UNSUPPORTED),
    ("u_misaligned_1", _bump("u", 1), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("u_ts_68", _set(u_ts=68), OK, OK, E_UNSUPPORTED),
    ("u_is_out", lambda a: setattr(a, "out", a.u), OK, OK, OK),
    ("u_ts_negative", _set(u_ts=-LD), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("unknown_flag", _FLAG, E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("peek_flag", lambda a: setattr(a, "flags", a.flags | aum_hip.SCAN_PEEK_LAST), E_UNSUPPORTED, OK, E_UNSUPPORTED),
    ("activated_no_z", lambda a: (setattr(a, "flags", aum_hip.SCAN_DELTA_ACTIVATED), setattr(a, "z", None)), OK, OK, E_UNSUPPORTED),
    ("state_misaligned", _bump("state", 4), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
    ("null_u+dtype_3", _set(u=None, dtype=3), E_NULL, E_NULL, E_NULL),
    ("dim_0+dtype_3", _set(dim=0, dtype=3), E_SHAPE, E_SHAPE, E_SHAPE),
    ("dtype_3+dstate_8", _set(dtype=3, dstate=8), E_DTYPE, E_DTYPE, E_DTYPE),
    ("dstate_8+unknown_flag", _both(_set(dstate=8), _FLAG), E_UNSUPPORTED, E_UNSUPPORTED, E_UNSUPPORTED),
]
# the packed entries only: (case, mutation, chunk_var, prefill_var / fwd_state_var); None: the entry has no such field
_VAR_CONV = [
    ("null_cu_seqlens", _set(cu_seqlens=None), E_NULL, E_NULL),
    ("nseq_0", _set(nseq=0), E_SHAPE, E_SHAPE),
    ("state_indices_misaligned", _bump("state_indices", 2), E_UNSUPPORTED, E_UNSUPPORTED),
    ("max_len_gt_total", _set(max_len=ROWS + 1), None, E_UNSUPPORTED),
    ("max_len_0", _set(max_len=0), None, E_SHAPE),
    ("null_x+null_cu_seqlens", _set(x=None, cu_seqlens=None), E_NULL, E_NULL),
    ("null_cu_seqlens+dim_0", _set(cu_seqlens=None, dim=0), E_NULL, E_NULL),
    ("nseq_0+state_indices_misaligned", _both(_set(nseq=0), _bump("state_indices", 2)), E_SHAPE, E_SHAPE),
    ("state_indices_misaligned+dim_0", _both(_bump("state_indices", 2), _set(dim=0)), E_UNSUPPORTED, E_UNSUPPORTED),
    ("dtype_3+max_len_gt_total", _set(dtype=3, max_len=ROWS + 1), None, E_DTYPE),
]
_VAR_SCAN = _VAR_CONV[:3] + [
    ("max_len_gt_total", _set(max_len=ROWS + 1), None, E_UNSUPPORTED),
    ("max_len_0", _set(max_len=0), None, E_SHAPE),
    ("valid_ranges", _ranges, None, OK),
    ("range_len_4", _both(_ranges, _set(range_len=4)), None, E_UNSUPPORTED),
    ("range_len_negative", _set(range_len=-8), None, E_SHAPE),
    ("null_carry", _both(_ranges, _set(carry=None)), None, E_NULL),
    ("carry_bytes_short", _both(_ranges, _set(carry_bytes=64)), None, E_WORKSPACE),
    ("carry_misaligned", _both(_ranges, _bump("carry", 2)), None, E_WORKSPACE),
    ("null_u+null_cu_seqlens", _set(u=None, cu_seqlens=None), E_NULL, E_NULL),
    ("null_cu_seqlens+dim_0", _set(cu_seqlens=None, dim=0), E_NULL, E_NULL),
    ("nseq_0+state_indices_misaligned", _both(_set(nseq=0), _bump("state_indices", 2)), E_SHAPE, E_SHAPE),
    ("state_indices_misaligned+dstate_8", _both(_bump("state_indices", 2), _set(dstate=8)), E_UNSUPPORTED, E_UNSUPPORTED),
    ("range_len_4+carry_bytes_short", _both(_ranges, _set(range_len=4, carry_bytes=64)), None, E_UNSUPPORTED),
    ("null_carry+carry_bytes_short", _both(_ranges, _set(carry=None, carry_bytes=64)), None, E_NULL),
    ("dtype_3+max_len_gt_total", _set(dtype=3, max_len=ROWS + 1), None, E_DTYPE),
    ("unknown_flag+range_len_4", _both(_ranges, _FLAG, _set(range_len=4)), None, E_UNSUPPORTED),
]
_CONV_ENTRIES = ("aum_conv1d_tm_chunk", "aum_conv1d_tm_chunk_var", "aum_conv1d_tm_prefill_var")
_SCAN_ENTRIES = ("aum_scan_tm_chunk", "aum_scan_tm_chunk_var", "aum_scan_tm_fwd_state_var")


def _table():
    rows = []
    for entries, shared, packed in ((_CONV_ENTRIES, _CONV, _VAR_CONV), (_SCAN_ENTRIES, _SCAN, _VAR_SCAN)):
        for name, mut, *codes in shared:
            rows += [(e, name, mut, c) for e, c in zip(entries, codes)]
        for name, mut, *codes in packed:
            rows += [(e, name, mut, c) for e, c in zip(entries[1:], codes) if c is not None]
    return rows


TABLE = _table()


def run_case(lib, entry, mut):
    a = _valid(entry, _BUF)
    mut(a)
    return getattr(lib.c, entry)(C.byref(a), None)


@pytest.mark.parametrize("entry,name,mut,code", TABLE, ids=[f"{e}-{n}" for e, n, _, _ in TABLE])
def test_streaming_entry_operand_check(emu, entry, name, mut, code):
    assert run_case(emu, entry, mut) == code
