"""Checks of chunked streaming inference shared by tests/test_stream_chunk.py (lane-array library, host tensors) and
tests/test_gpu_stream_chunk.py (libaum_hip.so on the MI355X): aum_conv1d_tm_chunk / aum_scan_tm_chunk against the fp64 oracle run on
the WHOLE sequence, bitwise partition invariance, agreement with the per-token kernels, Mamba.step_chunk and AudioMamba.stream_*.

Expected values never come from the kernels under test: outputs of tokens [t0, t0 + T) and the caches at t0 / t0 + T are
oracle.scan_fwd (its last_state) / oracle.conv1d_fwd in fp64 on the sequence from its start, fed the inputs as rounded to the
activations' dtype.  Bars are the project's existing ones: fp32 outputs and fp32 caches within 1e-4 (rel_err), 16-bit outputs 1e-2."""
import numpy as np
import torch

import aum_hip
from conftest import rel_err
from oracle import oracle

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OUT_BAR = {"f32": 1e-4, "bf16": 1e-2, "f16": 1e-2}
CACHE_BAR = 1e-4
TS = (1, 2, 3, 7, 8, 9, 64, 513)


def _cases(kinds):
    """every T x every dtype, the options rotating so that each appears with each dtype and with short and long chunks"""
    out = []
    i = 0
    for T in TS:
        for dt in ("f32", "bf16", "f16"):
            out.append((T, dt, kinds[i % len(kinds)], i))
            i += 1
    return out


# scan option sets: (delta form, z, D, bias, x/z halves of one xz tensor, prefix length (0: zero entry caches))
SCAN_KINDS = [("sp", True, True, True, True, 5), ("act", True, True, True, False, 11), ("raw", False, False, False, False, 0),
              ("sp", False, True, True, False, 3), ("act", True, False, True, True, 0), ("raw", True, True, True, True, 9),
              ("sp", True, False, False, False, 1)]
# conv option sets: (width, bias, silu, x as the first half of an xz tensor, prefix length)
CONV_KINDS = [(4, True, True, True, 5), (4, False, False, False, 0), (3, True, True, False, 2), (2, True, False, True, 7),
              (4, True, True, False, 1), (1, False, True, False, 3), (4, True, False, True, 2)]
SCAN_CASES = _cases(SCAN_KINDS)
CONV_CASES = _cases(CONV_KINDS)


def case_id(c):
    T, dt, kind, i = c
    return f"T{T}-{dt}-" + "-".join(str(int(k)) if isinstance(k, bool) else str(k) for k in kind)


def _round(a, dt):
    """fp64 array -> (tensor in the activations' dtype, the same values back in fp64)"""
    t = torch.tensor(a, dtype=torch.float64).to(DT[dt])
    return t, t.double().numpy()


def _softplus64(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


# ---- scan -------------------------------------------------------------------------------------------
def scan_setup(case, device, batch=2, dim=64):
    T, dt, (form, has_z, has_D, has_bias, halves, t0), seed = case
    rng = np.random.default_rng(100 + seed)
    L, N = t0 + T, 16
    u_t, u = _round(rng.standard_normal((batch, L, dim)), dt)
    z_t, z = _round(rng.standard_normal((batch, L, dim)), dt)
    B_t, Bm = _round(rng.standard_normal((batch, L, N)), dt)
    C_t, Cm = _round(rng.standard_normal((batch, L, N)), dt)
    A = -np.exp(rng.standard_normal((dim, N)) * 0.5).astype(np.float32)
    D = rng.standard_normal(dim).astype(np.float32) if has_D else None
    bias = (rng.standard_normal(dim) * 0.5).astype(np.float32) if has_bias else None
    if form == "raw" and bias is not None:
        bias = np.abs(bias)
    raw = rng.standard_normal((batch, L, dim)) * 0.7 - (0.5 if form != "raw" else 0.0)
    if form == "raw":
        raw = np.abs(raw) * 0.3            # a step size used as it is must be positive for the recurrence to decay
    if form == "act":                       # the caller applied bias and softplus (fp64), the kernel gets the rounded result
        d_t, d = _round(_softplus64(raw + (bias[None, None, :] if bias is not None else 0.0)), dt)
        o_bias, o_sp = None, False
    else:
        d_t, d = _round(raw, dt)
        o_bias, o_sp = bias, form == "sp"
    tr = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))           # the oracle is channel-major (batch, dim, len)
    ref = oracle.scan_fwd(tr(u), tr(d), A, tr(Bm), tr(Cm), D, tr(z) if has_z else None, o_bias, o_sp, prec="f64")
    entry = np.zeros((batch, dim, N))
    if t0:
        entry = oracle.scan_fwd(tr(u[:, :t0]), tr(d[:, :t0]), A, tr(Bm[:, :t0]), tr(Cm[:, :t0]), D, tr(z[:, :t0]) if has_z else None, o_bias, o_sp,
                                prec="f64")["last_state"]
    if halves:                              # u and z as the two halves of one (batch, L, 2 dim) tensor
        xz = torch.cat((u_t, z_t), dim=2).to(device)
        u_d, z_d = xz[..., :dim], xz[..., dim:]
    else:
        u_d, z_d = u_t.to(device), z_t.to(device)
    bc = torch.cat((B_t, C_t), dim=2).to(device)                        # B, C as column blocks of one row, read in place
    ops = {"u": u_d[:, t0:], "delta": d_t.to(device)[:, t0:], "z": z_d[:, t0:] if has_z else None, "B": bc[:, t0:, :N], "C": bc[:, t0:, N:],
           "A": torch.tensor(A).to(device), "D": None if D is None else torch.tensor(D).to(device),
           "bias": None if bias is None or form == "act" else torch.tensor(bias).to(device), "sp": form == "sp", "act": form == "act"}
    return {"T": T, "dt": dt, "ops": ops, "entry": torch.tensor(entry, dtype=torch.float32).to(device),
            "ref_out": ref["out"].transpose(0, 2, 1)[:, t0:], "ref_state": ref["last_state"]}


def scan_run(s, cuts, lib):
    """advance a copy of the entry state over the chunk cut at `cuts` (token counts); -> (out (batch, T, dim), exit state)"""
    o = s["ops"]
    state = s["entry"].clone()
    outs, t = [], 0
    for n in cuts:
        sl = lambda a: None if a is None else a[:, t:t + n]
        outs.append(aum_hip.scan_tm_chunk(state, sl(o["u"]), sl(o["delta"]), o["A"], sl(o["B"]), sl(o["C"]), o["D"], sl(o["z"]), o["bias"], o["sp"],
                                          o["act"], lib=lib))
        t += n
    assert t == s["T"]
    return torch.cat(outs, dim=1), state


def scan_run_per_token(s, lib):
    o = s["ops"]
    state = s["entry"].clone()
    outs = []
    for t in range(s["T"]):
        outs.append(aum_hip.state_update(state, o["u"][:, t], o["delta"][:, t], o["A"], o["B"][:, t], o["C"][:, t], o["D"],
                                         None if o["z"] is None else o["z"][:, t], o["bias"], o["sp"], lib=lib))
    return torch.stack(outs, dim=1), state


# ---- conv -------------------------------------------------------------------------------------------
def conv_setup(case, device, batch=2, dim=72):
    T, dt, (width, has_bias, silu, halves, t0), seed = case
    rng = np.random.default_rng(500 + seed)
    L = t0 + T
    dim = dim if dim % 8 == 0 else dim + 8 - dim % 8
    x_t, x = _round(rng.standard_normal((batch, L, dim)), dt)
    w = (rng.standard_normal((dim, width)) * 0.5).astype(np.float32)
    bias = rng.standard_normal(dim).astype(np.float32) if has_bias else None
    ref = oracle.conv1d_fwd(np.ascontiguousarray(x.transpose(0, 2, 1)), w, bias, silu, prec="f64").transpose(0, 2, 1)

    def window(t):       # the last `width` inputs before token t of the zero-padded sequence, (batch, dim, width)
        pad = np.concatenate((np.zeros((batch, width, dim)), x), axis=1)
        return np.ascontiguousarray(pad[:, t:t + width].transpose(0, 2, 1))

    if halves:
        xz = torch.cat((x_t, torch.zeros_like(x_t)), dim=2).to(device)
        x_d = xz[..., :dim]
    else:
        x_d = x_t.to(device)
    return {"T": T, "dt": dt, "x": x_d[:, t0:], "w": torch.tensor(w).to(device), "bias": None if bias is None else torch.tensor(bias).to(device),
            "silu": silu, "entry": torch.tensor(window(t0), dtype=torch.float32).to(device), "ref_out": ref[:, t0:], "ref_state": window(L)}


def conv_run(s, cuts, lib):
    state = s["entry"].clone()
    outs, t = [], 0
    for n in cuts:
        outs.append(aum_hip.conv1d_tm_chunk(s["x"][:, t:t + n], state, s["w"], s["bias"], s["silu"], lib=lib))
        t += n
    assert t == s["T"]
    return torch.cat(outs, dim=1), state


def conv_run_per_token(s, lib):
    state = s["entry"].clone()
    outs = [aum_hip.conv1d_update(s["x"][:, t], state, s["w"], s["bias"], s["silu"], lib=lib) for t in range(s["T"])]
    return torch.stack(outs, dim=1), state


# ---- the three kernel checks, for either operator -------------------------------------------------
def _np(t):
    return t.detach().float().cpu().numpy()


def check_vs_oracle(s, run, lib):
    out, state = run(s, [s["T"]], lib)
    e_out, e_state = rel_err(_np(out), s["ref_out"]), rel_err(_np(state), s["ref_state"])
    print(f"vs oracle: out {e_out:.3e} (bar {OUT_BAR[s['dt']]:.0e}), cache {e_state:.3e} (bar {CACHE_BAR:.0e})")
    assert out.dtype == DT[s["dt"]] and state.dtype == torch.float32
    assert e_out < OUT_BAR[s["dt"]]
    assert e_state < CACHE_BAR


def check_partition_bitwise(s, run, lib):
    T = s["T"]
    out, state = run(s, [T], lib)
    cuts = [[t1, T - t1] for t1 in range(1, T)] + ([[1] * T] if T > 1 else [])
    for c in cuts:
        o2, s2 = run(s, c, lib)
        assert torch.equal(o2, out), f"outputs differ for the cut {c[:3]}... of {T}"
        assert torch.equal(s2, state), f"caches differ for the cut {c[:3]}... of {T}"


def check_vs_per_token(s, run, run_tok, lib):
    out, state = run(s, [s["T"]], lib)
    o2, s2 = run_tok(s, lib)
    e_out, e_state = rel_err(_np(out), _np(o2)), rel_err(_np(state), _np(s2))
    print(f"vs per-token kernels: out {e_out:.3e}, cache {e_state:.3e}")
    assert e_out < OUT_BAR[s["dt"]]
    assert e_state < CACHE_BAR


# ---- module and model -----------------------------------------------------------------------------
def check_mamba_chunks(d_model, device):
    """prefill 65 tokens, then chunks of (1, 4, 8, 8, 3) through forward(..., inference_params): vs the whole-sequence forward, vs the
    all-step run, and the caches after the chunks vs after stepping"""
    from types import SimpleNamespace
    from mamba_ssm.modules.mamba_simple import Mamba
    torch.manual_seed(7)
    m = Mamba(d_model, layer_idx=0, bimamba_type="none").eval().to(device)
    chunks = (1, 4, 8, 8, 3)
    L = 65 + sum(chunks)
    x = torch.randn(2, L, d_model, device=device)

    def run(cuts):
        params = SimpleNamespace(key_value_memory_dict={}, seqlen_offset=0)
        outs = [m(x[:, :65], inference_params=params)]
        t = 65
        for n in cuts:
            params.seqlen_offset = t
            outs.append(m(x[:, t:t + n], inference_params=params))
            t += n
        return torch.cat(outs, dim=1), params.key_value_memory_dict[0]

    with torch.no_grad():
        full = m(x)
        got, (conv_c, ssm_c) = run(chunks)
        stepped, (conv_s, ssm_s) = run([1] * sum(chunks))
    errs = (rel_err(_np(got), _np(full)), rel_err(_np(got), _np(stepped)), rel_err(_np(conv_c), _np(conv_s)), rel_err(_np(ssm_c), _np(ssm_s)))
    print("Mamba chunks: vs full %.3e, vs steps %.3e, conv cache %.3e, ssm cache %.3e" % errs)
    assert got.shape == full.shape
    assert max(errs) < 1e-4


def make_causal_aum(embed_dim, device, depth=4, **over):
    from aum.model import AudioMamba
    torch.manual_seed(3)
    kw = dict(spectrogram_size=(128, 256), depth=depth, embed_dim=embed_dim, num_classes=7, bimamba_type="none", use_middle_cls_token=False,
              use_end_cls_token=True, transpose_token_sequence=True, if_bidirectional=False)
    kw.update(over)
    return AudioMamba(**kw).eval().to(device)


def check_model_stream(embed_dim, device, autocast_dtype=None):
    """push the 16 columns in hops of (1, 1, 2, 4, 8): stream_read after the last hop = model(spec); reading does not advance the
    caches; a mid-clip read = _run_layers on the hand-built prefix sequence + cls row"""
    import contextlib
    from mamba_ssm.ops.triton.layernorm import rms_norm_fn
    model = make_causal_aum(embed_dim, device)
    torch.manual_seed(11)
    spec = torch.randn(2, 256, 128, device=device)
    ctx = (lambda: torch.autocast(device_type=torch.device(device).type, dtype=autocast_dtype)) if autocast_dtype is not None else contextlib.nullcontext
    bar = 1e-4 if autocast_dtype is None else 2e-2
    with torch.no_grad(), ctx():
        full = model(spec)
        cache = model.allocate_inference_cache(2)
        col, mid = 0, None
        for k in (1, 1, 2, 4, 8):
            assert model.stream_push(spec[:, 16 * col:16 * (col + k)], cache) == col + k
            col += k
            if col == 4:
                mid = model.stream_read(cache)
        a = model.stream_read(cache)
        b = model.stream_read(cache)
        # the prefix of 4 columns by hand: its tokens in time-major order with their own position rows, then the cls row
        tok, pos = model.tokens(spec)
        assert pos == model.num_patches
        prefix = torch.cat((tok[:, :4 * 8], tok[:, pos:]), dim=1)
        hidden, residual = model._run_layers(prefix)
        f = rms_norm_fn(hidden[:, -1], model.norm_f.weight, model.norm_f.bias, eps=model.norm_f.eps, residual=residual[:, -1], prenorm=False,
                        residual_in_fp32=True)
        mid_ref = model.head(f)
    e_full, e_mid = rel_err(_np(a), _np(full)), rel_err(_np(mid), _np(mid_ref))
    print(f"model stream: final read vs model(spec) {e_full:.3e}, mid-clip read vs prefix forward {e_mid:.3e} (bar {bar:.0e})")
    assert torch.equal(a, b), "stream_read advanced the caches"
    assert e_full < bar
    assert e_mid < bar


def check_model_rejects(device):
    import pytest
    for over, word in (({"bimamba_type": "v1"}, "bimamba_type"), ({"if_bidirectional": True}, "if_bidirectional"),
                       ({"use_end_cls_token": False}, "use_end_cls_token"), ({"transpose_token_sequence": False}, "transpose_token_sequence"),
                       ({"use_middle_cls_token": True}, "use_middle_cls_token")):
        m = make_causal_aum(64, device, depth=2, **over)
        with pytest.raises(ValueError, match=word):
            m.allocate_inference_cache(1)
        with pytest.raises(ValueError, match=word):
            m.stream_read({"layers": {}, "columns": 0, "batch": 1})
