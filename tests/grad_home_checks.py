"""Gradient homes off the DistributedDataParallel happy path: shared bodies of tests/test_grad_home.py (CPU, lane-array library) and
tests/test_gpu_grad_home.py (device library).  A home is the bucket view a parameter's gradient lives in; the kernel that finishes the
gradient writes it there (ssi.grad_home / _homed, the out= / outs= / param_out= destinations of aum_hip).  Here the homes are attached by
hand -- p._aum_grad_home = flat[a:b].view_as(p) on a flat fp32 buffer filled with the sentinel 7.0 -- in one process, without a process group.

Part A, the destination kernels directly (check_sum_rows_dest, check_sum_rows_multi_dest, check_gemm_wgrad_dest, check_scan_param_dest,
check_unfit_dest): a destination 0, 1, 2 and 3 floats off a 16-byte boundary with 64 sentinel floats on each side gives the bits of the
same call without a destination, the result aliases it, the sentinels stay; the call without a destination meets the bar its existing test
holds against fp64 (kernel_checks' helpers; for the sums the bar of test_gpu_kernels.test_sum_rows, restated in _sum_bar).  What the store
code says about alignment (read before any of this ran): sum_rows_body stores two 16-byte groups through a struct declared
packed, aligned(4) -- global_store_dwordx4 on a 4-byte aligned address -- or, transposed, single floats; k_scant_bwd_reduce stores dA_xA,
dD and ddelta_bias one float at a time; aum_gemm_wgrad writes only its own partial tiles and its destination is aum_sum_rows'.  So every
destination takes any 4-byte aligned address and none of the four offsets is refused.  A tensor that is no fit (16-bit, not contiguous,
another element count, the count in another shape) is left untouched and the result is a new tensor.

Part B, the block and the model with homes against a deep copy without (gradients torch.equal; the copy without homes is held to the fp64
oracle once, check_oracle_once, through block_oracle_checks.reference_and_bars): steady state on two layouts of the flat buffer (every home
16-byte aligned / every home 4 bytes off), accumulation, one parameter used twice in one backward, frozen parameters, unfit homes, the
d A_log hand-over.  expected_block / expected_model below are the lists of gradients a kernel finishes, per mode.

On the host the x/dt and weight-gradient MFMA kernels do not exist (ssi._wgrad_tm and _xdt_bwd ask .is_cuda): the homes of x_proj, dt_proj,
in_proj and out_proj weights are reached on the device only, and so is the CPU-resident home of check_unfit_homes (every home is one there)
and the oracle's bars, which are derived for 16-bit autocast.  Everything else of both parts runs in both files.

Device file: 51 cases, 4.4 s on an MI355X; host file: 31 cases, 24 s.

Mutants (scratch copies, each against the host file): a destination store one element long -- "wrote behind its destination" (Slot.check);
one element short, and the transposed job stored untransposed -- "differs from the call without a destination" (Slot.check); grad_home
ignoring p.grad -- "a home was used while its gradient accumulates" (check_block_homes); grad_home without its claims (the parent commit's)
and claims released when the first gradient is handed over -- "two uses: HOME_HITS" (twice the list) in check_block_homes and
check_model_homes; grad_home ignoring requires_grad -- "the home of a frozen parameter was written" (check_frozen); _sum_out matching the
element count only -- "an unfit tensor was used as the destination" (check_unfit_dest)."""
import contextlib
import copy
import math
import types

import torch

import aum_hip
import block_oracle_checks as BO
import cases
import kernel_checks as KC

SENTINEL = KC.NORM_SENTINEL
GUARD = 64
OFFSETS = (0, 1, 2, 3)

# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
# (outer, ...): one full vector; the transposed x_proj set's element count; a tall set on the two-stage route (outer >= 1024, outer % 32 == 0)
SUM_SHAPES = [(5, 8), (3, 48, 80), (1024, 16)]
# (parts, tr_cols, which jobs get a destination): mixed, one transposed; the same with a two-stage set, which sends every job through sum_rows
SUM_MULTI_SETS = [([(7, 64, 16), (9, 40), (3, 48, 80), (5, 8)], [0, 0, 80, 0], [True, False, True, True]),
                  ([(1024, 16), (3, 48, 80), (9, 40)], [0, 80, 0], [True, True, False])]
_wg = {c[:4]: c for c in cases.GEMM_WGRAD_CASES}
WGRAD_CASES = [_wg[65, 256, 80, 1], _wg[130, 256, 256, 7]]
_scan = {c[0]: c for c in cases.SCAN_TM_CASES}
SCAN_CASES = [(_scan[n], s) for n in ("tm_l9", "tm_l75") for s in (1, 2)]
BLOCK_CASES = [BO.WIDE[n] for n in ("none_d768_l9", "v1_d384_l65", "v2_d384_l65")]
MODEL = dict(size="small", depth=2, num_classes=5, bimamba_type="v1", spectrogram_size=(128, 64))       # embed_dim 384
FROZEN = ("x_proj.weight", "A_log", "conv1d.weight", "norm.weight")


# ---- which gradients a kernel finishes -------------------------------------------------------------------------------------------------------
def _wgrad_kernel(n, k):
    """aum_gemm_wgrad's shape rule (aum_hip.gemm_wgrad_supported): dW (n, k) with n % 256 == 0 and k % 256 == 0 or a skinny width"""
    return n % 256 == 0 and (k % 256 == 0 or k in aum_hip.WGRAD_SKINNY_K)


def expected_block(mode, d_model, dev):
    """leaves of the bare block whose gradient arrives in its home.  From ssi._TM_HOMES: the conv sums and the scan's parameter sums always; x_proj
    and dt_proj on the device (dW (E, R) and (E, R + 2N) with E = 2 d_model); out_proj on the device where aum_gemm_wgrad takes (d_model, E) and
    the block owns its out_proj (Bi-Bi's is a plain linear here); A and A_b are handed to the block as they are: no A_log, no home"""
    E = 2 * d_model
    names = ["conv_w", "conv_b", "D", "dt_bias"]
    if dev != "cpu" and E % 256 == 0:
        names += ["x_proj_w", "dt_proj_w"]
    if mode == "v2":
        names += [n + "_b" for n in names]
    elif dev != "cpu" and _wgrad_kernel(d_model, E):
        names.append("out_proj_w")
    return sorted(names)


def expected_model(model, dev):
    """parameters of the model whose gradient arrives in its home: per block _TM_HOMES' conv, scan and A_log sums (step_cache puts neg_exp and the
    d A_log hand-over in play) and the RMSNorm weight sums, norm_f included; on the device the in / out / x / dt projection weights that
    aum_gemm_wgrad takes.  Everything else (patch embedding, cls token, positions, head) is autograd's own and must leave its home alone"""
    names = []
    for k, p in model.named_parameters():
        leaf = k.split(".", 2)[-1] if k.startswith("layers.") else k
        if leaf in ("mixer.conv1d.weight", "mixer.conv1d.bias", "mixer.D", "mixer.dt_proj.bias", "mixer.A_log", "mixer.A_b_log", "norm.weight", "norm_f.weight"):
            names.append(k)
        elif dev != "cpu" and leaf in ("mixer.x_proj.weight", "mixer.dt_proj.weight", "mixer.in_proj.weight", "mixer.out_proj.weight"):
            n, kk = (p.shape[1], p.shape[0]) if leaf == "mixer.x_proj.weight" else p.shape       # x_proj's sum leaves the kernel as (E, R + 2N)
            if _wgrad_kernel(n, kk):
                names.append(k)
    return sorted(names)


# ---- the flat buffer ------------------------------------------------------------------------------------------------------------------------
class Homes:
    """a sentinel-filled flat fp32 buffer with one slot per tensor of `named`, at least GUARD sentinels around each.  head = 0: every slot on
    a 16-byte boundary; head = 1: every slot one float behind one.  attach() hangs the slots on the tensors as their homes"""

    def __init__(self, named, dev, head=0):
        self.slots, at = {}, 0
        for k, p in named.items():
            at = (at + GUARD + 3) // 4 * 4 + head
            self.slots[k] = (at, p.numel())
            at += p.numel()
        self.flat = torch.full((at + GUARD + 4,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.named, self.head = named, head

    def view(self, k):
        a, n = self.slots[k]
        return self.flat[a:a + n].view_as(self.named[k])

    def attach(self):
        for k, p in self.named.items():
            p._aum_grad_home = self.view(k)
            assert p._aum_grad_home.data_ptr() % 16 == 4 * self.head
        return self

    def untouched(self, k):
        a, n = self.slots[k]
        return bool((self.flat[a:a + n] == SENTINEL).all())

    def gaps_intact(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for a, n in self.slots.values():
            keep[a:a + n] = False
        return bool((self.flat[keep] == SENTINEL).all())


class Slot:
    """one destination of `shape`, `off` floats behind a 16-byte boundary of a sentinel-filled flat buffer, GUARD sentinels on each side"""

    def __init__(self, shape, off, dev):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        a = GUARD + (-(self.buf.data_ptr() // 4 + GUARD)) % 4 + off
        self.view, self.a, self.n = self.buf[a:a + n].view(shape), a, n
        assert self.view.data_ptr() % 16 == 4 * off

    def check(self, tag, got, want):
        assert got.data_ptr() == self.view.data_ptr() and tuple(got.shape) == tuple(want.shape), tag + ("the result does not alias its destination",)
        assert torch.equal(got, want), tag + ("differs from the call without a destination",)
        assert bool((self.buf[:self.a] == SENTINEL).all()), tag + ("wrote in front of its destination",)
        assert bool((self.buf[self.a + self.n:] == SENTINEL).all()), tag + ("wrote behind its destination",)


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _sum_bar(tag, got, t, tr=False):
    """test_gpu_kernels.test_sum_rows' bar: against the fp64 sum, 2e-6 x sqrt(rows) of the largest sum (fp32 additions of `rows` terms)"""
    ref = t.double().sum(0)
    ref = ref.t() if tr else ref
    assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_contiguous(), tag
    assert float((got.double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max())) * t.shape[0] ** 0.5, tag


# ---- part A ---------------------------------------------------------------------------------------------------------------------------------
def check_sum_rows_dest(lib, dev, shape, dtype):
    """aum_hip.sum_rows(out=)"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).to(dtype).to(dev)
    want = aum_hip.sum_rows(t, lib=lib)
    _sum_bar((shape, str(dtype)), want, t)
    for off in OFFSETS:
        s = Slot(want.shape, off, dev)
        got = aum_hip.sum_rows(t, lib=lib, out=s.view)
        _sync(dev)
        s.check(("sum_rows", shape, str(dtype), off), got, want)


def check_sum_rows_multi_dest(lib, dev, shapes, tr, dest):
    """aum_hip.sum_rows_multi(outs=): some jobs with a destination, some without"""
    g = torch.Generator().manual_seed(len(shapes))
    parts = [torch.randn(sh, generator=g).to(dev) for sh in shapes]
    want = aum_hip.sum_rows_multi(parts, tr, lib=lib)
    for t, w, tc in zip(parts, want, tr):
        _sum_bar((shapes, tr), w, t, bool(tc))
        one = aum_hip.sum_rows(t, lib=lib)
        assert torch.equal(w, one.t().contiguous() if tc else one)
    for off in OFFSETS:
        slots = [Slot(w.shape, off, dev) if d else None for w, d in zip(want, dest)]
        got = aum_hip.sum_rows_multi(parts, tr, lib=lib, outs=[None if s is None else s.view for s in slots])
        _sync(dev)
        for q, (s, g_, w) in enumerate(zip(slots, got, want)):
            if s is None:
                assert torch.equal(g_, w), (shapes, off, q)
            else:
                s.check(("sum_rows_multi", tuple(shapes), off, q), g_, w)


def check_gemm_wgrad_dest(lib, dev, case, dtype):
    """aum_hip.gemm_wgrad(out=)"""
    t, n, k, splits, pad_y, pad_x = case
    g = torch.Generator().manual_seed(t * 7 + n + k + splits)
    y = torch.randn(t, n + pad_y, generator=g).to(dtype).to(dev)[:, pad_y:]
    x = torch.randn(t, k + pad_x, generator=g).to(dtype).to(dev)[:, :k]
    want = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib)
    KC.gemm_wgrad_assert(aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib, partials=True), want, y, x, splits)
    for off in OFFSETS:
        s = Slot((n, k), off, dev)
        got = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib, out=s.view)
        _sync(dev)
        s.check(("gemm_wgrad", case, str(dtype), off), got, want)


_PARAM_OUT = ("dD", "ddelta_bias", "dA_xA", "dA_b_xA")


def _scan_setup(lib, dev, case, dtype, segments):
    """the operands of kernel_checks.check_scan_tm for a Fo-Bi pair, the forward run once -> (ref, run(param_out) -> scan_tm_bwd's dict)"""
    name, batch, dim, length, dstate, has_z, has_D, has_bias, softplus = case
    ref = KC.scan_tm_reference(case, dtype, False, True)
    d = ref["inputs"]
    tm = lambda a: None if a is None else KC.T(a, dev, dtype).transpose(1, 2).contiguous()
    u, delta, z, dout = tm(d["u"]), tm(d["delta"]), tm(d["z"]), tm(d["dout"])
    bcm = torch.cat([tm(d["B"]), tm(d["C"])], dim=2).contiguous()
    Bm, Cm = bcm[:, :, :dstate], bcm[:, :, dstate:]
    A, A_b, D, bias = KC.T(d["A"], dev), KC.T(ref["A_b"], dev), KC.T(d["D"], dev), KC.T(d["delta_bias"], dev)
    ck = aum_hip.scan_tm_ckpt(batch, length, dim, dstate, True, dev, lib=lib)
    out, out_pre = aum_hip.scan_tm_fwd(u, delta, A, Bm, Cm, D, z, bias, softplus, False, A_b, want_out_pre=True, ckpt=ck, lib=lib, segments=segments)
    run = lambda po: aum_hip.scan_tm_bwd(u, delta, A, Bm, Cm, D, z, bias, dout, out_pre if has_z else None, ck, softplus, False, A_b, lib=lib,
                                         segments=segments, want_dA_xA=True, param_out=po)
    return ref, out, out_pre, (A, A_b), run


def check_scan_param_dest(lib, dev, case, dtype, segments):
    """aum_hip.scan_tm_bwd(param_out=) for dD, ddelta_bias, dA_xA and dA_b_xA of a Fo-Bi pair"""
    ref, out, out_pre, (A, A_b), run = _scan_setup(lib, dev, case, dtype, segments)
    want = run(None)
    KC.scan_tm_assert(case, dtype, False, True, None, ref, out, out_pre, out, want)
    assert torch.equal(want["dA_xA"], want["dA"] * A) and torch.equal(want["dA_b_xA"], want["dA_b"] * A_b)
    for off in OFFSETS:
        slots = {k: Slot(want[k].shape, off, dev) for k in _PARAM_OUT}
        got = run({k: s.view for k, s in slots.items()})
        _sync(dev)
        for k, s in slots.items():
            s.check(("scan_tm_bwd", case[0], str(dtype), segments, off, k), got[k], want[k])
        for k in ("du", "ddelta", "dz", "dBC", "dA", "dA_b"):           # and nothing else of the launch moved
            assert torch.equal(got[k], want[k]), (case[0], segments, off, k)


def unfit(shape, dev):
    """{kind: (the tensor passed, all of its storage)} for a destination of `shape`: every one is refused"""
    n = math.prod(shape)
    full = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device=dev)
    strided = full(n, 2)
    more, flat = full(n + 8), full(n)
    return {"bf16": (full(*shape, dt=torch.bfloat16),) * 2, "not contiguous": (strided[:, 0].view(shape) if len(shape) == 1 else strided[:, 0].unflatten(0, shape), strided),
            "another element count": (more, more), "the count in another shape": (flat.view(1, n), flat)}


def _refused(tag, got, want, passed, storage):
    assert torch.equal(got, want) and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), tag + ("wrong result",)
    assert got.data_ptr() != passed.data_ptr() and got.device == want.device, tag + ("an unfit tensor was used as the destination",)
    assert bool((storage == SENTINEL).all()), tag + ("an unfit tensor was written to",)


def check_unfit_dest(lib, dev, dtype16):
    """a tensor that is no fit as out= / outs= / param_out=: the right result in a new tensor, the passed tensor untouched.  The sums on the
    kernel route, the one-by-one route (a two-stage set in the call) and the torch route (an element count that is no multiple of 8)"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    for t in (r(5, 16), r(1024, 16), r(3, 7)):
        want = aum_hip.sum_rows(t, lib=lib)
        for kind, (o, st) in unfit(tuple(want.shape), dev).items():
            _refused(("sum_rows", tuple(t.shape), kind), aum_hip.sum_rows(t, lib=lib, out=o), want, o, st)
    for parts, tr in (([r(7, 64, 16), r(9, 40)], [16, 0]), ([r(1024, 16), r(3, 48, 80)], [0, 80]), ([r(3, 2, 5)], [5])):
        want = aum_hip.sum_rows_multi(parts, tr, lib=lib)
        for kind in unfit((8,), dev):
            outs = [unfit(tuple(w.shape), dev)[kind] for w in want]
            got = aum_hip.sum_rows_multi(parts, tr, lib=lib, outs=[o for o, _ in outs])
            for q, (g_, w, (o, st)) in enumerate(zip(got, want, outs)):
                _refused(("sum_rows_multi", tr, q, kind), g_, w, o, st)
    t_, n, k, splits, pad_y, pad_x = WGRAD_CASES[0]
    y, x = torch.randn(t_, n, generator=g).to(dtype16).to(dev), torch.randn(t_, k, generator=g).to(dtype16).to(dev)
    want = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib)
    for kind, (o, st) in unfit((n, k), dev).items():
        _refused(("gemm_wgrad", kind), aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib, out=o), want, o, st)
    _, _, _, _, run = _scan_setup(lib, dev, _scan["tm_l9"], torch.float32, 1)
    want = run(None)
    for kind in unfit((8,), dev):
        outs = {key: unfit(tuple(want[key].shape), dev)[kind] for key in _PARAM_OUT}
        got = run({key: o for key, (o, _) in outs.items()})
        for key, (o, st) in outs.items():
            _refused(("scan_tm_bwd", key, kind), got[key], want[key], o, st)
    _sync(dev)


# ---- part B: the bare block -----------------------------------------------------------------------------------------------------------------
def _autocast(dev, dtype):
    return torch.autocast(dev, dtype=dtype) if dtype is not None else contextlib.nullcontext()


def block_leaves(case, dtype, dev):
    """fresh leaves of the block (block_oracle_checks.operands: xz and dout on the 16-bit grid) -> ({name: leaf}, dout).  dtype None (the
    host): fp32 without autocast"""
    p, _ = BO.operands(case, dtype or torch.bfloat16)
    t = {k: torch.tensor(v, device=dev).requires_grad_(True) for k, v in p.items() if k != "dout"}
    return t, torch.tensor(p["dout"], device=dev)


def block_forward(ssi, case, t, dtype, dev, flip=False, A=None, A_b=None):
    """the block as block_oracle_checks.run_product calls it on token-major rows; flip: the batch entries in the other order (a second use
    of the same parameters on other data); A / A_b: in place of the leaves (neg_exp's)"""
    name, mode, batch, d_model, L = case
    xz = t["xz"].flip(0) if flip else t["xz"]
    xz = (xz if dtype is None else xz.to(dtype)).transpose(1, 2).contiguous().transpose(1, 2)
    assert ssi._is_tm(xz) and ssi.token_major_ok(2 * d_model, BO.N_STATE, 4, t["dt_proj_w"].shape[1], dtype)
    A, A_b = t["A"] if A is None else A, t.get("A_b") if A_b is None else A_b
    with _autocast(dev, dtype):
        if mode == "v1":
            return ssi.bimamba_inner_fn(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], t["out_proj_w"], None, A, A_b, None, None,
                                        t["D"], delta_bias=t["dt_bias"], delta_softplus=True)
        if mode == "none":
            return ssi.mamba_inner_fn(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], t["out_proj_w"], None, A, None, None, t["D"],
                                      delta_bias=t["dt_bias"], delta_softplus=True)
        of = ssi.mamba_inner_fn_no_out_proj(xz, t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], A, None, None, t["D"],
                                            delta_bias=t["dt_bias"], delta_softplus=True)
        ob = ssi.mamba_inner_fn_no_out_proj(xz, t["conv_w_b"], t["conv_b_b"], t["x_proj_w_b"], t["dt_proj_w_b"], A_b, None, None, t["D_b"],
                                            delta_bias=t["dt_bias_b"], delta_softplus=True, reverse=True)
        return torch.nn.functional.linear(((of + ob) / 2).transpose(1, 2), t["out_proj_w"], None)


def block_backward(ssi, case, t, dout, dtype, dev, uses=1):
    loss = sum((block_forward(ssi, case, t, dtype, dev, flip=bool(u)).float() * dout).sum() for u in range(uses))
    loss.backward()
    _sync(dev)


def _same_grads(tag, a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        ga, gb = a[k].grad, b[k].grad
        assert (ga is None) == (gb is None), tag + (k,)
        assert ga is None or torch.equal(ga, gb), tag + (k, "the gradient differs from the model without homes")


def _clones(t):
    return {k: None if v.grad is None else v.grad.clone() for k, v in t.items()}


def _drop_grads(t):
    for v in t.values():
        v.grad = None


def _steady(tag, ssi, homes, t, expect, backward):
    """one backward from empty gradients: exactly the expected gradients arrive in their homes, everything around them stays"""
    hits = ssi.HOME_HITS[0]
    backward()
    assert ssi.HOME_HITS[0] - hits == len(expect), tag + ("HOME_HITS", ssi.HOME_HITS[0] - hits, expect)
    for k, v in t.items():
        if k in expect:
            assert v.grad.data_ptr() == homes.view(k).data_ptr(), tag + (k, "not in its home")
        elif k in homes.slots:
            assert homes.untouched(k) and (v.grad is None or v.grad.data_ptr() != homes.view(k).data_ptr()), tag + (k, "a home nobody may write was written")
    assert homes.gaps_intact(), tag + ("wrote between the homes",)
    assert not ssi._HOME_CLAIMS, tag + ("claims left behind",)


def check_block_homes(ssi, case, dtype, dev, head):
    """the bare block: steady state, accumulation, a third backward from empty gradients, and two uses in one backward"""
    tag = (case[0], str(dtype), head)
    expect = expected_block(case[1], case[3], dev)
    t, dout = block_leaves(case, dtype, dev)
    r, _ = block_leaves(case, dtype, dev)
    homes = Homes({k: v for k, v in t.items() if k != "xz"}, dev, head).attach()
    bw = lambda m, uses=1: block_backward(ssi, case, m, dout, dtype, dev, uses)
    _steady(tag + ("steady",), ssi, homes, t, expect, lambda: bw(t))
    bw(r)
    _same_grads(tag + ("steady",), t, r)
    first = _clones(t)
    # accumulation: a second backward on top of the first
    hits = ssi.HOME_HITS[0]
    bw(t), bw(r)
    assert ssi.HOME_HITS[0] == hits, tag + ("a home was used while its gradient accumulates",)
    _same_grads(tag + ("accumulated",), t, r)
    assert homes.gaps_intact()
    # and from empty gradients again
    _drop_grads(t), _drop_grads(r)
    _steady(tag + ("third",), ssi, homes, t, expect, lambda: bw(t))
    for k, v in t.items():
        assert (v.grad is None and first[k] is None) or torch.equal(v.grad, first[k]), tag + (k, "the third backward differs from the first")
    # two uses of every parameter in one backward: the first node to finish takes the home, the second a tensor of its own
    _drop_grads(t)
    hits = ssi.HOME_HITS[0]
    bw(t, 2), bw(r, 2)
    assert ssi.HOME_HITS[0] - hits == len(expect), tag + ("two uses: HOME_HITS", ssi.HOME_HITS[0] - hits)
    _same_grads(tag + ("two uses",), t, r)
    assert homes.gaps_intact() and not ssi._HOME_CLAIMS


def check_oracle_once(ssi, dev, dtype=torch.bfloat16):
    """the block WITHOUT homes against the fp64 oracle at block_oracle_checks' bars (one case: bit-equality carries it to the others)"""
    case = BO.WIDE["v1_d384_l65"]
    activated, lib16 = BO.arm_roundings(case, "token_major", {}, False)
    q, ref, r_, bar = BO.reference_and_bars(case, dtype, activated, lib16)
    t, dout = block_leaves(case, dtype, dev)
    o = block_forward(ssi, case, t, dtype, dev)
    (o.float() * dout).sum().backward()
    _sync(dev)
    got = {"out": o.detach().double().cpu().numpy(), **{k: v.grad.double().cpu().numpy() for k, v in t.items()}}
    assert set(got) == set(ref)
    e = BO.distances(got, ref)
    over = {k: (e[k], bar[k]) for k in e if not e[k] < bar[k]}
    assert not over, over


def check_unfit_homes(ssi, case, dtype, dev):
    """homes that are no fit (16-bit, transposed, another shape, on the CPU) are ignored: gradients right, the tensors untouched"""
    r, dout = block_leaves(case, dtype, dev)
    block_backward(ssi, case, r, dout, dtype, dev)

    def make(kind, p):
        n = p.numel()
        if kind == "cpu":
            h = torch.full(p.shape, SENTINEL)
            return h, h
        if kind == "bf16":
            h = torch.full(p.shape, SENTINEL, dtype=torch.bfloat16, device=dev)
            return h, h
        if kind == "transposed":            # the parameter's shape, not contiguous
            st = torch.full((n, 2) if p.dim() == 1 else tuple(reversed(p.shape)), SENTINEL, device=dev)
            return (st[:, 0] if p.dim() == 1 else st.permute(*reversed(range(p.dim())))), st
        h = torch.full((1, n), SENTINEL, device=dev)        # another shape, the same count
        return h, h
    for kind in ("bf16", "transposed", "shape") + (("cpu",) if dev != "cpu" else ()):
        t, _ = block_leaves(case, dtype, dev)
        made = {k: make(kind, v) for k, v in t.items() if k != "xz"}
        for k, (h, _) in made.items():
            t[k]._aum_grad_home = h
        hits = ssi.HOME_HITS[0]
        block_backward(ssi, case, t, dout, dtype, dev)
        assert ssi.HOME_HITS[0] == hits, (kind, "an unfit home was used")
        _same_grads((case[0], kind), t, r)
        for k, (h, st) in made.items():
            assert bool((h == SENTINEL).all()) and bool((st == SENTINEL).all()), (kind, k, "an unfit home was written to")
            assert t[k].grad.data_ptr() != h.data_ptr(), (kind, k)


def check_a_used_twice(ssi, dtype, dev):
    """the v1 block on A, A_b from an open step cache (neg_exp), and A, A_b once more in the loss: the gradient that reaches _NegExpFn is not
    the scan's d A tensor, so it is multiplied by A (no hand-over, no home) -- equal to the copy without homes, and equal to the single-use
    gradient plus d (sum A) / d A_log = A up to the fp32 rounding of one addition and one product"""
    case = BO.WIDE["v1_d384_l65"]
    res = {}
    for arm in ("homes", "plain", "once"):
        t, dout = block_leaves(case, dtype, dev)
        logs = {k: torch.log(-t[k].detach()).requires_grad_(True) for k in ("A", "A_b")}
        if arm == "homes":
            homes = Homes({**{k: v for k, v in t.items() if k not in ("xz", "A", "A_b")}, **{k + "_log": v for k, v in logs.items()}}, dev, 1).attach()
        hits = ssi.HOME_HITS[0]
        with ssi.step_cache([types.SimpleNamespace(A_log=logs["A"], A_b_log=logs["A_b"])], dtype):
            A, A_b = ssi.neg_exp(logs["A"]), ssi.neg_exp(logs["A_b"])
            assert A.data_ptr() in ssi._A_OWNER and A_b.data_ptr() in ssi._A_OWNER          # out of the cache: the scan backward forms d A . A
            o = block_forward(ssi, case, t, dtype, dev, A=A, A_b=A_b)
            loss = (o.float() * dout).sum() + (0 if arm == "once" else A.sum() + A_b.sum())
        loss.backward()
        _sync(dev)
        assert not ssi._DA_XA and not ssi._A_OWNER and not ssi._HOME_CLAIMS, arm
        if arm == "homes":      # the A_log homes were offered to the scan but the gradients did not arrive there: not counted, not aliased
            assert ssi.HOME_HITS[0] - hits == len(expected_block("v1", case[3], dev)), (arm, ssi.HOME_HITS[0] - hits)
            assert all(logs[k].grad.data_ptr() != homes.view(k + "_log").data_ptr() for k in logs) and homes.gaps_intact()
        res[arm] = {k: v.grad.clone() for k, v in logs.items()}, {k: -torch.exp(v.detach()) for k, v in logs.items()}
    for k in ("A", "A_b"):
        assert torch.equal(res["homes"][0][k], res["plain"][0][k]), k
        once, A = res["once"][0][k].double(), res["once"][1][k].double()
        want = once + A
        # three fp32 roundings (d A . A handed over; d A + 1; the product), each half an ulp of a term no larger than these
        bound = 3 * 2.0 ** -24 * float((once.abs() + A.abs() + want.abs()).max())
        err = float((res["plain"][0][k].double() - want).abs().max())
        assert err <= bound, (k, err, bound)


# ---- part B: the model ----------------------------------------------------------------------------------------------------------------------
def make_model(dev):
    from aum.model import build_aum
    torch.manual_seed(11)
    model = build_aum(**MODEL).to(dev)
    g = torch.Generator().manual_seed(5)
    x = [(torch.randn(2, 64, 128, generator=g) * 0.5).to(dev) for _ in range(2)]
    w = torch.randn(2, MODEL["num_classes"], generator=g).to(dev)
    return model, x, w


def model_backward(model, xs, w, dtype, dev):
    with _autocast(dev, dtype):
        loss = sum((model(x).float() * w).sum() for x in xs)
    loss.backward()
    _sync(dev)


def check_model_homes(ssi, dtype, dev, head):
    """the depth-2 model: steady state (step_cache, neg_exp and the d A_log hand-over, the RMSNorm weight homes), accumulation, a third
    backward, two forwards in one backward; the hand-over tables empty after every backward"""
    tag = ("model", str(dtype), head)
    model, x, w = make_model(dev)
    ref = copy.deepcopy(model)
    t, r = dict(model.named_parameters()), dict(ref.named_parameters())
    expect = expected_model(model, dev)
    homes = Homes(t, dev, head).attach()
    bw = lambda m, xs=x[:1]: model_backward(m, xs, w, dtype, dev)
    empty = lambda: not ssi._DA_XA and not ssi._A_OWNER and not ssi._HOME_CLAIMS
    _steady(tag + ("steady",), ssi, homes, t, expect, lambda: bw(model))
    bw(ref)
    _same_grads(tag + ("steady",), t, r)
    assert empty()
    first = _clones(t)
    hits = ssi.HOME_HITS[0]
    bw(model), bw(ref)
    assert ssi.HOME_HITS[0] == hits, tag + ("a home was used while its gradient accumulates",)
    _same_grads(tag + ("accumulated",), t, r)
    model.zero_grad(set_to_none=True), ref.zero_grad(set_to_none=True)
    _steady(tag + ("third",), ssi, homes, t, expect, lambda: bw(model))
    for k, v in t.items():
        assert (v.grad is None and first[k] is None) or torch.equal(v.grad, first[k]), tag + (k, "the third backward differs from the first")
    model.zero_grad(set_to_none=True)
    hits = ssi.HOME_HITS[0]
    bw(model, x), bw(ref, x)                # loss = model(x1) + model(x2): every parameter has two nodes in the pass
    assert ssi.HOME_HITS[0] - hits == len(expect), tag + ("two uses: HOME_HITS", ssi.HOME_HITS[0] - hits)
    _same_grads(tag + ("two uses",), t, r)
    assert homes.gaps_intact() and empty()


def check_frozen(ssi, dtype, dev):
    """a parameter frozen AFTER its home was attached: its slice of the flat buffer stays sentinel, every other gradient is the all-trainable
    run's; with every parameter frozen and only the input taking a gradient the whole buffer stays and d input is the same bits"""
    model, x, w = make_model(dev)
    t = dict(model.named_parameters())
    homes = Homes(t, dev, 1).attach()
    xin = x[0].clone().requires_grad_(True)
    model_backward(model, [xin], w, dtype, dev)
    want, dx = _clones(t), xin.grad.clone()
    for leaf in FROZEN + ("all",):
        model.zero_grad(set_to_none=True)
        homes.flat.fill_(SENTINEL)
        frozen = [k for k in t if leaf == "all" or k.endswith(leaf)]
        assert frozen and (leaf == "all" or len(frozen) >= MODEL["depth"]), leaf
        for k in frozen:
            t[k].requires_grad_(False)
        xin.grad = None
        model_backward(model, [xin], w, dtype, dev)
        for k in t:
            if k in frozen:
                assert t[k].grad is None and homes.untouched(k), (leaf, k, "the home of a frozen parameter was written")
            else:
                assert torch.equal(t[k].grad, want[k]), (leaf, k)
        assert torch.equal(xin.grad, dx) and homes.gaps_intact(), leaf
        if leaf == "all":
            assert bool((homes.flat == SENTINEL).all())
        for k in frozen:
            t[k].requires_grad_(True)


def check_da_xa_handover(ssi, monkeypatch, dtype, dev):
    """under the model's step_cache d A_log arrives in its home (check_model_homes) and is, bit for bit, what the model computes with
    step_cache replaced by a null context: -exp(A_log) and g * A in torch"""
    import aum.model as M
    model, x, w = make_model(dev)
    plain = copy.deepcopy(model)
    t = dict(model.named_parameters())
    Homes(t, dev, 0).attach()
    hits = ssi.HOME_HITS[0]
    model_backward(model, x[:1], w, dtype, dev)
    assert ssi.HOME_HITS[0] - hits == len(expected_model(model, dev))
    assert not ssi._DA_XA and not ssi._A_OWNER
    monkeypatch.setattr(M, "step_cache", lambda mixers, dt: contextlib.nullcontext())
    model_backward(plain, x[:1], w, dtype, dev)
    for (k, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        if k.endswith("A_log") or k.endswith("A_b_log"):
            assert p.grad.data_ptr() == p._aum_grad_home.data_ptr(), k
            assert torch.equal(p.grad, q.grad), (k, "the handed-over d A . A differs from g * A")
