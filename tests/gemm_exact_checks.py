"""The matrix products of the projections, held to their contract -- exact 16-bit products, fp32 accumulation, ONE rounding -- element by element:
aum_gemm_tn (every schedule), aum_gemm_wgrad, aum_dtproj_tm_fwd, aum_xdt_tm_fwd, aum_xdt_tm_bwd and the channel-major aum_proj_fwd / _bwd_data /
_bwd_weight.  Shared by tests/test_gemm_exact.py (CPU: the conditions on the inputs on the reference alone; the plain-loop host library; the
lane-array build of proj_kernels.h) and tests/test_gpu_gemm_exact.py (device library).  The older checks of these kernels (gemm_assert,
dtproj_assert, xdt_assert, xdt_bwd_assert, check_proj) allow one 16-bit ulp of the LARGEST result; they stay as they are.

Part A -- exact inputs, bit-equal outputs, no tolerance.  Operands are integers in [-V, V] times a power of two, each operand with its own V
and scale (recipe()); every product is then an fp32 number and, with sum |a||b| < 2^24 quanta, so is every partial sum in any order: the
kernel's fp32 accumulator holds the fp64 product exactly and the stored value must be its one nearest-even rounding, bit for bit.  Chained
outputs (delta from x_dbl, du from dx_dbl, and the proj kernels' twins) are expected from the EXPECTED ROUNDED intermediate, so that a
kernel that feeds the unrounded fp32 accumulators on fails.  check_conditions asserts on the fp64 reference alone, for every case and dtype:
  1. sum |a||b| (plus |addend|) < 2^24 q_a q_b, with the rounded intermediate as the operand of a chained product;
  2. results and intermediates finite, below 65504 in fp16, every nonzero magnitude at least 2^-14 (no 16-bit subnormals);
  3. at least 10 % of an output needs rounding, at least 0.5 % are exact ties, ties to even occur toward zero and away from it;
  4. rounding toward zero changes at least 1 % of the elements, and so does rounding half away from zero (each on its own).
The fp32 weight gradients (aum_gemm_wgrad, aum_proj_bwd_weight) are held to 1 and 2 and must equal the fp64 sum, per split partial too.

Recipe (V, log2 scale) per operand:
  family                       dtype  activation side   first weight                     chained weight (w_dt fwd, w_x^T bwd)
  gemm_tn, gemm_wgrad          bf16   15, 0             15, 0                            -
                               fp16   31, 0             31, 0 (k >= 1024: -4)            -
  dtproj                       bf16   15, 0             15, 0                            -
                               fp16   rank 8: 255, 0 / 255, -4;  rank 24: 63, 0 / 63, -3;  rank 48, 64: 31, 0 / 31, -2
  xdt fwd, xdt bwd             bf16   15, 0             15, 0                            3, 0 (dim >= 1024: 1, 0)
                               fp16   31, 0             31, -4 (dim >= 1024: -6)         3, -4
  proj (dim 64)                bf16   30, 0             15, 0                            3, 0
                               fp16   62, 0             31, -4                           15, -4
  du_in / dB | dC of the backward kernels: the activation side's V on the quantum of the sum they join (exact in the 16-bit type).
Why: V = 15 (bf16) / 31 (fp16) carries sums of 64 and more products past the 8 / 11 significand bits; at dt rank 8 fp16 needs V = 255 (8 x
255^2 is far below 2^24); the fp16 scales keep x_dbl, the dt block, delta and du at dim >= 1024 and the k = 1536 GEMM below 65504.  The
chained weight stays small so that the second sum keeps ties: with V = 3 at dim >= 1024 bf16's delta and du had 1.9 % ties, of which half
(0.93 %) change under half-away -- under condition 4 -- and V = 1 (weights in {-1, 0, 1}) gives 3.5-3.9 %.  The proj cases have dim 64 only:
the activation side takes larger integers, and fp16's dx_dbl rows (w_dt^T ddelta, 64 terms) need V = 15 on w_dt to pass 2048.

Measured shares (lowest - highest over the cases; print_shares(), tests/test_gemm_exact.py::test_input_conditions -s):
  output             dtype  inexact        ties           toward zero differs   half away differs
  gemm_tn            bf16   42.6-81.6 %    11.7-23.4 %    22.3-40.8 %           5.9-11.3 %
  gemm_tn            fp16   27.0-70.2 %    16.9-22.6 %    13.7-35.0 %           8.5-11.3 %
  dtproj             bf16   25.0-47.1 %    19.4-23.4 %    10.9-23.3 %           9.5-12.5 %
  dtproj             fp16   20.2-85.9 %     9.4-22.0 %    10.1-54.7 %           1.6-11.4 %
  xdt x_dbl          bf16   52.2-82.0 %    12.2-18.9 %    25.0-41.0 %           5.7-12.5 %
  xdt x_dbl          fp16   37.0-69.7 %    16.9-23.2 %    19.1-34.2 %           8.8-10.7 %
  xdt delta          bf16   86.4-96.0 %     3.2- 9.0 %    42.0-50.4 %           1.6- 5.5 %
  xdt delta          fp16   82.2-96.0 %     3.0-12.2 %    39.9-47.9 %           1.5- 6.3 %
  xdt_bwd dt block   bf16   62.4-81.6 %    11.9-18.5 %    33.4-40.5 %           6.0- 8.9 %
  xdt_bwd dt block   fp16   47.0-70.4 %    16.5-23.4 %    22.5-35.5 %           8.0-11.9 %
  xdt_bwd du         bf16   93.7-97.0 %     2.3- 4.7 %    46.6-48.5 %           1.2- 2.5 %
  xdt_bwd du         fp16   88.9-96.1 %     2.9- 7.7 %    43.8-48.2 %           1.5- 3.9 %
  proj x_dbl         bf16 / fp16   64.4-65.3 % / 47.5-47.8 %    19.0-19.7 % / 22.2-22.5 %    32.6 % / 23.8 %    9.0 % / 11.4 %
  proj delta         bf16 / fp16   82.6-88.8 % / 93.3-95.3 %     8.4- 9.3 % /  4.0- 4.2 %    41.1 % / 45.8 %    4.1 % /  1.8 %
  proj dx_dbl        bf16 / fp16   17.7-21.0 % / 23.8-27.3 %    14.6-17.2 % / 18.7-20.6 %     7.3 % / 11.5 %    8.5 % /  9.6 %
  proj dconv         bf16 / fp16   90.2-91.6 % / 95.0-96.1 %     6.3- 7.3 % /  3.1- 4.0 %    45.9 % / 45.6 %    3.0 % /  1.3 %   (last two: the lowest)

Part B -- the usual randn operands of kernel_checks.py at the same shapes, a DERIVED per-element interval in place of the global bar:
e = k 2^-23 (|a| @ |b|^T) elementwise in fp64 -- the any-order summation bound with one FULL fp32 ulp per accumulation, so that a matrix unit
that truncates inside still passes -- and rn(ref - e) <= out <= rn(ref + e), rn the (monotone) rounding of out's type.  An addend (du_in)
counts as one more accumulation; the fp32 weight gradients take their token count (the total: the longest split plus one per summed partial;
aum_proj_bwd_weight: ntok + 64).  Chained outputs take the kernel's OWN rounded intermediate as the operand, as the older asserts do.
Largest figure per family on the MI355X (185 device cases).  For an fp32 output the figure is |out - ref| / e.  For a 16-bit output
|out - ref| is the final rounding itself (half a 16-bit ulp, thousands of e), so the figure is the smallest error BEFORE that rounding that
explains out -- 0 where out = rn(ref), else the distance from ref to the rounding boundary on out's side -- over e:
  gemm_tn 0.001 (all four schedules)     gemm_wgrad 0.454          dtproj_tm_fwd 0.002
  xdt_tm_fwd x_dbl 0.001 / delta 0.017   xdt_tm_bwd dt block 0.001 / du 0.007
  proj x_dbl, delta, dx_dbl < 0.001      proj dconv 0.004          proj dw 0.004
(the plain loops of the host library give the same order of figures; theirs is sequential fp32 summation.)

Part C -- edges, exact again (check_edges, check_subnormal_inputs; aum_gemm_tn under every schedule at k = 448, aum_dtproj_tm_fwd, aum_xdt_tm_fwd):
an all-zero row and a row whose products cancel in pairs give +0 as the bit pattern; fp16 results 65504 (stays), 65520 (the tie: inf),
65536 and beyond (inf), 65488 (a tie, down to 65472) and their negatives equal Tensor.to(float16) of the exact value; the largest finite
inputs of the type against weights below 1/2 stay inside fp32 and are bit-equal; 16-bit SUBNORMAL inputs (integers times 2^-24 in fp16,
2^-133 in bf16 -- the latter subnormal as fp32 numbers too) against weights of 2^10 / 2^120 give the rounded fp64 product bit for bit on the
MI355X: v_mfma_f32_16x16x32_{bf16,f16} of gfx950 does not flush subnormal inputs (MFMA_FLUSHES_SUBNORMAL_INPUTS).

Mutants (scratch copies of the tree, never committed).  (a), (b), (d) in the plain loops of tests/emu/aum_emu.cpp, run by tests/test_gemm_exact.py;
"old" = the max-abs checks of the same loops in tests/test_emu_kernels.py (test_gemm_tn_contract, test_dtproj_tm_contract, test_xdt_tm_contract,
test_xdt_tm_bwd_contract, test_gemm_wgrad_contract):
  (a) the loops' 16-bit stores round toward zero            new: 119 of 175 fail -- every exact and interval case of gemm_tn (19 of 20), dtproj, xdt fwd and
                                                            bwd, every edge and subnormal case; the wgrad and (lane-array, untouched) proj cases pass.
                                                            old: 9 of 19 fail (where the largest result happens to lose most of an ulp), 10 pass
  (b) xdt fwd delta from the fp32 accumulators, not from    new: 40 fail -- all 18 test_xdt_tm_fwd_exact (delta differs from the product of the expected
      the rounded x_dbl                                     rounded x_dbl), all 18 _interval (delta outside the interval around the product of the kernel's
                                                            own x_dbl), the xdt edge and subnormal cases.   old: all 19 pass
  (d) wgrad split boundaries 64 tokens early                new: 24 fail -- every exact and interval case with more than one split (partials name the first
                                                            wrong element; totals still pass).   old: 2 of 11 wgrad cases fail
  (c) one wave's last k-slot of the last K-step of k_gemm_tn multiplied as zero: a device-kernel mutant; it was NOT run -- the device runs
      of this work take the committed tree only, and a mutant is never put there.  What stands for it here: dropping one of k products changes
      an exact-input result by a whole product (|a b| >= 1 quantum wherever both are nonzero: 94 % of the pairs at V = 15), and assert_bits
      reports every such element; the old bar sees a dropped product only where it exceeds one 16-bit ulp of the LARGEST result.
"""
import torch

import aum_hip
import cases
import xdt_tiny_checks as XT

BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = (BF16, FP16)
DT_ID = {BF16: "bf16", FP16: "fp16"}
dt_id = lambda d: DT_ID[d]
FP16_MAX = 65504.0
SENTINEL = 7.0                      # check_gemm's: exact in both types

SCHEDS = {"auto": 0, "lockstep": aum_hip.GEMM_LOCKSTEP, "pipelined": aum_hip.GEMM_PIPELINED, "paced": aum_hip.GEMM_PACED}
PACED_MIN_K = 448                   # seven K-steps; below it the paced flag is refused (tests/test_gpu_kernels.py::test_gemm_tn)

# (m, n, k, pad_a, pad_c)
GEMM_CASES = [(1, 256, 64, 0, 0), (257, 512, 192, 0, 0), (385, 512, 448, 0, 0), (576, 256, 512, 0, 0), (130, 768, 1536, 64, 256)]
# (t, n, k, splits, pad_y, pad_x): three of cases.GEMM_WGRAD_CASES and every skinny k at one split and at three
WGRAD_CASES = ([(65, 256, 256, 1, 0, 0), (513, 512, 256, 3, 8, 16), (130, 256, 256, 7, 0, 8)]
               + [(65, 256, k, 1, 0, 0) for k in aum_hip.WGRAD_SKINNY_K] + [(513, 512, k, 3, 0, 0) for k in aum_hip.WGRAD_SKINNY_K])
assert all(c in cases.GEMM_WGRAD_CASES for c in WGRAD_CASES[:3])
DTPROJ_CASES = [(1, 64, 8, 40), (33, 96, 24, 56), (129, 256, 48, 80), (70, 128, 64, 96)]              # (ntok, dim, rank, ncols)
# (ntok, dim, rank, ncols); ncols 48: the Tiny layout [dt 12 | 4 zero | B | C] built by xdt_tiny_checks.pad_weights
XDT_CASES = [(1, 256, 8, 80), (33, 256, 24, 80), (129, 768, 32, 80), (300, 1024, 64, 80), (145, 1536, 48, 80),
             (145, 768, 24, 56), (300, 512, 16, 56), (17, 128, 16, 48), (129, 384, 16, 48)]
# (ntok, dim, pad, ncols): the dt block is ncols - 32 wide
XDT_BWD_CASES = ([(33, 256, 8, 80), (145, 768, 16, 80), (300, 1536, 0, 80)]
                 + [(t, d, 8, 56) for t in (33, 145, 300) for d in (256, 768)])
# the smallest of cases.PROJ_CASES and one whose dt_rank is no multiple of 16
PROJ_CASES = [c for c in cases.PROJ_CASES if c[0] in ("n8", "tiny_ranks")]
assert len(PROJ_CASES) == 2
EDGE_FAMILIES = ("gemm_auto", "gemm_lockstep", "gemm_pipelined", "gemm_paced", "dtproj", "xdt")

# Part C: does the matrix unit treat 16-bit subnormal INPUTS as zero?  (observed on the MI355X, see the header and DESIGN.md section 3)
MFMA_FLUSHES_SUBNORMAL_INPUTS = {BF16: False, FP16: False}

RATIOS = {}                          # Part B: family -> the largest (smallest error before the rounding that explains out) / e seen in this process
SHARES = {}                          # Part A: (family, dtype) -> [inexact share, tie share] lists


# ---- the 16-bit grid in fp64 ----------------------------------------------------------------------------------------------------------
def rn16(x64, dtype):
    """fp64 -> the 16-bit type by round-to-nearest-even through fp32 (the values of Part A and C are exact in fp32; in Part B the double
    rounding is inside the interval's slack, see assert_interval)"""
    return x64.to(torch.float32).to(dtype)


def _bits(t16):
    return t16.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def _from_bits(b, dtype):
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(dtype)


def mag_step(t16, up):
    """the neighbour of every element on the 16-bit grid, away from zero (up) or toward it: sign-magnitude bit patterns +- 1"""
    b = _bits(t16)
    return _from_bits(b + (1 if up else -1), t16.dtype)


def roundings(ref, dtype):
    """ref (fp64, exact) on the 16-bit grid: nearest-even, toward zero, half away from zero, and the masks inexact / tie / tie resolved
    toward zero (down) / away (up)"""
    rne = rn16(ref, dtype)
    r = rne.double()
    inexact = r != ref
    below = r.abs() < ref.abs()                                  # nearest-even went toward zero
    lo = torch.where(below, r, mag_step(rne, False).double())    # the grid point toward zero of ref (where inexact)
    hi = torch.where(below, mag_step(rne, True).double(), r)
    tie = inexact & ((ref - lo).abs() == (hi - ref).abs())
    rz = torch.where(inexact, lo, r)
    rha = torch.where(tie, hi, r)
    return dict(rne=rne, rz=rz, rha=rha, inexact=inexact, tie=tie, tie_down=tie & below, tie_up=tie & ~below)


def check_conditions(name, dtype, ref, absum, quantum, family=None, rounded=True):
    """The conditions of Part A on one output, on the fp64 reference alone.  ref: the fp64 result; absum: |a| @ |b|^T (plus |addend|) in
    fp64; quantum: q_a q_b, of which every product is a whole multiple.  rounded=False: an fp32 output (weight gradients), conditions 1
    and 2 only."""
    assert absum.max().item() < 2.0 ** 24 * quantum, (name, "1: fp32 sums not exact in every order", absum.max().item() / quantum)
    assert torch.isfinite(ref).all(), (name, "2: not finite")
    nz = ref[ref != 0].abs()
    assert nz.numel() and nz.min().item() >= 2.0 ** -14, (name, "2: a 16-bit subnormal", nz.min().item() if nz.numel() else None)
    assert torch.equal(ref.float().double(), ref), (name, "not exact in fp32")
    if not rounded:
        return None
    if dtype == FP16:
        assert ref.abs().max().item() < FP16_MAX, (name, "2: beyond fp16", ref.abs().max().item())
    r = roundings(ref, dtype)
    n = ref.numel()
    inexact, ties = r["inexact"].sum().item() / n, r["tie"].sum().item() / n
    assert inexact >= 0.10, (name, "3: inexact share", inexact)
    assert ties >= 0.005, (name, "3: tie share", ties)
    assert r["tie_down"].any() and r["tie_up"].any(), (name, "3: ties to even in one direction only")
    rz, rha = (r["rz"] != r["rne"].double()).sum().item() / n, (r["rha"] != r["rne"].double()).sum().item() / n
    assert rz >= 0.01 and rha >= 0.01, (name, "4: toward zero / half away change too few elements", rz, rha)
    if family:
        SHARES.setdefault((family, dtype), []).append((inexact, ties, rz, rha))
    return inexact, ties, rz, rha


def assert_bits(name, out, want):
    """out is want bit for bit (16-bit or fp32 patterns: -0 and +0 differ); names the count and the first wrong element"""
    assert out.shape == want.shape and out.dtype == want.dtype, (name, out.shape, want.shape, out.dtype, want.dtype)
    iv = torch.int16 if out.element_size() == 2 else torch.int32
    o, w = out.detach().cpu().contiguous().view(iv), want.detach().cpu().contiguous().view(iv)
    if torch.equal(o, w):
        return
    bad = (o != w).reshape(o.shape[0], -1) if o.dim() > 1 else (o != w).reshape(1, -1)
    row, col = [int(v) for v in bad.nonzero()[0]]
    flat_o, flat_w = out.detach().cpu().reshape(bad.shape), want.detach().cpu().reshape(bad.shape)
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first (row, col, got, want) = "
                         f"({row}, {col}, {flat_o[row, col].item()!r}, {flat_w[row, col].item()!r})")


def _value_step(t, toward):
    """neighbour of every element of the 16-bit tensor t in the direction of the fp64 tensor `toward`"""
    up_in_value = toward > t.double()
    zero = t.double() == 0
    away = (up_in_value == (t.double() > 0)) | zero
    nb = torch.where(away, mag_step(t, True), mag_step(t, False))
    tiny = mag_step(torch.zeros_like(t), True)                    # the smallest subnormal
    return torch.where(zero, torch.where(up_in_value, tiny, -tiny), nb)


def assert_interval(name, out, ref, e, family):
    """Part B: rn(ref - e) <= out <= rn(ref + e) per element, rn the rounding of out's type (monotone, so an fp32 result within e of ref
    cannot round outside).  ref, e: fp64 on the host.  The two bounds are formed in fp64 and rounded fp64 -> fp32 -> 16 bit; that loses
    nothing: the accumulator v is an fp32 number, so v >= ref - e gives v = rn32(v) >= rn32(ref - e), and rn16 is monotone.  Records in RATIOS the smallest error before the rounding that explains out, over e."""
    o = out.detach().cpu()
    conv = (lambda x: x.float()) if o.dtype == torch.float32 else (lambda x: rn16(x, o.dtype))
    lo, hi = conv(ref - e).double(), conv(ref + e).double()
    od = o.double()
    bad = ~((lo <= od) & (od <= hi))
    # the smallest |error| of the fp32 value that rounds to out: 0 where out = rn(ref), else the distance from ref to the rounding boundary
    # on out's side (fp32 outputs: |out - ref| less half an fp32 ulp; taken as |out - ref|)
    if o.dtype == torch.float32:
        d = (od - ref).abs()
    else:
        nb = _value_step(o, ref).double()
        d = torch.where(od == conv(ref).double(), torch.zeros_like(ref), ((od + nb) / 2 - ref).abs())
    ratio = torch.where(e > 0, d / e.clamp_min(1e-300), torch.zeros_like(d)).max().item()
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"{name}: max explained error / e = {ratio:.3f}; {int((od != conv(ref).double()).sum())} of {od.numel()} elements differ from rn(ref)")
    if bad.any():
        b2 = bad.reshape(bad.shape[0], -1)
        row, col = [int(v) for v in b2.nonzero()[0]]
        f = lambda t: t.reshape(b2.shape)[row, col].item()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside [rn(ref - e), rn(ref + e)]; first (row, col, got, "
                             f"lo, hi, ref, e) = ({row}, {col}, {f(od)!r}, {f(lo)!r}, {f(hi)!r}, {f(ref)!r}, {f(e)!r})")
    return ratio


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, V, qexp):
    """integers in [-V, V] times 2^qexp, fp64"""
    return torch.randint(-V, V + 1, shape, generator=g).double() * 2.0 ** qexp


def recipe(family, dtype, k, k2=0):
    """(V, log2 scale) per operand: ((V_a, q_a), (V_b, q_b), (V_c, q_c)).  a: the activation-side operand, b: the first weight, c: the
    weight of the chained product (w_dt forward, w_x^T backward).  See the header for the reasons."""
    bf = dtype == BF16
    if family in ("gemm", "wgrad"):
        return ((15, 0), (15, 0), None) if bf else ((31, 0), (31, -4 if k >= 1024 else 0), None)
    if family == "dtproj":
        if bf:
            return (15, 0), (15, 0), None
        return ((255, 0), (255, -4), None) if k <= 8 else ((63, 0), (63, -3), None) if k < 32 else ((31, 0), (31, -2), None)
    if family in ("xdt", "xdt_bwd", "proj"):
        # first product over k (dim forward, dim backward), second over k2 (rank forward, ncols backward)
        if family == "proj":                                      # dim 64: larger integers carry the results past the significand
            return ((30, 0), (15, 0), (3, 0)) if bf else ((62, 0), (31, -4), (15, -4))
        if bf:
            return (15, 0), (15, 0), (1 if k >= 1024 else 3, 0)
        return (31, 0), (31, -6 if k >= 1024 else -4), (3, -4)
    raise KeyError(family)


def exact_pair(g, m, n, k, ra, rb, dtype):
    a, b = ints(g, (m, k), *ra), ints(g, (n, k), *rb)
    assert torch.equal(a.to(dtype).double(), a) and torch.equal(b.to(dtype).double(), b), "operand not exact in the 16-bit type"
    return a, b


def quantum(*recipes):
    q = 0
    for r in recipes:
        q += r[1]
    return 2.0 ** q


# ---- aum_gemm_tn -----------------------------------------------------------------------------------------------------------------------
def gemm_operands(case, dtype, exact):
    m, n, k, pad_a, pad_c = case
    g = _gen("gemm", case, DT_ID[dtype], exact)
    if exact:
        ra, rb, _ = recipe("gemm", dtype, k)
        a_full, b = exact_pair(g, m, n, k + pad_a, ra, rb, dtype)
        b = b[:, :k].contiguous()
        q = quantum(ra, rb)
    else:                                                         # check_gemm's operands
        a_full, b, q = torch.randn(m, k + pad_a, generator=g).to(dtype).double(), (torch.randn(n, k, generator=g) / k ** 0.5).to(dtype).double(), None
    a = a_full[:, :k]
    return dict(a_full=a_full, a=a, b=b, ref=a @ b.t(), absum=a.abs() @ b.abs().t(), q=q)


def gemm_conditions(case, dtype):
    o = gemm_operands(case, dtype, True)
    return check_conditions(("gemm", case, DT_ID[dtype]), dtype, o["ref"], o["absum"], o["q"], family="gemm")


def run_gemm(lib, dev, case, dtype, o, flags):
    """the call of check_gemm: the result a column block of a wider buffer with rows behind it, all of which must come back untouched"""
    m, n, k, pad_a, pad_c = case
    a = o["a_full"].to(dtype).to(dev)[:, :k]
    b = o["b"].to(dtype).to(dev)
    c_buf = torch.full((m + 260, n + pad_c), SENTINEL, dtype=dtype, device=dev)
    out = aum_hip.gemm_tn(a, b, out=c_buf[:m][:, pad_c:], lib=lib, flags=flags)
    assert torch.all(c_buf[m:] == SENTINEL), "rows behind the result were written"
    assert torch.all(c_buf[:m, :pad_c] == SENTINEL), "columns outside the result were written"
    return out


def gemm_refused(lib, dev, case, dtype, flags):
    """the paced flag below its shortest product stays a refusal (nothing launched)"""
    import pytest
    if not (flags & aum_hip.GEMM_PACED and case[2] < PACED_MIN_K):
        return False
    with pytest.raises(RuntimeError):
        aum_hip.gemm_tn(torch.zeros(case[0], case[2], dtype=dtype, device=dev), torch.zeros(case[1], case[2], dtype=dtype, device=dev), lib=lib, flags=flags)
    return True


def check_gemm_exact(lib, dev, case, dtype, scheds=("auto",)):
    o = gemm_operands(case, dtype, True)
    want = rn16(o["ref"], dtype)
    outs = []
    for s in scheds:
        if dev != "cpu" and gemm_refused(lib, dev, case, dtype, SCHEDS[s]):
            continue
        out = run_gemm(lib, dev, case, dtype, o, SCHEDS[s])
        assert_bits(("gemm_tn exact", case, DT_ID[dtype], s), out, want)
        outs.append(out)
    return outs


def check_gemm_interval(lib, dev, case, dtype, scheds=("auto",)):
    o = gemm_operands(case, dtype, False)
    e = case[2] * 2.0 ** -23 * o["absum"]
    first = None
    for s in scheds:
        if dev != "cpu" and gemm_refused(lib, dev, case, dtype, SCHEDS[s]):
            continue
        out = run_gemm(lib, dev, case, dtype, o, SCHEDS[s])
        assert_interval(("gemm_tn interval", case, DT_ID[dtype], s), out, o["ref"], e, "gemm_tn")
        if first is None:
            first = out.clone()
        assert_bits(("gemm_tn schedules bit-equal", case, DT_ID[dtype], s), out, first)


# ---- aum_gemm_wgrad --------------------------------------------------------------------------------------------------------------------
def wgrad_operands(case, dtype, exact):
    t, n, k, splits, pad_y, pad_x = case
    g = _gen("wgrad", case, DT_ID[dtype], exact)
    if exact:
        ra, rb, _ = recipe("wgrad", dtype, t)
        y_full, x_full = ints(g, (t, n + pad_y), *ra), ints(g, (t, k + pad_x), *rb)
        q = quantum(ra, rb)
    else:                                                         # check_gemm_wgrad's operands
        y_full, x_full, q = torch.randn(t, n + pad_y, generator=g).to(dtype).double(), torch.randn(t, k + pad_x, generator=g).to(dtype).double(), None
    return dict(y_full=y_full, x_full=x_full, y=y_full[:, pad_y:], x=x_full[:, :k], q=q)


def wgrad_ranges(t, splits):
    chunk = (((t + splits - 1) // splits) + 63) // 64 * 64        # gemm_wgrad_assert's
    return [(min(s * chunk, t), min((s + 1) * chunk, t)) for s in range(splits)]


def wgrad_conditions(case, dtype):
    o = wgrad_operands(case, dtype, True)
    check_conditions(("wgrad", case, DT_ID[dtype]), dtype, o["y"].t() @ o["x"], o["y"].abs().t() @ o["x"].abs(), o["q"], rounded=False)


def _run_wgrad(lib, dev, case, dtype, o):
    t, n, k, splits, pad_y, pad_x = case
    y = o["y_full"].to(dtype).to(dev)[:, pad_y:]
    x = o["x_full"].to(dtype).to(dev)[:, :k]
    part = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib, partials=True)
    total = aum_hip.gemm_wgrad(y, x, splits=splits, lib=lib)
    assert part.shape == (splits, n, k) and part.dtype == torch.float32 and total.shape == (n, k) and total.dtype == torch.float32
    return part, total


def check_wgrad_exact(lib, dev, case, dtype):
    """every split's partial tile is the fp64 sum over its token range exactly (an empty split: +0 everywhere), and so is the total"""
    o = wgrad_operands(case, dtype, True)
    part, total = _run_wgrad(lib, dev, case, dtype, o)
    for s, (t0, t1) in enumerate(wgrad_ranges(case[0], case[3])):
        assert_bits(("gemm_wgrad exact partial", case, DT_ID[dtype], s), part[s], (o["y"][t0:t1].t() @ o["x"][t0:t1]).float())
    assert_bits(("gemm_wgrad exact total", case, DT_ID[dtype]), total, (o["y"].t() @ o["x"]).float())


def check_wgrad_interval(lib, dev, case, dtype):
    """e of a partial: its token count accumulations; of the total: those of the longest partial plus one per summed partial"""
    o = wgrad_operands(case, dtype, False)
    part, total = _run_wgrad(lib, dev, case, dtype, o)
    ya, xa = o["y"].abs(), o["x"].abs()
    longest = 0
    for s, (t0, t1) in enumerate(wgrad_ranges(case[0], case[3])):
        longest = max(longest, t1 - t0)
        assert_interval(("gemm_wgrad interval partial", case, DT_ID[dtype], s), part[s], o["y"][t0:t1].t() @ o["x"][t0:t1],
                        (t1 - t0) * 2.0 ** -23 * (ya[t0:t1].t() @ xa[t0:t1]), "gemm_wgrad")
    assert_interval(("gemm_wgrad interval total", case, DT_ID[dtype]), total, o["y"].t() @ o["x"],
                    (longest + case[3]) * 2.0 ** -23 * (ya.t() @ xa), "gemm_wgrad")


# ---- aum_dtproj_tm_fwd -----------------------------------------------------------------------------------------------------------------
def dtproj_operands(case, dtype, exact):
    ntok, dim, rank, ncols = case
    g = _gen("dtproj", case, DT_ID[dtype], exact)
    if exact:
        ra, rb, _ = recipe("dtproj", dtype, rank)
        x, w = ints(g, (ntok, ncols), *ra), ints(g, (dim, rank), *rb)           # the B | C columns hold integers too: they must not be read
        q = quantum(ra, rb)
    else:                                                         # check_dtproj's operands
        x, w, q = torch.randn(ntok, ncols, generator=g).to(dtype).double(), (torch.randn(dim, rank, generator=g) / rank ** 0.5).to(dtype).double(), None
    xr = x[:, :rank]
    return dict(x=x, w=w, ref=xr @ w.t(), absum=xr.abs() @ w.abs().t(), q=q)


def dtproj_conditions(case, dtype):
    o = dtproj_operands(case, dtype, True)
    return check_conditions(("dtproj", case, DT_ID[dtype]), dtype, o["ref"], o["absum"], o["q"], family="dtproj")


def _run_dtproj(lib, dev, case, dtype, o):
    return aum_hip.dtproj_tm_fwd(o["x"].to(dtype).to(dev), case[2], o["w"].to(dtype).to(dev), lib=lib)


def check_dtproj_exact(lib, dev, case, dtype):
    o = dtproj_operands(case, dtype, True)
    assert_bits(("dtproj_tm_fwd exact", case, DT_ID[dtype]), _run_dtproj(lib, dev, case, dtype, o), rn16(o["ref"], dtype))


def check_dtproj_interval(lib, dev, case, dtype):
    o = dtproj_operands(case, dtype, False)
    assert_interval(("dtproj_tm_fwd interval", case, DT_ID[dtype]), _run_dtproj(lib, dev, case, dtype, o), o["ref"],
                    case[2] * 2.0 ** -23 * o["absum"], "dtproj_tm_fwd")


# ---- aum_xdt_tm_fwd --------------------------------------------------------------------------------------------------------------------
def xdt_operands(case, dtype, exact):
    """u (ntok, dim), wx (ncols, dim), wdt (dim, rank); ncols 48: the padded Tiny layout through xdt_tiny_checks.pad_weights (built at its
    width 384; a narrower dim takes the first columns of w_x and rows of w_dt of that layout)"""
    ntok, dim, rank, ncols = case
    g = _gen("xdt", case, DT_ID[dtype], exact)
    tiny = ncols == XT.NCOLS
    wshape = ((XT.R + 2 * XT.N, XT.DIM), (XT.DIM, XT.R)) if tiny else ((ncols, dim), (dim, rank))
    if exact:
        ra, rb, rc = recipe("xdt", dtype, dim, rank)
        u, wx, wdt = ints(g, (ntok, dim), *ra), ints(g, wshape[0], *rb), ints(g, wshape[1], *rc)
        q1, q2 = quantum(ra, rb), quantum(ra, rb, rc)
    else:                                                         # check_xdt's operands
        u = torch.randn(ntok, dim, generator=g).to(dtype).double()
        wx = (torch.randn(*wshape[0], generator=g) / dim ** 0.5).to(dtype).double()
        wdt = (torch.randn(*wshape[1], generator=g) / rank ** 0.5).to(dtype).double()
        q1 = q2 = None
    if tiny:
        assert rank == XT.RP and dim <= XT.DIM
        wx, wdt = XT.pad_weights(wx, wdt)
        wx, wdt = wx[:, :dim].contiguous(), wdt[:dim].contiguous()
    return dict(u=u, wx=wx, wdt=wdt, q1=q1, q2=q2)


def xdt_expected(o, dtype, rank):
    """x_dbl: the rounded fp64 product; delta: the rounded fp64 product of THAT rounded x_dbl"""
    ref_x = o["u"] @ o["wx"].t()
    x16 = rn16(ref_x, dtype)
    xr = x16.double()[:, :rank]
    return dict(ref_x=ref_x, abs_x=o["u"].abs() @ o["wx"].abs().t(), x16=x16, ref_d=xr @ o["wdt"].t(), abs_d=xr.abs() @ o["wdt"].abs().t())


def xdt_conditions(case, dtype):
    o = xdt_operands(case, dtype, True)
    x = xdt_expected(o, dtype, case[2])
    a = check_conditions(("xdt x_dbl", case, DT_ID[dtype]), dtype, x["ref_x"], x["abs_x"], o["q1"], family="xdt x_dbl")
    b = check_conditions(("xdt delta", case, DT_ID[dtype]), dtype, x["ref_d"], x["abs_d"], o["q2"], family="xdt delta")
    # the test tells the rounded intermediate from the unrounded one: delta of the fp32 accumulators rounds elsewhere
    unrounded = rn16(x["ref_x"][:, :case[2]] @ o["wdt"].t(), dtype)
    assert (unrounded.view(torch.int16) != rn16(x["ref_d"], dtype).view(torch.int16)).float().mean().item() >= 0.01, (case, "delta does not see the intermediate rounding")
    return a, b


def _run_xdt(lib, dev, dtype, o, **kw):
    return aum_hip.xdt_tm_fwd(o["u"].to(dtype).to(dev), o["wx"].to(dtype).to(dev), o["wdt"].to(dtype).to(dev), lib=lib, **kw)


def check_xdt_exact(lib, dev, case, dtype):
    o = xdt_operands(case, dtype, True)
    x = xdt_expected(o, dtype, case[2])
    x_dbl, delta = _run_xdt(lib, dev, dtype, o)
    assert_bits(("xdt_tm_fwd exact x_dbl", case, DT_ID[dtype]), x_dbl, x["x16"])
    assert_bits(("xdt_tm_fwd exact delta", case, DT_ID[dtype]), delta, rn16(x["ref_d"], dtype))
    if not lib.host:             # the softplus form's x_dbl is the plain form's (its delta: tests/test_gpu_delta_activated.py)
        bias = torch.zeros(case[1], device=dev)
        xs, _ = _run_xdt(lib, dev, dtype, o, delta_bias=bias, delta_softplus=True)
        assert_bits(("xdt_tm_fwd softplus x_dbl", case, DT_ID[dtype]), xs, x_dbl)


def check_xdt_interval(lib, dev, case, dtype):
    """delta against the product of the kernel's OWN rounded x_dbl, as xdt_assert has it"""
    ntok, dim, rank, ncols = case
    o = xdt_operands(case, dtype, False)
    x_dbl, delta = _run_xdt(lib, dev, dtype, o)
    x = xdt_expected(o, dtype, rank)
    assert_interval(("xdt_tm_fwd interval x_dbl", case, DT_ID[dtype]), x_dbl, x["ref_x"], dim * 2.0 ** -23 * x["abs_x"], "xdt_tm_fwd x_dbl")
    xr = x_dbl.detach().cpu().double()[:, :rank]
    assert_interval(("xdt_tm_fwd interval delta", case, DT_ID[dtype]), delta, xr @ o["wdt"].t(), rank * 2.0 ** -23 * (xr.abs() @ o["wdt"].abs().t()),
                    "xdt_tm_fwd delta")


# ---- aum_xdt_tm_bwd --------------------------------------------------------------------------------------------------------------------
def xdt_bwd_operands(case, dtype, exact):
    ntok, dim, pad, ncols = case
    R = ncols - 32
    g = _gen("xdt_bwd", case, DT_ID[dtype], exact)
    if exact:
        ra, rb, rc = recipe("xdt_bwd", dtype, dim, ncols)
        ddf, duf = ints(g, (ntok, dim + pad), *ra), ints(g, (ntok, dim + pad), ra[0], ra[1] + rb[1] + rc[1])
        wdt_t, wx_t = ints(g, (R, dim), *rb), ints(g, (dim, ncols), *rc)
        dbc = ints(g, (ntok, 32), ra[0], ra[1] + rb[1])           # on the dt block's quantum, exact in the 16-bit type
        q1, q2 = quantum(ra, rb), quantum(ra, rb, rc)
    else:                                                         # check_xdt_bwd's operands
        ddf, duf = torch.randn(ntok, dim + pad, generator=g).to(dtype).double(), torch.randn(ntok, dim + pad, generator=g).to(dtype).double()
        dbc = torch.randn(ntok, 32, generator=g).float().double()
        wdt_t = (torch.randn(R, dim, generator=g) / dim ** 0.5).to(dtype).double()
        wx_t = (torch.randn(dim, ncols, generator=g) / ncols ** 0.5).to(dtype).double()
        q1 = q2 = None
    return dict(ddf=ddf, duf=duf, dd=ddf[:, :dim], du=duf[:, :dim], dbc=dbc, wdt_t=wdt_t, wx_t=wx_t, q1=q1, q2=q2, R=R)


def xdt_bwd_expected(o, dtype):
    ref_r = o["dd"] @ o["wdt_t"].t()
    dx16 = torch.cat([rn16(ref_r, dtype), rn16(o["dbc"], dtype)], dim=1)
    dx = dx16.double()
    return dict(ref_r=ref_r, abs_r=o["dd"].abs() @ o["wdt_t"].abs().t(), dx16=dx16, ref_u=o["du"] + dx @ o["wx_t"].t(),
                abs_u=o["du"].abs() + dx.abs() @ o["wx_t"].abs().t())


def xdt_bwd_conditions(case, dtype):
    o = xdt_bwd_operands(case, dtype, True)
    x = xdt_bwd_expected(o, dtype)
    assert torch.equal(rn16(o["dbc"], dtype).double(), o["dbc"]), "dbc not exact in the 16-bit type"
    a = check_conditions(("xdt_bwd dt block", case, DT_ID[dtype]), dtype, x["ref_r"], x["abs_r"], o["q1"], family="xdt_bwd dt block")
    b = check_conditions(("xdt_bwd du", case, DT_ID[dtype]), dtype, x["ref_u"], x["abs_u"], o["q2"], family="xdt_bwd du")
    return a, b


def _run_xdt_bwd(lib, dev, case, dtype, o):
    ntok, dim, pad, ncols = case
    ddf, duf = o["ddf"].to(dtype).to(dev), o["duf"].to(dtype).to(dev)
    tail = duf[:, dim:].clone()
    du = duf[:, :dim]
    dx = aum_hip.xdt_tm_bwd(ddf[:, :dim], o["dbc"].float().to(dev), o["wdt_t"].to(dtype).to(dev), o["wx_t"].to(dtype).to(dev), du, lib=lib)
    assert torch.equal(duf[:, dim:], tail), "columns behind the du rows were written"
    return dx, du


def check_xdt_bwd_exact(lib, dev, case, dtype):
    o = xdt_bwd_operands(case, dtype, True)
    x = xdt_bwd_expected(o, dtype)
    dx, du = _run_xdt_bwd(lib, dev, case, dtype, o)
    R = o["R"]
    assert_bits(("xdt_tm_bwd exact dB | dC block", case, DT_ID[dtype]), dx[:, R:], o["dbc"].to(dtype))
    assert_bits(("xdt_tm_bwd exact dt block", case, DT_ID[dtype]), dx[:, :R], x["dx16"][:, :R])
    assert_bits(("xdt_tm_bwd exact du", case, DT_ID[dtype]), du, rn16(x["ref_u"], dtype))


def check_xdt_bwd_interval(lib, dev, case, dtype):
    """du against du_in + the kernel's OWN rounded dx_dbl . W_x, as xdt_bwd_assert has it: ncols accumulations and the addition of du_in"""
    ntok, dim, pad, ncols = case
    o = xdt_bwd_operands(case, dtype, False)
    dx, du = _run_xdt_bwd(lib, dev, case, dtype, o)
    x = xdt_bwd_expected(o, dtype)
    R = o["R"]
    assert_bits(("xdt_tm_bwd dB | dC block", case, DT_ID[dtype]), dx[:, R:], o["dbc"].float().to(dtype))
    assert_interval(("xdt_tm_bwd interval dt block", case, DT_ID[dtype]), dx[:, :R], x["ref_r"], dim * 2.0 ** -23 * x["abs_r"], "xdt_tm_bwd dt block")
    dxd = dx.detach().cpu().double()
    assert_interval(("xdt_tm_bwd interval du", case, DT_ID[dtype]), du, o["du"] + dxd @ o["wx_t"].t(),
                    (ncols + 1) * 2.0 ** -23 * (o["du"].abs() + dxd.abs() @ o["wx_t"].abs().t()), "xdt_tm_bwd du")


# ---- aum_proj_fwd / _bwd_data / _bwd_weight (channel-major) ---------------------------------------------------------------------------
def proj_operands(case, dtype, exact):
    name, dim, R, Nst, batch, length = case
    ntok, rt = batch * length, R + 2 * Nst
    g = _gen("proj", case, DT_ID[dtype], exact)
    if exact:
        ra, rb, rc = recipe("proj", dtype, dim, R)
        conv, w_x, w_dt = ints(g, (dim, ntok), *ra), ints(g, (rt, dim), *rb), ints(g, (dim, R), *rc)
        ddelta, du = ints(g, (dim, ntok), *ra), ints(g, (dim, ntok), ra[0], ra[1] + rb[1] + rc[1])
        dB, dC = ints(g, (batch, Nst, length), ra[0], ra[1] + rc[1]), ints(g, (batch, Nst, length), ra[0], ra[1] + rc[1])
        q = dict(a=quantum(ra), x=quantum(ra, rb), d=quantum(ra, rb, rc), dx=quantum(ra, rc), dc=quantum(ra, rc, rb))
    else:                                                         # check_proj's operands
        r = lambda *s: torch.randn(*s, generator=g)
        conv, w_x, w_dt = r(dim, ntok).to(dtype).double(), (r(rt, dim) / dim ** 0.5).to(dtype).double(), (r(dim, R) / R ** 0.5).to(dtype).double()
        ddelta, du = r(dim, ntok).to(dtype).double(), r(dim, ntok).to(dtype).double()
        dB, dC = r(batch, Nst, length).float().double(), r(batch, Nst, length).float().double()
        q = None
    return dict(conv=conv, w_x=w_x, w_dt=w_dt, ddelta=ddelta, du=du, dB=dB, dC=dC, q=q)


def proj_expected(o, dtype, case):
    name, dim, R, Nst, batch, length = case
    ntok = batch * length
    flat = lambda t: t.transpose(0, 1).reshape(Nst, ntok)
    ref_x = o["w_x"] @ o["conv"]
    x16 = rn16(ref_x, dtype)
    xr = x16.double()[:R]
    ref_r = o["w_dt"].t() @ o["ddelta"]
    dx16 = torch.cat([rn16(ref_r, dtype), rn16(flat(o["dB"]), dtype), rn16(flat(o["dC"]), dtype)], dim=0)
    dx = dx16.double()
    return dict(ref_x=ref_x, abs_x=o["w_x"].abs() @ o["conv"].abs(), x16=x16, ref_d=o["w_dt"] @ xr, abs_d=o["w_dt"].abs() @ xr.abs(),
                ref_r=ref_r, abs_r=o["w_dt"].abs().t() @ o["ddelta"].abs(), dx16=dx16,
                ref_c=o["du"] + o["w_x"].t() @ dx, abs_c=o["du"].abs() + o["w_x"].abs().t() @ dx.abs(),
                ref_wx=dx @ o["conv"].t(), abs_wx=dx.abs() @ o["conv"].abs().t(), ref_wdt=o["ddelta"] @ xr.t(), abs_wdt=o["ddelta"].abs() @ xr.abs().t())


def proj_conditions(case, dtype):
    o = proj_operands(case, dtype, True)
    x, q, tag = proj_expected(o, dtype, case), o["q"], (case[0], DT_ID[dtype])
    check_conditions(("proj x_dbl",) + tag, dtype, x["ref_x"], x["abs_x"], q["x"], family="proj x_dbl")
    check_conditions(("proj delta",) + tag, dtype, x["ref_d"], x["abs_d"], q["d"], family="proj delta")
    check_conditions(("proj dx_dbl dt rows",) + tag, dtype, x["ref_r"], x["abs_r"], q["dx"], family="proj dx_dbl")
    check_conditions(("proj dconv",) + tag, dtype, x["ref_c"], x["abs_c"], q["dc"], family="proj dconv")
    # the weight gradients (fp32): dx_dbl (quantum q.dx) . conv (quantum q.a), ddelta (q.a) . rounded x_dbl (q.x)
    check_conditions(("proj dw_x",) + tag, dtype, x["ref_wx"], x["abs_wx"], q["dx"] * q["a"], rounded=False)
    check_conditions(("proj dw_dt",) + tag, dtype, x["ref_wdt"], x["abs_wdt"], q["x"] * q["a"], rounded=False)


def _run_proj(lib, dev, case, dtype, o):
    name, dim, R, Nst, batch, length = case
    act = lambda t: t.to(dtype).to(dev).contiguous()
    x_dbl, delta = aum_hip.proj_fwd(act(o["conv"]), act(o["w_x"]), act(o["w_dt"]), Nst, lib=lib)
    dconv = act(o["du"])
    dx_dbl = aum_hip.proj_bwd_data(act(o["ddelta"]), act(o["w_dt"].t()), act(o["w_x"].t()), o["dB"].float().to(dev), o["dC"].float().to(dev), dconv,
                                   length, lib=lib)
    dw_x = aum_hip.proj_bwd_weight(act(o["conv"]), dx_dbl, True, lib=lib)
    dw_dt = aum_hip.proj_bwd_weight(act(o["ddelta"]), x_dbl[:R], False, lib=lib)
    return x_dbl, delta, dx_dbl, dconv, dw_x, dw_dt


def check_proj_exact(lib, dev, case, dtype):
    """the chained expectations of the token-major kernels on channel-major operands: delta from the expected rounded x_dbl, dconv from
    the expected rounded dx_dbl, the fp32 weight gradients exact"""
    o = proj_operands(case, dtype, True)
    x, tag = proj_expected(o, dtype, case), (case[0], DT_ID[dtype])
    x_dbl, delta, dx_dbl, dconv, dw_x, dw_dt = _run_proj(lib, dev, case, dtype, o)
    assert_bits(("proj_fwd exact x_dbl",) + tag, x_dbl, x["x16"])
    assert_bits(("proj_fwd exact delta",) + tag, delta, rn16(x["ref_d"], dtype))
    assert_bits(("proj_bwd_data exact dx_dbl",) + tag, dx_dbl, x["dx16"])
    assert_bits(("proj_bwd_data exact dconv",) + tag, dconv, rn16(x["ref_c"], dtype))
    assert_bits(("proj_bwd_weight exact dw_x",) + tag, dw_x.contiguous(), x["ref_wx"].float())
    assert_bits(("proj_bwd_weight exact dw_dt",) + tag, dw_dt.contiguous(), x["ref_wdt"].float())


def check_proj_interval(lib, dev, case, dtype):
    name, dim, R, Nst, batch, length = case
    ntok, rt = batch * length, R + 2 * Nst
    o = proj_operands(case, dtype, False)
    x, tag = proj_expected(o, dtype, case), (case[0], DT_ID[dtype])
    x_dbl, delta, dx_dbl, dconv, dw_x, dw_dt = _run_proj(lib, dev, case, dtype, o)
    u = 2.0 ** -23
    c = lambda t: t.detach().cpu().double()
    assert_interval(("proj_fwd interval x_dbl",) + tag, x_dbl, x["ref_x"], dim * u * x["abs_x"], "proj x_dbl")
    xr = c(x_dbl)[:R]
    assert_interval(("proj_fwd interval delta",) + tag, delta, o["w_dt"] @ xr, R * u * (o["w_dt"].abs() @ xr.abs()), "proj delta")
    assert_interval(("proj_bwd_data interval dx_dbl dt rows",) + tag, dx_dbl[:R], x["ref_r"], dim * u * x["abs_r"], "proj dx_dbl")
    assert_bits(("proj_bwd_data dB | dC rows",) + tag, dx_dbl[R:], x["dx16"][R:])
    dx = c(dx_dbl)
    assert_interval(("proj_bwd_data interval dconv",) + tag, dconv, o["du"] + o["w_x"].t() @ dx, (rt + 1) * u * (o["du"].abs() + o["w_x"].abs().t() @ dx.abs()),
                    "proj dconv")
    # the weight gradients sum ntok products in token splits and the splits' partials after that: at most ntok + 64 additions
    assert_interval(("proj_bwd_weight interval dw_x",) + tag, dw_x.contiguous(), dx @ o["conv"].t(), (ntok + 64) * u * (dx.abs() @ o["conv"].abs().t()), "proj dw")
    assert_interval(("proj_bwd_weight interval dw_dt",) + tag, dw_dt.contiguous(), o["ddelta"] @ xr.t(), (ntok + 64) * u * (o["ddelta"].abs() @ xr.abs().t()), "proj dw")


# ---- Part C: edges ---------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = 40                       # six special rows and ordinary ones behind them
OVERFLOW_TAILS = (0, 1, 2, -1, 3)    # 32 * 2047 + 16 * these: 65504 (stays), 65520 (the tie to 2^16: inf), 65536 (inf), 65488 (a tie, down to 65472), 65552 (inf)


def _lowbit(x):
    """the value of the lowest set significand bit of every element of the fp64 tensor x (inf where x = 0)"""
    m, e = torch.frexp(x)
    M = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (M & -M).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())
    return torch.where(x == 0, torch.full_like(x, float("inf")), low)


def assert_rows_exact(name, a, b, ref):
    """every row's fp32 sum is exact in any order: sum |a b| < 2^24 quanta, a row's quantum = (lowest bit among its a) x (lowest among b)"""
    qa = _lowbit(a).min(dim=1).values
    qb = _lowbit(b).min().item()
    live = torch.isfinite(qa)
    absum = (a.abs() @ b.abs().t()).max(dim=1).values
    assert (absum[live] < 2.0 ** 24 * qa[live] * qb).all(), (name, "a row's fp32 sums are not exact in every order")
    assert torch.isfinite(ref.float()).all() and torch.equal(ref.float().double(), ref), (name, "a result is not an fp32 number")


def edge_family(family):
    """(m, n, k) of the product a (m, k) . b (n, k)^T the family's kernel forms, and the output columns that may overflow"""
    if family.startswith("gemm_"):
        return EDGE_ROWS, 256, 448
    return (EDGE_ROWS, 96, 24) if family == "dtproj" else (EDGE_ROWS, 80, 256)


XDT_EDGE_RANK = 24


def run_product(lib, dev, family, a, b, dtype, wdt=None):
    """out (m, n) = a . b^T through the family's kernel; xdt also returns delta = x_dbl[:, :24] . wdt^T"""
    t = lambda x: x.to(dtype).to(dev)
    assert torch.equal(a.to(dtype).double(), a) and torch.equal(b.to(dtype).double(), b), "operand not exact in the 16-bit type"
    if family.startswith("gemm_"):
        return aum_hip.gemm_tn(t(a), t(b), lib=lib, flags=SCHEDS[family[5:]]), None
    if family == "dtproj":
        g = _gen("edge filler", family, DT_ID[dtype])
        x = torch.cat([a, ints(g, (a.shape[0], 32), 15, 0)], dim=1)                   # B | C columns: not to be read
        return aum_hip.dtproj_tm_fwd(t(x), a.shape[1], t(b), lib=lib), None
    return aum_hip.xdt_tm_fwd(t(a), t(b), t(wdt), lib=lib)


def edge_operands(family, dtype):
    m, n, k = edge_family(family)
    g = _gen("edges", family, DT_ID[dtype])
    top = torch.finfo(dtype).max
    a, b = ints(g, (m, k), 15, 0), ints(g, (n, k), 15, 0)
    b[:, 2:4] = ints(g, (n, 2), 15, -6)                           # what the largest finite inputs meet: the products stay inside fp32
    b[:, 9::2] = b[:, 8::2]                                       # columns in equal pairs from 8 on: what the cancelling row meets
    over = torch.arange(n) >= n // 2 if family != "xdt" else torch.arange(n) >= 40          # xdt: B | C columns only, delta stays finite
    b[over, 0] = 2047.0 if dtype == FP16 else 255.0
    b[over, 1] = torch.tensor(OVERFLOW_TAILS, dtype=torch.float64)[torch.arange(n) % 5][over]
    a[:6] = 0
    v = ints(g, ((k - 8) // 2,), 15, 0)
    a[1, 8::2], a[1, 9::2] = v, -v                                # products cancel in pairs: exactly 0, the partial sums are not
    a[2, 0], a[2, 1] = 32, 16
    a[3, 0], a[3, 1] = -32, -16
    a[4, 0] = 64
    a[5, 2] = a[5, 3] = top
    wdt = ints(g, (k, XDT_EDGE_RANK), 3, -8) if family == "xdt" else None
    return a, b, wdt, over


def check_edges(lib, dev, family, dtype):
    """zero row and cancelling row: +0 as the bit pattern; fp16 results at and past the top of the range: what Tensor.to(float16) makes of the
    exact value; the largest finite inputs: finite fp32 sums, bit-equal"""
    a, b, wdt, over = edge_operands(family, dtype)
    ref = a @ b.t()
    assert_rows_exact(("edges", family, DT_ID[dtype]), a, b, ref)
    want = rn16(ref, dtype)
    assert (ref[:2] == 0).all() and (want[:2].view(torch.int16) == 0).all() and (a[1] != 0).sum() >= 16
    if dtype == FP16:
        cols = over.nonzero().flatten()
        tails = b[cols, 1]
        row = want[2, cols].double()
        assert (row[tails == 0] == FP16_MAX).all() and torch.isposinf(row[tails == 1]).all() and torch.isposinf(row[tails == 2]).all()
        assert (row[tails == -1] == 65472.0).all() and torch.isposinf(row[tails == 3]).all()
        assert torch.equal(want[3, cols].double(), -row) and torch.isinf(want[4, cols]).all()
        assert (ref[2, cols][tails == 1] == 65520.0).all()
    assert torch.isfinite(want[5]).all() and (want[5] != 0).sum() > want.shape[1] // 2 and ref[5].abs().max() > 0.25 * torch.finfo(dtype).max
    out, delta = run_product(lib, dev, family, a, b, dtype, wdt)
    assert_bits(("edges", family, DT_ID[dtype]), out, want)
    if family == "xdt":
        xr = want.double()[:, :XDT_EDGE_RANK]
        assert_rows_exact(("edges delta", DT_ID[dtype]), xr, wdt, xr @ wdt.t())
        assert_bits(("edges delta", DT_ID[dtype]), delta, rn16(xr @ wdt.t(), dtype))


def subnormal_operands(family, dtype):
    """rows 0 .. m/2: every a a 16-bit subnormal (integers times the type's smallest subnormal); the rest: subnormals at even k, the
    smallest normals times small integers at odd k; b scaled so that every result is a normal number of the type"""
    m, n, k = edge_family(family)
    g = _gen("subnormal", family, DT_ID[dtype])
    sub, tiny, up = (-24, -14, 10) if dtype == FP16 else (-133, -126, 120)
    a = ints(g, (m, k), 15, sub)
    mixed = ints(g, (m - m // 2, k // 2), 3, tiny)
    a[m // 2:, 1::2] = mixed
    b = ints(g, (n, k), 15, up)
    wdt = ints(g, (k, XDT_EDGE_RANK), 3, 0) if family == "xdt" else None
    is_sub = (a != 0) & (a.abs() < torch.finfo(dtype).tiny)
    assert is_sub[:m // 2].sum() > 0.8 * (m // 2) * k and is_sub[m // 2:, 0::2].any() and not is_sub[m // 2:, 1::2].any()
    return a, b, wdt, is_sub


def check_subnormal_inputs(lib, dev, family, dtype, flushed):
    """flushed=False: the contract -- exact products of the subnormal inputs, fp32 sums, one rounding.  flushed=True: the product of the
    operands with every 16-bit subnormal of a replaced by zero (rows of subnormals alone: +0), exactly."""
    a, b, wdt, is_sub = subnormal_operands(family, dtype)
    a_eff = torch.where(is_sub, torch.zeros_like(a), a) if flushed else a
    ref = a_eff @ b.t()
    assert_rows_exact(("subnormal inputs", family, DT_ID[dtype]), a_eff, b, ref)
    full = a @ b.t()
    nz = full[full != 0].abs()
    assert nz.min().item() >= torch.finfo(dtype).tiny and nz.max().item() < FP16_MAX, "a result outside the type's normal range"
    want = rn16(ref, dtype)
    out, delta = run_product(lib, dev, family, a, b, dtype, wdt)
    assert_bits(("subnormal inputs", family, DT_ID[dtype], "flushed" if flushed else "exact"), out, want)
    if family == "xdt":
        xr = want.double()[:, :XDT_EDGE_RANK]
        assert_rows_exact(("subnormal inputs delta", DT_ID[dtype]), xr, wdt, xr @ wdt.t())
        assert_bits(("subnormal inputs delta", DT_ID[dtype]), delta, rn16(xr @ wdt.t(), dtype))


# ---- reports ---------------------------------------------------------------------------------------------------------------------------
def print_shares():
    """the measured shares of Part A per output family and dtype (the table in the header): lowest and highest over the cases"""
    for (family, dtype), rows in sorted(SHARES.items(), key=lambda kv: (kv[0][0], DT_ID[kv[0][1]])):
        col = lambda i: f"{100 * min(r[i] for r in rows):.1f}-{100 * max(r[i] for r in rows):.1f} %"
        print(f"shares {family:18s} {DT_ID[dtype]}: inexact {col(0)}, ties {col(1)}, toward zero differs {col(2)}, half away differs {col(3)}")


def print_ratios():
    for family, r in sorted(RATIOS.items()):
        print(f"ratio {family:22s} {r:.3f}")
