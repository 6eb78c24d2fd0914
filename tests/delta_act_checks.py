"""Checks of the activated-delta path (AUM_XDT_DELTA_SOFTPLUS / AUM_SCAN_DELTA_ACTIVATED), shared by the host (lane-array build) and
the GPU test files: the token-major scans fed delta = softplus(raw + delta_bias) against the fp64 oracle fed the same activated delta, with
the backward's ddelta / ddelta_bias held to the RAW-space gradients (d delta * sigmoid(raw + bias))."""
import numpy as np
import torch

import aum_hip
import cases
import kernel_checks as KC
from oracle import oracle as O


def softplus64(x):
    """torch softplus(beta=1, threshold=20) (SSI:106-107) in fp64"""
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def check_scan_tm_activated(lib, dev, case, dtype, reverse=False, bidir=False, segments=1, tol=KC.TOL_BF16):
    """aum_scan_tm_fwd / _bwd (or the _seg_ forms) with delta_activated=True: delta = the 16-bit rounding of softplus(raw + bias) in fp64
    (what aum_xdt_tm_fwd writes, within its one rounding).  The bias is passed too and must NOT be added again."""
    name, batch, dim, length, dstate, has_z, has_D, has_bias, softplus = case
    assert has_z and softplus, "the activated path is the block's: z present, delta_softplus"
    d = cases.scan_inputs(*case)
    q = {k: KC.rq(d[k], dtype) for k in ("u", "delta", "z", "B", "C", "dout")}
    bias = d["delta_bias"] if has_bias else np.zeros(dim, np.float32)
    pre_act = q["delta"].astype(np.float64) + bias.astype(np.float64)[None, :, None]
    act = KC.rq(softplus64(pre_act).astype(np.float32), dtype)               # the activated delta as the x/dt kernel stores it
    rng = np.random.default_rng(7)
    A_b = (d["A"] * np.exp(rng.normal(0, 0.1, d["A"].shape))).astype(np.float32) if bidir else None
    tm = lambda a: None if a is None else KC.T(a, dev, dtype).transpose(1, 2).contiguous()
    u, z, dout = tm(d["u"]), tm(d["z"]), tm(d["dout"])
    xz = torch.cat([u, z], dim=2).contiguous()                               # the block's [x | z] rows
    u, z = xz[:, :, :dim], xz[:, :, dim:]
    dl = tm(act)
    bcm = torch.cat([tm(d["B"]), tm(d["C"])], dim=2).contiguous()
    Bm, Cm = bcm[:, :, :dstate], bcm[:, :, dstate:]
    A, D = KC.T(d["A"], dev), KC.T(d["D"], dev)
    bias_t = KC.T(d["delta_bias"], dev) if has_bias else None
    ck = aum_hip.scan_tm_ckpt(batch, length, dim, dstate, bidir, dev, lib=lib, dtype=dtype)
    ck.fill_(float("nan"))
    out, out_pre = aum_hip.scan_tm_fwd(u, dl, A, Bm, Cm, D, z, bias_t, True, reverse, KC.T(A_b, dev), want_out_pre=True, ckpt=ck, lib=lib,
                                       segments=segments, delta_activated=True)
    g = aum_hip.scan_tm_bwd(u, dl, A, Bm, Cm, D, z, bias_t, dout, out_pre, ck, True, reverse, KC.T(A_b, dev), lib=lib, segments=segments,
                            delta_activated=True)
    # oracle: the activated delta as it is (no bias, no softplus); ddelta chained through sigmoid(raw + bias) into raw space
    ref = O.scan_fwd(q["u"], act, d["A"], q["B"], q["C"], d["D"], q["z"], None, False, reverse, "f64")
    gr = O.scan_bwd(q["u"], act, d["A"], q["B"], q["C"], d["D"], q["z"], None, q["dout"], False, reverse, "f64")
    ref_out, ref_pre = ref["out"], ref["y_pre"]
    if bidir:
        rb = O.scan_fwd(q["u"], act, A_b, q["B"], q["C"], d["D"], q["z"], None, False, True, "f64")
        ref_out, ref_pre = ref_out + rb["out"], ref_pre + rb["y_pre"]
        gb = O.scan_bwd(q["u"], act, A_b, q["B"], q["C"], d["D"], q["z"], None, q["dout"], False, True, "f64")
        for k in ("du", "ddelta", "dB", "dC", "dD", "dz"):
            if gr.get(k) is not None:
                gr[k] = gr[k] + gb[k]
        gr["dA_b"] = gb["dA"]
    gr["ddelta"] = gr["ddelta"] * sigmoid64(pre_act)
    gr["ddelta_bias"] = gr["ddelta"].sum(axis=(0, 2))
    cm = lambda t: KC.N(t).transpose(0, 2, 1)
    pairs = {"out": (cm(out), ref_out), "out_pre": (cm(out_pre), ref_pre)}
    got = dict(du=cm(g["du"]), ddelta=cm(g["ddelta"]), dz=cm(g["dz"]), dA=KC.N(g["dA"]), dA_b=KC.N(g["dA_b"]),
               dB=KC.N(g["dBC"])[:, :, :dstate].transpose(0, 2, 1), dC=KC.N(g["dBC"])[:, :, dstate:].transpose(0, 2, 1), dD=KC.N(g["dD"]),
               ddelta_bias=KC.N(g["ddelta_bias"]))
    for k in ("du", "ddelta", "dA", "dA_b", "dB", "dC", "dD", "dz", "ddelta_bias"):
        if gr.get(k) is None or (k == "dD" and not has_D) or (k == "ddelta_bias" and not has_bias):
            assert got.get(k) is None, k
            continue
        pairs[k] = (got[k], gr[k])
    errs = KC._scan_errors(pairs)
    bad = {k: v for k, v in errs.items() if not (v < tol * (4 if k.split(":")[-1].startswith("d") else 1))}
    assert not bad, (name, str(dtype), "rev" if reverse else "fwd", "bidir" if bidir else "uni", segments, bad, errs)
    return errs
