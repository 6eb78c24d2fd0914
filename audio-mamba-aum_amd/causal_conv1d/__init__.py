"""Drop-in for the `causal_conv1d` wheel's public function used by the reference
(`from causal_conv1d import causal_conv1d_fn`, SSI:9, MS:14): depthwise causal conv + optional SiLU, HIP-backed."""
import torch

import aum_hip

__version__ = "1.1.3.post1+aum.gfx950"


class CausalConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias=None, activation=None):
        if activation not in (None, "silu", "swish"):
            raise NotImplementedError("activation must be None, silu, or swish")
        if x.stride(-1) != 1:
            x = x.contiguous()
        ctx.silu = activation in ("silu", "swish")
        ctx.save_for_backward(x, weight, bias)
        return aum_hip.conv1d_fwd(x, weight, bias, ctx.silu)

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias = ctx.saved_tensors
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        dx, dw, db = aum_hip.conv1d_bwd(x, weight, bias, dout.to(x.dtype), ctx.silu)
        return dx, dw.to(weight.dtype).reshape(weight.shape), (db.to(bias.dtype) if bias is not None else None), None


def causal_conv1d_fn(x, weight, bias=None, activation=None):
    """x: (batch, dim, seqlen); weight: (dim, width); bias: (dim,); activation: None | "silu" | "swish"."""
    return CausalConv1dFn.apply(x, weight, bias, activation)


class CausalConv1dPeeksFn(torch.autograd.Function):
    """aum_hip.conv1d_tm_peeks_fwd / conv1d_tm_peeks_bwd on (rows, dim) rows.  The parameter gradients are returned the ordinary way (no
    grad_home bucket destinations)."""

    @staticmethod
    def forward(ctx, x, weight, bias, silu, peek_every, seq_map):
        if x.stride(-1) != 1:
            x = x.contiguous()
        ctx.silu, ctx.peek_every, ctx.seq_map = silu, peek_every, seq_map
        ctx.save_for_backward(x, weight, bias)
        return aum_hip.conv1d_tm_peeks_fwd(x, weight, bias, silu, seq_map, peek_every)

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias = ctx.saved_tensors
        dx, dw, db = aum_hip.conv1d_tm_peeks_bwd(dout.to(x.dtype).contiguous(), x, weight, bias, ctx.silu, ctx.seq_map, ctx.peek_every)
        return dx, dw.to(weight.dtype).reshape(weight.shape), (None if bias is None else db.to(bias.dtype)), None, None, None


def causal_conv1d_peeks_fn(x, weight, bias=None, activation=None, peek_every=None, seq_map=None):
    """The causal conv over rows [column 0's tokens | cls | column 1's tokens | cls | ...]: row j of a sequence is a peek row iff
    (j + 1) % (peek_every + 1) == 0 -- it sees the last width - 1 committed rows and itself and does not enter the window of later rows;
    every sequence starts from a zero window.  Differentiable (HIP both ways).  x: token-major (batch, T, dim), or packed (total, dim)
    rows with seq_map; weight (dim, width <= 4) or (dim, 1, width).  Returns y in x's shape and dtype."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish")
    x2, m, shape = aum_hip.peeks_rows(x, seq_map, "causal_conv1d_peeks_fn")
    y = CausalConv1dPeeksFn.apply(x2, weight, bias, activation is not None, peek_every, m)
    return y if shape is None else y.reshape(*shape, y.shape[-1])


def causal_conv1d_peeks_ref(x, weight, bias=None, activation=None, peek_every=None, seq_map=None):
    """causal_conv1d_peeks_fn as a differentiable Python loop over the rows, in the dtype it is given (run it in float64 for an oracle)."""
    x2, m, shape = aum_hip.peeks_rows(x, seq_map, "causal_conv1d_peeks_ref")
    dim = x2.shape[1]
    w = weight.reshape(dim, -1).to(x2.dtype)
    outs, at = [], 0
    for n in m.lens:
        win = [torch.zeros(dim, dtype=x2.dtype, device=x2.device) for _ in range(w.shape[1] - 1)]
        for j in range(n):
            full = win + [x2[at + j]]
            pre = sum(w[:, k] * full[k] for k in range(w.shape[1]))
            if bias is not None:
                pre = pre + bias.to(pre.dtype)
            outs.append(torch.nn.functional.silu(pre) if activation is not None else pre)
            if (j + 1) % (peek_every + 1) != 0:
                win = full[1:]
        at += n
    y = torch.stack(outs) if outs else x2.new_zeros(x2.shape)
    return y if shape is None else y.reshape(*shape, y.shape[-1])


def causal_conv1d_update(x, conv_state, weight, bias=None, activation=None, *, seq_map=None):
    """Streaming inference (the wheel's function of the same name, call site MS:328-334).  x (batch, dim): one token; conv_state (batch, dim,
    width) is shifted left and extended by x IN PLACE; returns act(sum(conv_state * weight, -1) + bias) in x's dtype (aum_causal_conv1d_update;
    a cache that is not fp32 goes through an fp32 copy and is written back).  x (batch, dim, seqlen), as the wheel takes from 1.4 on:
    `seqlen` successive updates, returned as (batch, dim, seqlen) -- one launch (aum_conv1d_tm_chunk: the token-major (batch, seqlen, dim)
    storage is read in place when x is its transposed view, e.g. the x half of in_proj output rows) where that kernel takes the shape,
    token by token otherwise.
    seq_map (extension, keyword only; aum_hip.seq_map): PACKED SESSIONS -- x (1, dim, total) holds the new tokens of several sessions behind
    one another, conv_state (nrows, dim, width) is a pool of caches and session i advances row seq_map.rows[i] by seq_map.lens[i] tokens;
    the other rows are not touched.  One launch (aum_conv1d_tm_chunk_var) where that kernel takes the shape, a host loop over the sessions
    otherwise; returns (1, dim, total).  The wheel's layout over aum_hip.conv1d_stream, which picks the launch."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish")
    silu = activation in ("silu", "swish")
    if seq_map is not None:
        if x.dim() != 3 or x.shape[0] != 1 or conv_state.dim() != 3:
            raise ValueError("causal_conv1d_update: with seq_map x is (1, dim, total) and conv_state the pool (nrows, dim, width)")
        aum_hip.check_seq_map("causal_conv1d_update", seq_map, x.shape[2], conv_state.shape[0], x.device)
    if x.dim() != 3:
        return aum_hip.conv1d_stream(x, conv_state, weight, bias, silu)
    return aum_hip.conv1d_stream(x.transpose(1, 2), conv_state, weight, bias, silu, seq_map).transpose(1, 2)
