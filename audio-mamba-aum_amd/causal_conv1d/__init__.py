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
