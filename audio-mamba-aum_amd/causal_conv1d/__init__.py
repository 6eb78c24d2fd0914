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


def _check_seq_map(name, seq_map, total, cache):
    if not isinstance(seq_map, aum_hip.SeqMap):
        raise TypeError(f"{name}: seq_map must come from aum_hip.seq_map()")
    if seq_map.total != total:
        raise ValueError(f"{name}: seq_map describes {seq_map.total} packed tokens, got {total}")
    if max(seq_map.rows) >= cache.shape[0]:
        raise ValueError(f"{name}: seq_map names cache row {max(seq_map.rows)}, the pool has {cache.shape[0]} rows")


def causal_conv1d_update(x, conv_state, weight, bias=None, activation=None, *, seq_map=None):
    """Streaming inference (the wheel's function of the same name, call site MS:328-334).  x (batch, dim): one token; conv_state (batch, dim,
    width) is shifted left and extended by x IN PLACE; returns act(sum(conv_state * weight, -1) + bias) in x's dtype (aum_causal_conv1d_update;
    a cache that is not fp32 goes through an fp32 copy and is written back).  x (batch, dim, seqlen), as the wheel takes from 1.4 on:
    `seqlen` successive updates, returned as (batch, dim, seqlen) -- one launch (aum_conv1d_tm_chunk: the token-major (batch, seqlen, dim)
    storage is read in place when x is its transposed view, e.g. the x half of in_proj output rows) where that kernel takes the shape,
    token by token otherwise.
    seq_map (extension, keyword only; aum_hip.seq_map): PACKED SESSIONS -- x (1, dim, total) holds the new tokens of several sessions behind
    one another, conv_state (nrows, dim, width) is a pool of caches and session i advances row seq_map.rows[i] by seq_map.lens[i] tokens;
    the other rows are not touched.  One launch (aum_conv1d_tm_chunk_var) where that kernel takes the shape; otherwise a host loop over
    the sessions through this function (the lengths are host values: no synchronisation).  Returns (1, dim, total)."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish")
    silu = activation in ("silu", "swish")
    if seq_map is not None:
        if x.dim() != 3 or x.shape[0] != 1 or conv_state.dim() != 3:
            raise ValueError("causal_conv1d_update: with seq_map x is (1, dim, total) and conv_state the pool (nrows, dim, width)")
        _check_seq_map("causal_conv1d_update", seq_map, x.shape[2], conv_state)
    st = conv_state if conv_state.dtype == torch.float32 and conv_state.is_contiguous() else conv_state.float().contiguous()
    if seq_map is not None:
        xt = x[0].t()                                            # (total, dim) packed rows
        if seq_map.total and not aum_hip.conv1d_tm_chunk_var_supported(xt, st):
            xt = xt.contiguous()
        if seq_map.total == 0:
            out = x.new_empty(x.shape)
        elif aum_hip.conv1d_tm_chunk_var_supported(xt, st):
            out = aum_hip.conv1d_tm_chunk_var(xt, st, weight, bias, silu, seq_map).t().unsqueeze(0)
        else:
            outs, o = [], 0
            for n, r in zip(seq_map.lens, seq_map.rows):
                if n:
                    outs.append(causal_conv1d_update(x[:, :, o:o + n], st[r:r + 1], weight, bias, activation))
                o += n
            out = torch.cat(outs, dim=2)
    elif x.dim() == 3:
        xt = x.transpose(1, 2)                                   # (batch, seqlen, dim)
        if not aum_hip.conv1d_tm_chunk_supported(xt, st):        # channel-major storage or a misaligned view: token-major copy
            xt = xt.contiguous()
        if aum_hip.conv1d_tm_chunk_supported(xt, st):
            out = aum_hip.conv1d_tm_chunk(xt, st, weight, bias, silu).transpose(1, 2)
        else:
            out = torch.stack([aum_hip.conv1d_update(x[:, :, t], st, weight, bias, silu) for t in range(x.shape[2])], dim=2)
    else:
        out = aum_hip.conv1d_update(x, st, weight, bias, silu)
    if st is not conv_state:
        conv_state.copy_(st)
    return out
