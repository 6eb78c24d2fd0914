"""Drop-in for the reference's mamba_ssm.ops.triton.layernorm
(/root/reference/vim-mamba_ssm/mamba_ssm/ops/triton/layernorm.py = "LN"): RMSNorm, rms_norm_fn, layer_norm_fn,
rms_norm_ref, layer_norm_ref with the same signatures and return conventions.  The fused residual-add + RMSNorm
forward/backward (LN:51-120, 180-290 in Triton upstream) is the hand-written gfx950 kernel pair behind
aum_rmsnorm_fwd / aum_rmsnorm_bwd.  No Triton is involved despite the module path (kept for import parity).
"""
import torch
import torch.nn.functional as F

import aum_hip


def _scaled(x, row_scale):
    """x with sample b multiplied by row_scale[b] (stochastic depth on the mixer output, MM:90): the torch statement of the factor"""
    return x if row_scale is None else x * row_scale.reshape((-1,) + (1,) * (x.dim() - 1)).to(x.dtype)


def layer_norm_ref(x, weight, bias, residual=None, eps=1e-6, prenorm=False, upcast=False, row_scale=None):
    """Pure-PyTorch LayerNorm with optional residual add (contract of LN:19-32)."""
    dtype = x.dtype
    if upcast:
        x, weight = x.float(), weight.float()
        bias = bias.float() if bias is not None else None
        residual = residual.float() if residual is not None else None
    x = _scaled(x, row_scale)
    if residual is not None:
        x = (x + residual).to(x.dtype)
    out = F.layer_norm(x.to(weight.dtype), x.shape[-1:], weight=weight, bias=bias, eps=eps).to(dtype)
    return (out, x) if prenorm else out


def rms_norm_ref(x, weight, bias, residual=None, eps=1e-6, prenorm=False, upcast=False, row_scale=None):
    """Pure-PyTorch RMSNorm with optional residual add (contract of LN:35-48).  row_scale: (batch,) factors on x, sample by sample, in
    front of the add (what DropPath does to the mixer output in training); None: no factor."""
    dtype = x.dtype
    if upcast:
        x, weight = x.float(), weight.float()
        bias = bias.float() if bias is not None else None
        residual = residual.float() if residual is not None else None
    x = _scaled(x, row_scale)
    if residual is not None:
        x = (x + residual).to(x.dtype)
    inv = torch.rsqrt(x.square().mean(dim=-1, keepdim=True) + eps)
    out = x * inv * weight
    if bias is not None:
        out = out + bias
    out = out.to(dtype)
    return (out, x) if prenorm else out


class LayerNormFn(torch.autograd.Function):
    """LN:380-461.  is_rms_norm=True is the HIP kernel pair; plain LayerNorm (never reached by AuM: rms_norm=True,
    MM:206) is composed from torch ops so the public function keeps working.
    row_scale (batch,) fp32: stochastic depth's per-sample factor on x, applied inside the kernels (aum_rmsnorm_drop_fwd / _bwd: a
    dropped sample's x is not read, its dx is +0); it needs the residual and receives no gradient.  None: the unscaled pair."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False,
                is_rms_norm=False, row_scale=None):
        if not is_rms_norm or bias is not None:
            raise NotImplementedError("HIP fused add+norm implements RMSNorm without bias (what AuM uses, MM:77-97)")
        if row_scale is not None and residual is None:
            raise ValueError("row_scale multiplies x on its way into the residual add: it needs a residual")
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        r2 = None
        if residual is not None:
            assert residual.shape == shape
            r2 = residual.reshape(-1, shape[-1])
            if r2.stride(-1) != 1:
                r2 = r2.contiguous()
        res_dtype = r2.dtype if r2 is not None else (torch.float32 if residual_in_fp32 else None)
        ctx.rows_per_scale = None
        if row_scale is None:
            y, rstd, res_out = aum_hip.rmsnorm_fwd(x2, weight, r2, eps, residual_dtype=res_dtype)
            ctx.save_for_backward(res_out, weight, rstd)
        else:
            if x.dim() < 2 or row_scale.shape != shape[:1]:
                raise ValueError(f"row_scale must be ({shape[0]},): one factor per sample of x {tuple(shape)}, not {tuple(row_scale.shape)}")
            ctx.rows_per_scale = x2.shape[0] // shape[0]
            y, rstd, res_out = aum_hip.rmsnorm_drop_fwd(x2, weight, r2, row_scale, ctx.rows_per_scale, eps)
            ctx.save_for_backward(res_out, weight, rstd, row_scale)
        ctx.shape, ctx.has_residual, ctx.prenorm, ctx.x_dtype = shape, residual is not None, prenorm, x.dtype
        ctx.wparam = weight
        y = y.reshape(shape)
        return (y, res_out.reshape(shape)) if prenorm else y

    @staticmethod
    def backward(ctx, dy, *args):
        x, weight, rstd = ctx.saved_tensors[:3]
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1:
            dy2 = dy2.contiguous()
        dres = None
        if ctx.prenorm and args[0] is not None:
            dres = args[0].reshape(-1, dy.shape[-1])
            if dres.stride(-1) != 1:
                dres = dres.contiguous()
            dres = dres.to(x.dtype)
        from mamba_ssm.ops.selective_scan_interface import _homed, grad_home
        home = grad_home(ctx.wparam)          # the weight gradient's place in a DistributedDataParallel bucket, if the parameter has one
        if ctx.rows_per_scale is None:
            dx, dw, dres_in = aum_hip.rmsnorm_bwd(dy2.to(ctx.x_dtype), x, weight, rstd, dres, ctx.has_residual,
                                                  x_dtype=ctx.x_dtype, dw_out=home)
        else:
            dx, dw, dres_in = aum_hip.rmsnorm_drop_bwd(dy2.to(ctx.x_dtype), x, weight, rstd, ctx.saved_tensors[3], ctx.rows_per_scale, dres,
                                                       x_dtype=ctx.x_dtype, dw_out=home)
        return (dx.reshape(ctx.shape), _homed(dw.to(weight.dtype), home), None,
                dres_in.reshape(ctx.shape) if ctx.has_residual else None, None, None, None, None, None)


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False,
                  is_rms_norm=False, row_scale=None):
    if is_rms_norm and bias is None:
        return LayerNormFn.apply(x, weight, bias, residual, eps, prenorm, residual_in_fp32, True, row_scale)
    if row_scale is not None:
        raise NotImplementedError("row_scale (stochastic depth inside the add + norm) exists for RMSNorm without bias, the HIP kernel pair")
    # plain LayerNorm / biased RMSNorm: off the AuM path; torch composition with the reference's return convention
    res_dtype = residual.dtype if residual is not None else (torch.float32 if residual_in_fp32 else x.dtype)
    pre = x.to(res_dtype) if residual is None else (x.float() + residual.float()).to(res_dtype)
    ref = rms_norm_ref if is_rms_norm else layer_norm_ref
    out = ref(pre.float(), weight.float(), bias.float() if bias is not None else None, eps=eps).to(x.dtype)
    return (out, pre) if prenorm else out


def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6, row_scale=None):
    return layer_norm_fn(x, weight, bias, residual, eps, prenorm, residual_in_fp32, True, row_scale)


def rms_norm_pool_ref(x, weight, residual, eps=1e-6, rows_per_sample=None):
    """Pure-PyTorch add + RMSNorm + mean over a sample's tokens, the statement of rms_norm_pool_fn: the norm in fp32 on x + residual, its rows
    rounded to x's dtype (the hidden_states the reference's final norm returns, MM:649-657), their mean (MM:669) added in fp32 and rounded
    once.  x (B, L, D), or (B L, D) with rows_per_sample = L -> (B, D)."""
    if x.dim() == 2:
        x, residual = (t.reshape(-1, rows_per_sample, t.shape[-1]) for t in (x, residual))
    z = x.float() + residual.float()
    y = (z * torch.rsqrt(z.square().mean(dim=-1, keepdim=True) + eps) * weight.float()).to(x.dtype)
    return (y.float().sum(dim=1) / x.shape[1]).to(x.dtype)


class RMSNormPoolFn(torch.autograd.Function):
    """aum_rmsnorm_pool_fwd / _bwd under autograd: x (B, L, D) bf16 / fp16 and the fp32 residual stream -> (B, D); gradients to x, the
    weight (into its gradient home where it has one) and the residual.  Without grad mode nothing is saved and the kernel only reads."""

    @staticmethod
    def forward(ctx, x, weight, residual, eps, rows_per_sample):
        cols = x.shape[-1]
        x2, r2 = x.reshape(-1, cols), residual.reshape(-1, cols)
        x2 = x2 if x2.stride(-1) == 1 else x2.contiguous()
        r2 = r2 if r2.stride(-1) == 1 else r2.contiguous()
        need = any(ctx.needs_input_grad)
        pooled, rstd, res_out = aum_hip.rmsnorm_pool_fwd(x2, weight, r2, rows_per_sample, eps, save=need)
        if need:
            ctx.save_for_backward(res_out, weight, rstd)
        ctx.shape, ctx.per, ctx.wparam = x.shape, rows_per_sample, weight
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        res_out, weight, rstd = ctx.saved_tensors
        from mamba_ssm.ops.selective_scan_interface import _homed, grad_home
        home = grad_home(ctx.wparam)
        dpooled = dpooled if dpooled.stride(-1) == 1 else dpooled.contiguous()
        dx, dw, dres = aum_hip.rmsnorm_pool_bwd(dpooled, res_out, weight, rstd, ctx.per, dw_out=home)
        return dx.reshape(ctx.shape), _homed(dw.to(weight.dtype), home), dres.reshape(ctx.shape), None, None


def rms_norm_pool_fn(x, weight, residual, eps=1e-6, rows_per_sample=None):
    """Fused final add + RMSNorm + mean over the tokens of each sample: what rms_norm_fn(x, weight, None, residual=residual).mean(dim=1)
    computes, without the (B, L, D) normalised tensor or its gradient ever existing.  x (B, L, D) -> (B, D); a (B L, D) x takes
    rows_per_sample = L.  x is bf16 / fp16 and the residual fp32 (the autocast residual stream); CPU tensors without a library that takes
    them run rms_norm_pool_ref."""
    if x.dim() == 3:
        if rows_per_sample not in (None, x.shape[1]):
            raise ValueError(f"rms_norm_pool_fn: rows_per_sample {rows_per_sample} against x {tuple(x.shape)}")
        rows_per_sample = x.shape[1]
    elif x.dim() != 2 or rows_per_sample is None or rows_per_sample < 1 or x.shape[0] % rows_per_sample:
        raise ValueError(f"rms_norm_pool_fn: x must be (B, L, D), or (B L, D) with rows_per_sample = L; got {tuple(x.shape)}, {rows_per_sample}")
    if residual is None or residual.shape != x.shape:
        raise ValueError("rms_norm_pool_fn: the residual stream is required, in x's shape")
    if x.device.type == "cpu" and not _host_library():
        return rms_norm_pool_ref(x, weight, residual, eps, rows_per_sample)
    return RMSNormPoolFn.apply(x, weight, residual, eps, rows_per_sample)


def _host_library():
    """whether aum_hip's library in use takes host tensors (the tests' lane-array build where libaum_hip.so would be)"""
    return aum_hip._product is not None and aum_hip._product.host


class RMSNorm(torch.nn.Module):
    """LN:481-502: .weight (ones), .bias = None, .eps; forward(x, residual=None, prenorm=False, residual_in_fp32=False)."""

    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False, row_scale=None):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, eps=self.eps, prenorm=prenorm,
                           residual_in_fp32=residual_in_fp32, row_scale=row_scale)
