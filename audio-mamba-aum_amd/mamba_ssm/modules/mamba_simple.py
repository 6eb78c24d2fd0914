"""Drop-in for the reference's mamba_ssm.modules.mamba_simple.Mamba
(/root/reference/vim-mamba_ssm/mamba_ssm/modules/mamba_simple.py = "MS"): same constructor signature (MS:35-56),
parameter / sub-module names (the checkpoint contract: in_proj, conv1d, x_proj, dt_proj, out_proj, A_log, D, A_b_log,
and for v2 conv1d_b, x_proj_b, dt_proj_b, D_b), initialisation (MS:94-127) and forward dispatch (MS:169-311).

Differences: the kernels underneath are libaum_hip.so; Bi-Bi (v2) passes reverse=True instead of flipping xz and the
result (MS:229-246); single-token decoding (`step`, inference caches, MS:313-400) exists for the causal block
(bimamba_type="none") as the reference's element-wise composition -- AuM itself never passes inference_params
(MM:620-622).
"""
import collections
import contextlib
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from mamba_ssm.ops.selective_scan_interface import (InProjFn, bimamba_inner_fn, mamba_inner_fn, mamba_inner_fn_no_out_proj,
                                                    neg_exp, selective_scan_fn)
import mamba_ssm.ops.selective_scan_interface as ssi
from causal_conv1d import causal_conv1d_fn, causal_conv1d_update
from mamba_ssm.ops.triton.selective_state_update import selective_state_update


# What streaming inference reads of a block's parameters, converted ONCE (Mamba.stream_params): conv_w (E, width) / conv_b fp32 contiguous and
# 16-byte aligned, A = -exp(A_log) (E, N), D, dt_bias fp32, w_x = x_proj.weight and w_dt = dt_proj.weight in the working 16-bit (or fp32) dtype.
# b_off: the column of B in the rows w_x produces (C follows at b_off + d_state) and the rank w_dt contracts: dt_rank, except in the PADDED
# layout of a 16-bit plan whose dt_rank is no multiple of 8 (AuM-Tiny: 12), where w_x (48, E) is [dt 12 | 4 zero rows | B 16 | C 16] and
# w_dt (E, 16) has zero columns 12..15 -- the x/dt kernels' 48-column width.  The pad columns of x_dbl are exact zeros and add +0 terms to
# delta: the numbers are those of the unpadded products.
StreamParams = collections.namedtuple("StreamParams", "conv_w conv_b A D dt_bias w_x w_dt dtype b_off")


class Mamba(nn.Module):
    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1,
                 dt_init="random", dt_scale=1.0, dt_init_floor=1e-4, conv_bias=True, bias=False, use_fast_path=True,
                 layer_idx=None, device=None, dtype=None, bimamba_type="none", if_devide_out=False,
                 init_layer_scale=None):
        fk = {"device": device, "dtype": dtype}
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = int(expand * d_model)
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.use_fast_path, self.layer_idx = use_fast_path, layer_idx
        self.bimamba_type, self.if_devide_out = bimamba_type, if_devide_out
        self.init_layer_scale = init_layer_scale
        if init_layer_scale is not None:
            self.gamma = nn.Parameter(init_layer_scale * torch.ones(d_model), requires_grad=True)

        self.in_proj = nn.Linear(d_model, self.d_inner * 2, bias=bias, **fk)
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, d_conv, groups=self.d_inner, padding=d_conv - 1,
                                bias=conv_bias, **fk)
        self.activation = "silu"
        self.act = nn.SiLU()
        self.x_proj = nn.Linear(self.d_inner, self.dt_rank + 2 * d_state, bias=False, **fk)
        self.dt_proj = nn.Linear(self.dt_rank, self.d_inner, bias=True, **fk)
        self._init_dt(self.dt_proj, dt_init, dt_scale, dt_min, dt_max, dt_init_floor, fk)
        self.A_log = self._make_A_log(device)
        self.D = nn.Parameter(torch.ones(self.d_inner, device=device))          # fp32 skip, MS:126
        self.D._no_weight_decay = True

        if bimamba_type in ("v1", "v2"):
            self.A_b_log = self._make_A_log(device)                              # MS:130-147
        if bimamba_type == "v2":                                                 # MS:149-165
            self.conv1d_b = nn.Conv1d(self.d_inner, self.d_inner, d_conv, groups=self.d_inner, padding=d_conv - 1,
                                      bias=conv_bias, **fk)
            self.x_proj_b = nn.Linear(self.d_inner, self.dt_rank + 2 * d_state, bias=False, **fk)
            self.dt_proj_b = nn.Linear(self.dt_rank, self.d_inner, bias=True, **fk)
            self.D_b = nn.Parameter(torch.ones(self.d_inner, device=device))
            self.D_b._no_weight_decay = True
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=bias, **fk)

    # ---- initialisers (MS:94-123) ----------------------------------------------------------------
    def _init_dt(self, dt_proj, dt_init, dt_scale, dt_min, dt_max, dt_init_floor, fk):
        std = self.dt_rank ** -0.5 * dt_scale
        if dt_init == "constant":
            nn.init.constant_(dt_proj.weight, std)
        elif dt_init == "random":
            nn.init.uniform_(dt_proj.weight, -std, std)
        else:
            raise NotImplementedError
        # bias such that softplus(bias) is log-uniform in [dt_min, dt_max]
        dt = torch.exp(torch.rand(self.d_inner, **fk) * (math.log(dt_max) - math.log(dt_min))
                       + math.log(dt_min)).clamp(min=dt_init_floor)
        with torch.no_grad():
            dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))
        dt_proj.bias._no_reinit = True

    def _make_A_log(self, device):
        A = torch.arange(1, self.d_state + 1, dtype=torch.float32, device=device).repeat(self.d_inner, 1)
        p = nn.Parameter(torch.log(A))       # S4D-real, kept in fp32
        p._no_weight_decay = True
        return p

    # ---- forward (MS:169-311) ---------------------------------------------------------------------
    def forward(self, hidden_states, inference_params=None, *, time_reversed=False, peek_every=None):
        """MS:169.  `time_reversed` (extension, keyword only): the block applied to the time-reversed sequence and reversed
        back, flip(forward(flip(h))), without the copies -- the odd layers of an `if_bidirectional` model (MM:623-638): every stage but
        the conv and the scan is token-wise, and those two take a direction flag.
        `peek_every`=P (extension, keyword only; causal block, no caches): timeline training -- see forward_peeks."""
        if peek_every is not None:
            if inference_params is not None or time_reversed:
                raise ValueError("forward(peek_every=) takes neither inference_params nor time_reversed")
            return self.forward_peeks(hidden_states, peek_every)
        conv_state = ssm_state = None
        if time_reversed and (inference_params is not None or not self.use_fast_path):
            return self.forward(hidden_states.flip([1]), inference_params).flip([1])
        if inference_params is not None:                                   # streaming inference, MS:176-182
            if self.bimamba_type != "none":
                raise NotImplementedError("inference caches only make sense for the causal (bimamba_type='none') block")
            conv_state, ssm_state = self._get_states_from_cache(inference_params, hidden_states.shape[0])
            if inference_params.seqlen_offset > 0:                         # states updated in place
                if hidden_states.dim() == 3 and hidden_states.shape[1] > 1:
                    out, _, _ = self.step_chunk(hidden_states, conv_state, ssm_state)
                else:
                    out, _, _ = self.step(hidden_states, conv_state, ssm_state)
                return out
            # seqlen_offset == 0 (MS:268-271, 300-302): the prompt runs as one sequence and leaves both caches behind.  Where the
            # token-major kernels take the block's shapes that is prefill_chunk on the zeroed caches; elsewhere the un-fused branch below
            if self._prefill_ok(hidden_states, conv_state, ssm_state):
                conv_state.zero_()
                ssm_state.zero_()
                out, _, _ = self.prefill_chunk(hidden_states, conv_state, ssm_state)
                return out if self.init_layer_scale is None else out * self.gamma
        batch, seqlen, _ = hidden_states.shape
        tm = (ssi.TOKEN_MAJOR and self.use_fast_path and inference_params is None
              and not (ssi._REF_DZ_DROP and self.bimamba_type == "v1")      # that option lives in the channel-major block
              and ssi.token_major_preferred(batch, self.d_inner, self.bimamba_type != "none", seqlen=seqlen)
              and ssi.token_major_ok(self.d_inner, self.d_state, self.d_conv, self.dt_rank,
                                     torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else hidden_states.dtype))
        if tm:
            # token-major block: xz rows [x | z] as the GEMM writes them; (B, 2E, L) is the transposed VIEW the interface expects
            xz = ssi.InProjTmFn.apply(self.in_proj.weight, hidden_states.reshape(batch * seqlen, -1))
            xz = xz.view(batch, seqlen, -1).transpose(1, 2)
        else:
            # matmul + transpose in one GEMM: xz is (B, 2E, L) stored channel-major, like MS:185-189
            xz = InProjFn.apply(self.in_proj.weight, hidden_states.reshape(batch * seqlen, -1))
            xz = xz.reshape(-1, batch, seqlen).permute(1, 0, 2)
        if self.in_proj.bias is not None:
            xz = xz + self.in_proj.bias.to(xz.dtype)[None, :, None]
        A = neg_exp(self.A_log)
        if self.use_fast_path and inference_params is None:                # MS:190
            if self.bimamba_type == "v1":
                A_b = neg_exp(self.A_b_log)
                out = bimamba_inner_fn(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight,
                                       self.dt_proj.weight, self.out_proj.weight, self.out_proj.bias, A, A_b, None,
                                       None, self.D.float(), delta_bias=self.dt_proj.bias.float(),
                                       delta_softplus=True, reverse=time_reversed)
            elif self.bimamba_type == "v2":
                A_b = neg_exp(self.A_b_log)
                # Bi-Bi's two pipelines are independent until their outputs are added; each is one-direction launches of 1 536 waves at
                # the bench shape (half of what the time-serial kernels hold), so the two run next to each other on two side streams
                # (forward here; autograd runs each pipeline's backward on the stream its forward ran on; why BOTH leave the calling
                # stream: ssi.side_streams).  AUM_V2_STREAMS=0: in line.
                two = tm and xz.is_cuda and ssi.v2_two_streams(tuple(self.parameters()), module=self)
                if two:
                    main = torch.cuda.current_stream(xz.device)
                    s_f, s_b = ssi.side_streams(xz.device)
                    s_f.wait_stream(main)
                    s_b.wait_stream(main)
                    for t_ in (xz, A, A_b):
                        t_.record_stream(s_f)
                        t_.record_stream(s_b)
                with (torch.cuda.stream(s_f) if two else contextlib.nullcontext()):
                    out_f = mamba_inner_fn_no_out_proj(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight,
                                                       self.dt_proj.weight, A, None, None, self.D.float(),
                                                       delta_bias=self.dt_proj.bias.float(), delta_softplus=True,
                                                       reverse=time_reversed)
                with (torch.cuda.stream(s_b) if two else contextlib.nullcontext()):
                    out_b = mamba_inner_fn_no_out_proj(xz, self.conv1d_b.weight, self.conv1d_b.bias,
                                                       self.x_proj_b.weight, self.dt_proj_b.weight, A_b, None, None,
                                                       self.D_b.float(), delta_bias=self.dt_proj_b.bias.float(),
                                                       delta_softplus=True, reverse=not time_reversed)
                if two:
                    main.wait_stream(s_f)
                    main.wait_stream(s_b)
                    out_f.record_stream(main)          # allocated on the side streams, consumed on the calling one
                    out_b.record_stream(main)
                y = out_f + out_b                                          # (B, E, L) logical, both in xz's storage order
                if self.if_devide_out:
                    y = y / 2
                out = ssi.out_proj_shared(self.out_proj.weight, y, tm)      # (B*L, D): the SSI:517 dispatch in y's storage order
                if self.out_proj.bias is not None:
                    out = out + self.out_proj.bias.to(out.dtype)
                out = out.reshape(batch, seqlen, -1)
            else:
                out = mamba_inner_fn(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight,
                                     self.dt_proj.weight, self.out_proj.weight, self.out_proj.bias, A, None, None,
                                     self.D.float(), delta_bias=self.dt_proj.bias.float(), delta_softplus=True,
                                     reverse=time_reversed)
        else:       # un-fused composition of the same ops (MS:264-308)
            x, z = xz.chunk(2, dim=1)
            if conv_state is not None:                                     # MS:268-271: the last d_conv inputs
                conv_state.copy_(F.pad(x, (self.d_conv - x.shape[-1], 0)))
            x = causal_conv1d_fn(x, self.conv1d.weight.reshape(self.d_inner, -1), self.conv1d.bias, self.activation)
            x_dbl = self.x_proj(x.transpose(1, 2).reshape(batch * seqlen, -1))
            dt, Bm, Cm = torch.split(x_dbl, [self.dt_rank, self.d_state, self.d_state], dim=-1)
            dt = (self.dt_proj.weight.to(dt.dtype) @ dt.t()).reshape(-1, batch, seqlen).permute(1, 0, 2)
            Bm = Bm.reshape(batch, seqlen, -1).transpose(1, 2).contiguous()
            Cm = Cm.reshape(batch, seqlen, -1).transpose(1, 2).contiguous()
            y = selective_scan_fn(x, dt.to(x.dtype), A, Bm.to(x.dtype), Cm.to(x.dtype), self.D.float(),
                                  z=z.to(x.dtype), delta_bias=self.dt_proj.bias.float(), delta_softplus=True,
                                  return_last_state=ssm_state is not None)
            if ssm_state is not None:                                      # MS:300-302
                y, last_state = y
                ssm_state.copy_(last_state)
            out = self.out_proj(y.transpose(1, 2))
        if self.init_layer_scale is not None:
            out = out * self.gamma
        return out

    def forward_peeks(self, hidden_states, peek_every):
        """The causal block on (batch, T, d_model) rows [P tokens | peek row | P tokens | peek row | ...] from the start of a clip,
        differentiable: what step_chunk(peek_every=P) computes from zeroed caches, with gradients.  Row j is a peek row iff
        (j + 1) % (P + 1) == 0: it sees the conv window and the state of the committed rows in front of it and enters neither.
            in_proj -> causal_conv1d_peeks_fn -> x_proj / dt_proj -> selective_scan_peeks_fn -> out_proj
        The projections are ordinary differentiable products (the fused x/dt kernels are written for the offline block's operand
        layout and are not used here); the conv and the scan are HIP both ways.  ssi.peeks_on_ref(): the two on their pure-torch twins."""
        if self.bimamba_type != "none":
            raise NotImplementedError("forward(peek_every=) needs the causal (bimamba_type='none') block")
        if isinstance(peek_every, bool) or not isinstance(peek_every, int) or peek_every < 1:
            raise ValueError(f"forward: peek_every is the number of committed rows before each peek row, an int >= 1, not {peek_every!r}")
        if hidden_states.dim() != 3 or hidden_states.shape[1] < 1:
            raise ValueError("forward(peek_every=): hidden_states must be (batch, T >= 1, d_model)")
        E, N, R = self.d_inner, self.d_state, self.dt_rank
        xz = self.in_proj(hidden_states)                                            # (batch, T, 2E): rows [x | z]
        x, z = xz[..., :E], xz[..., E:]
        xc = ssi.conv_peeks(x, self.conv1d.weight.reshape(E, self.d_conv), self.conv1d.bias, self.activation, peek_every)
        x_dbl = self.x_proj(xc)
        dt = F.linear(x_dbl[..., :R], self.dt_proj.weight)                          # the bias and the softplus are the scan's
        y = ssi.scan_peeks(xc, dt.to(xc.dtype), neg_exp(self.A_log), x_dbl[..., R:R + N].to(xc.dtype), x_dbl[..., R + N:R + 2 * N].to(xc.dtype),
                           self.D.float(), z.to(xc.dtype), self.dt_proj.bias.float(), True, peek_every)
        out = self.out_proj(y)
        return out if self.init_layer_scale is None else out * self.gamma

    def step(self, hidden_states, conv_state, ssm_state):
        """One token of streaming inference for the causal block (MS:313-358): (batch, 1, d_model) in, (batch, 1, d_model) out, the caches
        conv_state (batch, d_inner, d_conv) and ssm_state (batch, d_inner, d_state) advanced in place -- the block's four stages on a
        sequence of length one, the two recurrent ones on the library's per-token kernels (round 4):
            xc = causal_conv1d_update(x, conv_state, w, b, silu)                 window <- last d_conv inputs; silu(<window, w> + b)
            (dt, B, C) = x_proj(xc);   dt = dt W_dt^T                            (bias and softplus inside the state update, MS:340)
            y = selective_state_update(ssm_state, xc, dt, A, B, C, D, z, dt_bias, softplus)
            out = out_proj(y)"""
        if hidden_states.dim() != 3 or hidden_states.shape[1] != 1:
            raise ValueError("step() advances the caches by exactly one token: hidden_states must be (batch, 1, d_model)")
        E, N, R = self.d_inner, self.d_state, self.dt_rank
        x_new, z = self.in_proj(hidden_states[:, 0]).split(E, dim=-1)
        xc = causal_conv1d_update(x_new, conv_state, self.conv1d.weight.view(E, self.d_conv), self.conv1d.bias, self.activation)
        proj = self.x_proj(xc)
        dt_in, B_t, C_t = proj[:, :R], proj[:, R:R + N], proj[:, R + N:R + 2 * N]
        dt = F.linear(dt_in, self.dt_proj.weight)                                   # the bias is not added here (MS:340)
        y = selective_state_update(ssm_state, xc, dt, -torch.exp(self.A_log.float()), B_t, C_t, self.D, z=z, dt_bias=self.dt_proj.bias,
                                   dt_softplus=True)
        return self.out_proj(y).unsqueeze(1), conv_state, ssm_state

    def _stream_sources(self):
        return (self.conv1d.weight, self.conv1d.bias, self.A_log, self.D, self.dt_proj.bias, self.x_proj.weight, self.dt_proj.weight)

    @torch.no_grad()
    def stream_params(self, dtype=None):
        """The parameters as step_chunk reads them (StreamParams), converted once and cached: a hop through 24 blocks otherwise spends
        144 launches on fp32 copies and 48 on rebuilding A = -exp(A_log) (profiles/r07_stream_hop.txt).  dtype: the working dtype of the
        activations (default: in_proj.weight's).  The cache is keyed on every source parameter's identity, _version, dtype and device and
        on dtype: an optimizer step, load_state_dict, .to() or .half() rebuild it, nothing else does.  A write through `p.data` does not
        move `_version`: write under torch.no_grad() instead, as the optimizers do, or call invalidate_stream_params() behind such a
        write.  The tensors are shared between calls: do not write to them."""
        import aum_hip
        dtype = self.in_proj.weight.dtype if dtype is None else dtype
        key = (dtype,) + tuple(None if p is None else (id(p), p._version, p.dtype, p.device) for p in self._stream_sources())
        hit = self.__dict__.get("_stream_params")
        if hit is not None and hit[0] == key:
            return hit[1]
        E, N, R = self.d_inner, self.d_state, self.dt_rank
        w_x, w_dt, b_off = self.x_proj.weight.detach().to(dtype), self.dt_proj.weight.detach().to(dtype), R
        Rp = -(-R // 8) * 8
        if Rp != R and dtype in (torch.bfloat16, torch.float16) and N == 16 and aum_hip.xdt_fwd_shape_ok(Rp + 2 * N, E):
            # the padded layout (StreamParams): only where the kernels take the padded shape and would refuse the plain one
            px, pdt = w_x.new_zeros(Rp + 2 * N, E), w_dt.new_zeros(E, Rp)
            px[:R], px[Rp:] = w_x[:R], w_x[R:]
            pdt[:, :R] = w_dt
            w_x, w_dt, b_off = px, pdt, Rp
        plan = StreamParams(aum_hip._al16(aum_hip._f32c(self.conv1d.weight.reshape(E, -1))), aum_hip._al16(aum_hip._f32c(self.conv1d.bias)),
                            -torch.exp(self.A_log.float()), aum_hip._f32c(self.D), aum_hip._f32c(self.dt_proj.bias), w_x, w_dt, dtype, b_off)
        self.__dict__["_stream_params"] = (key, plan)
        return plan

    def invalidate_stream_params(self):
        """drop the cached stream_params(): the next call converts the parameters again (behind a write the key cannot see: `p.data`).
        Moves this block's generation, which a cached AudioMamba.stream_stack() compares: it is rebuilt as well."""
        self.__dict__.pop("_stream_params", None)
        self.__dict__["_stream_gen"] = self.__dict__.get("_stream_gen", 0) + 1

    @staticmethod
    def _check_packed(what, hidden_states, conv_state, ssm_state, seq_map):
        """The entry check of the packed form of `what` (step_chunk / prefill_chunk with a seq_map): hidden_states (1, total, d_model),
        pools of one size, and the map against them (aum_hip.check_seq_map, once per call) -> False where the map holds no token."""
        import aum_hip
        if hidden_states.dim() != 3 or hidden_states.shape[0] != 1 or conv_state.shape[0] != ssm_state.shape[0]:
            raise ValueError(f"{what}(seq_map=): hidden_states (1, total, d_model), pools of one size, not {conv_state.shape[0]} / {ssm_state.shape[0]} rows")
        aum_hip.check_seq_map(what, seq_map, hidden_states.shape[1], conv_state.shape[0], hidden_states.device)
        return seq_map.total != 0

    def _xdt_stage(self, xc2, plan):
        """The x/dt stage of step_chunk's ladder and of both prefill bodies: the contiguous (ntok, E) conv output -> (delta (ntok, E), B and
        C (ntok, N) as column views of the x_dbl rows, activated).  One fused launch where aum_xdt_tm_fwd takes the shape -- delta then
        carries dt_bias and the softplus (activated) -- else x_proj and dt_proj from the library, cast to the working dtype, bias and
        softplus left to the scan (MS:340).  How the scan is told is the caller's: the scans' operand checks differ."""
        import aum_hip
        N, R = self.d_state, self.dt_rank
        if xc2.is_cuda and aum_hip.xdt_tm_supported(xc2, plan.w_x, plan.w_dt):
            proj, delta = aum_hip.xdt_tm_fwd(xc2, plan.w_x, plan.w_dt, delta_bias=plan.dt_bias, delta_softplus=True)
            Bo, activated = plan.b_off, True                                    # plan.w_x's rows may be padded (StreamParams) ...
        else:
            proj = self.x_proj(xc2)
            delta = F.linear(proj[:, :R], self.dt_proj.weight)
            proj, delta = proj.to(xc2.dtype), delta.to(xc2.dtype)
            Bo, activated = R, False                                            # ... x_proj's are not
        return delta, proj[:, Bo:Bo + N], proj[:, Bo + N:Bo + 2 * N], activated

    def step_chunk(self, hidden_states, conv_state, ssm_state, seq_map=None, commit=True, peek=False, peek_every=None):
        """T >= 1 tokens of streaming inference for the causal block in one pass: (batch, T, d_model) in, (batch, T, d_model) out, the
        caches advanced in place by T tokens -- what T calls of step() compute, with the projections as one small GEMM each and the
        recurrent middle as ONE launch where aum_hip.stream_block takes the shapes (16-bit activations, fp32 caches, the widths of
        aum_xdt_tm_fwd, at most 128 tokens per session), else as the ladder (the result does not depend on how a stream is cut into chunks):
            xz = in_proj(h)                                                      (batch, T, 2E) token-major rows [x | z]
            xc = aum_hip.conv1d_stream(x half in place, conv_state, w, b, silu)  T window updates (causal_conv1d_update, token-major)
            (dt, B, C) = x_proj(xc);  delta = dt W_dt^T                          (one fused launch where aum_xdt_tm_fwd takes the shape)
            y = aum_hip.scan_stream(ssm_state, xc, delta, A, B, C, D, z half, dt_bias, softplus)        (selective_scan_update)
            out = out_proj(y)
        Both give the same bits.  The per-call parameter conversions come from stream_params() on every path.
        seq_map (aum_hip.seq_map): PACKED SESSIONS at different positions in one pass -- hidden_states (1, total, d_model) holds the new
        tokens of several sessions behind one another, the caches are pools of nrows rows, session i advances row seq_map.rows[i] by
        seq_map.lens[i] tokens (the other rows are not touched).  Only the recurrent stages see the session boundaries (the map checked
        here, once); the projections take the packed rows as they are.
        commit=False: the caches are read and not written (the one-launch path only: NotImplementedError elsewhere).
        peek=True: the LAST row of every session (of the T rows without seq_map) is a peek row -- it runs through the block like any
        other row and its output is returned, and the caches are advanced by the rows before it only (a cls row behind a hop's tokens:
        it sees the state they produced, the next hop does not see it).  One launch with the flag where the one-launch path takes the
        shapes -- the peek row counts towards its 128 -- else the ladder with the two flags; both give the same bits at the kernels.
        peek_every=P (an int >= 1; not with peek=True or commit=False): a peek row behind every P committed rows of every session -- row j
        of a session is a peek row iff (j + 1) % (P + 1) == 0 (the cls row behind every time column: AudioMamba.stream_timeline).  Always
        the ladder, conv and scan through aum_hip.conv1d_tm_chunk_peeks / scan_tm_chunk_peeks (the one-launch kernel has no peek
        period); the caches are bit for bit those of peek=True calls on one group of P + 1 rows after the other."""
        import aum_hip
        if self.bimamba_type != "none":
            raise NotImplementedError("inference caches only make sense for the causal (bimamba_type='none') block")
        if peek_every is not None and (peek or not commit):
            raise ValueError("step_chunk(peek_every=) excludes peek=True and commit=False")
        if seq_map is not None:
            if not self._check_packed("step_chunk", hidden_states, conv_state, ssm_state, seq_map):
                return hidden_states.new_empty(hidden_states.shape), conv_state, ssm_state
        elif hidden_states.dim() != 3 or hidden_states.shape[1] < 1:
            raise ValueError("step_chunk() takes hidden_states of shape (batch, T >= 1, d_model)")
        batch, T, _ = hidden_states.shape
        E, N = self.d_inner, self.d_state
        xz = self.in_proj(hidden_states.reshape(batch * T, -1)).view(batch, T, 2 * E)
        x, z = xz[..., :E], xz[..., E:]
        plan = self.stream_params(xz.dtype)
        if peek_every is None and self.stream_block_ok(xz, conv_state, ssm_state, plan, seq_map):
            y = aum_hip.stream_block(x if seq_map is None else x[0], z if seq_map is None else z[0], conv_state, ssm_state, plan,
                                     seq_map=seq_map, commit=commit, peek=peek)
            return self.out_proj(y.reshape(batch * T, E)).view(batch, T, -1), conv_state, ssm_state
        if not commit:
            raise NotImplementedError("step_chunk(commit=False) needs the one-launch path (aum_hip.stream_block_supported)")
        xc = aum_hip.conv1d_stream(x, conv_state, plan.conv_w, plan.conv_b, self.activation in ("silu", "swish"), seq_map, peek=peek,
                                   peek_every=peek_every)
        if not xc.is_contiguous():
            xc = xc.contiguous()
        delta, Bm, Cm, activated = self._xdt_stage(xc.reshape(batch * T, E), plan)
        y = aum_hip.scan_stream(ssm_state, xc, delta.view(batch, T, E), plan.A, Bm.view(batch, T, N), Cm.view(batch, T, N), plan.D, z,
                                plan.dt_bias, True, activated, seq_map, peek=peek, peek_every=peek_every)
        out = self.out_proj(y.reshape(batch * T, E)).view(batch, T, -1)
        return out, conv_state, ssm_state

    def _prefill_ok(self, hidden_states, conv_state, ssm_state):
        """forward(x, inference_params) at seqlen_offset == 0: through prefill_chunk?  Only for the causal block with silu, on a DEVICE,
        with fp32 caches (what the kernels advance in place; the reference's default caches carry the parameters' dtype) and widths for
        which ssi.token_major_ok holds -- the rule of the offline token-major forward (dt_rank and dt_rank + 2 d_state keep 16-byte
        rows: dt_rank a multiple of 4 in fp32, of 8 in 16 bits).  Everything else keeps the un-fused branch."""
        work = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else self.in_proj.weight.dtype
        return (ssi.TOKEN_MAJOR and self.use_fast_path and self.bimamba_type == "none" and hidden_states.is_cuda and hidden_states.dim() == 3
                and hidden_states.shape[1] >= 1 and self.activation in ("silu", "swish")
                and conv_state.dtype == torch.float32 and ssm_state.dtype == torch.float32
                and ssi.token_major_ok(self.d_inner, self.d_state, self.d_conv, self.dt_rank, work))

    def _prefill_block_ok(self, xz):
        """what prefill_supported and prefill_packed_supported ask of the block itself for these (., ., 2E) in_proj rows: silu, rows of
        this block, a width aum_scan_tm_fwd takes, and 4-byte aligned B / C columns (an even dt_rank for 16-bit activations)"""
        import aum_hip
        E = xz.shape[2] // 2
        return (self.activation in ("silu", "swish") and E == self.d_inner and aum_hip.scan_tm_supported(E, self.d_state)
                and (xz.element_size() == 4 or self.dt_rank % 2 == 0))

    def prefill_supported(self, xz, conv_state, ssm_state):
        """prefill_chunk's dispatch for these (batch, T, 2E) in_proj rows and fixed-batch caches: what conv1d_tm_prefill and
        aum_scan_tm_fwd_state take -- silu, x rows the token-major conv takes with an fp32 (batch, E, width <= 4) window, d_state 16,
        E % 64 == 0, an fp32 contiguous 16-byte aligned (batch, E, 16) state, and B / C columns of the x_dbl rows that are 4-byte aligned
        for 16-bit activations (an even dt_rank; nothing for fp32).  The 16-byte widths of aum_xdt_tm_fwd are NOT required: where that
        kernel refuses, the x/dt products are the library's."""
        import aum_hip
        E = xz.shape[2] // 2
        return (self._prefill_block_ok(xz) and aum_hip.conv1d_tm_chunk_supported(xz[..., :E], conv_state)
                and aum_hip.scan_state_supported(ssm_state, xz.shape[0], E, self.d_state))

    def prefill_packed_supported(self, xz, conv_state, ssm_state, seq_map, range_len=0):
        """prefill_chunk(seq_map=)'s dispatch, the sibling of prefill_supported for (1, total, 2E) packed in_proj rows and POOLS of caches:
        what aum_conv1d_tm_prefill_var and aum_scan_tm_fwd_state_var take -- silu, x rows the token-major conv takes with an fp32
        (nrows, E, width <= 4) pool of windows, d_state 16, E % 64 == 0, an fp32 contiguous 16-byte aligned (nrows, E, 16) pool of states,
        B / C columns of the x_dbl rows 4-byte aligned for 16-bit activations (an even dt_rank), and a range_len that cuts the longest
        session into at most 32 ranges."""
        import aum_hip
        E = xz.shape[2] // 2
        return (self._prefill_block_ok(xz) and xz.shape[0] == 1 and aum_hip.conv1d_tm_prefill_var_supported(xz[0, :, :E], conv_state)
                and aum_hip.scan_state_supported(ssm_state, ssm_state.shape[0], E, self.d_state)
                and range_len % aum_hip.SCAN_TM_CK == 0 and (range_len == 0 or -(-max(seq_map.lens) // range_len) <= aum_hip.SCAN_TM_MAX_SEGMENTS))

    def _prefill_packed(self, hidden_states, conv_state, ssm_state, seq_map):
        """prefill_chunk with a seq_map: (1, total, d_model) packed backlogs, pools of caches"""
        import aum_hip
        if not self._check_packed("prefill_chunk", hidden_states, conv_state, ssm_state, seq_map):
            return hidden_states.new_empty(hidden_states.shape), conv_state, ssm_state
        total = hidden_states.shape[1]
        E = self.d_inner
        xz = self.in_proj(hidden_states[0]).view(1, total, 2 * E)
        plan = self.stream_params(xz.dtype)
        rng = aum_hip.scan_tm_var_range(seq_map.lens, E, device=xz.device) if xz.is_cuda else 0
        if not self.prefill_packed_supported(xz, conv_state, ssm_state, seq_map, rng):
            return self.step_chunk(hidden_states, conv_state, ssm_state, seq_map=seq_map)
        x, z = xz[0, :, :E], xz[0, :, E:]
        xc = aum_hip._conv1d_tm_prefill_var(x, conv_state, plan.conv_w, plan.conv_b, True, seq_map, None, aum_hip.get())
        delta, Bm, Cm, activated = self._xdt_stage(xc, plan)
        args = (ssm_state, xc, delta, plan.A, Bm, Cm, plan.D, z, None if activated else plan.dt_bias, not activated, activated)
        if not aum_hip.scan_tm_fwd_state_var_supported(*args, range_len=rng, max_len=max(seq_map.lens)):      # no quiet second path
            raise RuntimeError(f"prefill_chunk(seq_map=): aum_scan_tm_fwd_state_var does not take xc {tuple(xc.shape)} {xc.dtype}, delta "
                               f"{tuple(delta.shape)} strides {delta.stride()}, x_dbl strides {Bm.stride()}, range_len {rng}")
        y = aum_hip._scan_tm_fwd_state_var(*args, seq_map, rng, None, aum_hip.get())      # the map was checked above, once
        return self.out_proj(y).view(1, total, -1), conv_state, ssm_state

    def prefill_chunk(self, hidden_states, conv_state, ssm_state, seq_map=None):
        """A BACKLOG of T >= 1 tokens through the causal block at the speed of the offline forward: step_chunk's contract -- (batch, T,
        d_model) in and out, the fixed-batch caches conv_state (batch, d_inner, d_conv) and ssm_state (batch, d_inner, d_state) advanced
        in place by T tokens -- on the time-parallel kernels instead of one serial chain per wave:
            xz = in_proj(h)                                                      (batch, T, 2E) token-major rows [x | z]
            xc = aum_hip.conv1d_tm_prefill(x half, conv_state, w, b, silu)       conv1d_tm_fwd on [carried window ; x]
            (dt, B, C) = x_proj(xc);  delta = dt W_dt^T                          (one fused launch where aum_xdt_tm_fwd takes the shape)
            y = aum_hip.scan_tm_fwd_state(xc, delta, ..., state_in=ssm_state, state_out=ssm_state, segments=scan_tm_segments(...))
            out = out_proj(y)
        step_chunk / step continue from the caches it leaves (and it continues from theirs): the state crosses as exact fp32, the
        window holds the inputs themselves.  Against step_chunk on the same tokens the results agree to the kernels' tolerance, not
        bitwise (long rows are cut into time segments, which re-associates the recurrence).  Where the kernels do not take the shapes
        this IS step_chunk: prefill_supported says which (the blocks of AuM-Tiny, -Small and -Base all take the fast path; an odd
        dt_rank with 16-bit activations does not).
        seq_map (aum_hip.seq_map): the backlogs of SEVERAL SESSIONS in one pass, as step_chunk(seq_map=) takes their hops -- hidden_states
        (1, total, d_model) holds the sessions' tokens behind one another, the caches are pools of nrows rows, session i advances row
        seq_map.rows[i] by seq_map.lens[i] tokens and the other rows are not touched.  The four projections take the packed rows as they
        are; only aum_hip.conv1d_tm_prefill_var and aum_hip.scan_tm_fwd_state_var (cut into ranges where aum_hip.scan_tm_var_range says
        so) see the session boundaries.  Against prefill_chunk session by session the results agree to the kernels' tolerance, not
        bitwise: the GEMMs see another M.  Where prefill_packed_supported refuses, this is step_chunk(seq_map=)."""
        import aum_hip
        if self.bimamba_type != "none":
            raise NotImplementedError("inference caches only make sense for the causal (bimamba_type='none') block")
        if seq_map is not None:
            return self._prefill_packed(hidden_states, conv_state, ssm_state, seq_map)
        if hidden_states.dim() != 3 or hidden_states.shape[1] < 1:
            raise ValueError("prefill_chunk() takes hidden_states of shape (batch, T >= 1, d_model)")
        batch, T, _ = hidden_states.shape
        E, N = self.d_inner, self.d_state
        if conv_state.shape[0] != batch or ssm_state.shape[0] != batch:
            raise ValueError(f"prefill_chunk() advances fixed-batch caches: {conv_state.shape[0]} / {ssm_state.shape[0]} rows for a batch of {batch}")
        xz = self.in_proj(hidden_states.reshape(batch * T, -1)).view(batch, T, 2 * E)
        x, z = xz[..., :E], xz[..., E:]
        plan = self.stream_params(xz.dtype)
        if not self.prefill_supported(xz, conv_state, ssm_state):
            return self.step_chunk(hidden_states, conv_state, ssm_state)
        xc = aum_hip.conv1d_tm_prefill(x, conv_state, plan.conv_w, plan.conv_b, True).contiguous()
        delta, Bm, Cm, activated = self._xdt_stage(xc.view(batch * T, E), plan)
        seg = aum_hip.scan_tm_segments(batch, E, T, False, device=xc.device) if xc.is_cuda else 1
        args = (xc, delta.view(batch, T, E), plan.A, Bm.view(batch, T, N), Cm.view(batch, T, N), plan.D, z, None if activated else plan.dt_bias,
                not activated, activated)
        y = aum_hip.scan_tm_fwd_state(*args, state_in=ssm_state, state_out=ssm_state, segments=seg)     # raises where it refuses: no quiet second path
        out = self.out_proj(y.reshape(batch * T, E)).view(batch, T, -1)
        return out, conv_state, ssm_state

    def stream_block_ok(self, xz, conv_state, ssm_state, plan, seq_map=None):
        """step_chunk's dispatch: the one-launch middle for these (batch, T, 2E) in_proj rows and caches?  (aum_hip.debug.stream_fused
        = False: never -- the three-launch path, for A/B runs.)"""
        import aum_hip
        if not (aum_hip.debug.stream_fused and xz.is_cuda and self.activation in ("silu", "swish") and self.d_conv == 4 and self.conv1d.bias is not None):
            return False
        batch, T, E2 = xz.shape
        rows = xz.view(batch * T, E2)
        lens = (T,) if seq_map is None else seq_map.lens
        if seq_map is None and conv_state.shape[0] != batch:
            return False
        return aum_hip.stream_block_supported(rows[:, :E2 // 2], rows[:, E2 // 2:], conv_state, ssm_state, plan, max(lens))

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        """MS:360-373"""
        device = self.out_proj.weight.device
        conv_state = torch.zeros(batch_size, self.d_inner, self.d_conv, device=device,
                                 dtype=self.conv1d.weight.dtype if dtype is None else dtype)
        ssm_state = torch.zeros(batch_size, self.d_inner, self.d_state, device=device,
                                dtype=self.dt_proj.weight.dtype if dtype is None else dtype)
        return conv_state, ssm_state

    def _get_states_from_cache(self, inference_params, batch_size, initialize_states=False):
        """MS:375-400"""
        assert self.layer_idx is not None
        if self.layer_idx not in inference_params.key_value_memory_dict:
            inference_params.key_value_memory_dict[self.layer_idx] = self.allocate_inference_cache(batch_size, 0)
        conv_state, ssm_state = inference_params.key_value_memory_dict[self.layer_idx]
        if initialize_states:
            conv_state.zero_()
            ssm_state.zero_()
        return conv_state, ssm_state
