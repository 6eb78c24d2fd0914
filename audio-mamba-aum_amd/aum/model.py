"""AuM (Audio Mamba) assembled from the drop-in mamba_ssm package: patch embed -> middle cls token -> abs pos embed
-> depth x [fused add+RMSNorm -> Mamba mixer] -> final fused add+RMSNorm -> cls -> linear head.

Mirrors the default configuration of the reference's AudioMamba (/root/reference/src/models/mamba_models.py = "MM":
forward_features MM:509-667, Block.forward MM:58-99, defaults MM:191-242) and produces the SAME state-dict keys
(patch_embed.proj.*, cls_token, pos_embed.pos_embed, layers.{i}.mixer.*, layers.{i}.norm.weight, norm_f.weight,
head.*) so published checkpoints load.  Also mirrored: the cls-token placements of RUN's flags (middle / end / head,
MM:528-535), `transpose_token_sequence` (time-major token order, MM:545-566) and `if_bidirectional` layer pairing
(MM:623-638), and ImageNet Vim initialisation (`imagenet_pretrain`, MM:348-395; aum.checkpoint.load_imagenet_checkpoint).
The cls layouts of MM:518-537 are all here: one cls token (also at a random position per forward), `use_double_cls_token`
(cls_token_head / cls_token_tail) and `if_cls_token=False` with `final_pool_type` none / mean / max (MM:659-685).
Options off that surface (rope, flexible patch sizes, token dropout, final_pool_type 'all') are rejected.
"""
import math
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from mamba_ssm.modules.mamba_simple import Mamba
from mamba_ssm.ops.selective_scan_interface import _autocast_dtype, step_cache
from mamba_ssm.ops.triton.layernorm import RMSNorm, rms_norm_fn, rms_norm_pool_fn

AUM_SIZES = {"base": 768, "small": 384, "tiny": 192}      # embed dims; depth 24 for all three (RUN:227-237)


class PatchEmbed(nn.Module):
    """FlexiPatchEmbed default branch (TOK:278-310): conv2d(kernel=stride=patch) -> flatten -> (B, N, Dm)."""

    def __init__(self, patch_size, strides, in_chans, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=strides)
        fan_in = in_chans * patch_size[0] * patch_size[1]
        nn.init.trunc_normal_(self.proj.weight, std=math.sqrt(1.0 / fan_in) / 0.87962566103423978)   # lecun_normal_
        nn.init.zeros_(self.proj.bias)

    def forward(self, x):
        # non-overlapping patches: the conv is a [B*N, C*ph*pw] x [C*ph*pw, Dm] GEMM (no MIOpen find/autotune in the loop)
        Bsz, C, Fd, Td = x.shape
        ph, pw = self.proj.kernel_size
        nf, nt = Fd // ph, Td // pw
        cols = x[:, :, :nf * ph, :nt * pw].reshape(Bsz, C, nf, ph, nt, pw).permute(0, 2, 4, 1, 3, 5)
        cols = cols.reshape(Bsz * nf * nt, C * ph * pw)
        out = F.linear(cols, self.proj.weight.reshape(self.proj.out_channels, -1), self.proj.bias)
        return out.reshape(Bsz, nf * nt, -1)


class FrontendTokensFn(torch.autograd.Function):
    """Waveform -> (B, N+1, Dm) token sequence in one launch (aum_frontend_tokens_fwd): log-mel frames, patch GEMM, bias,
    position rows and the cls row, with the arithmetic of the autocast reference (16-bit conv output, fp32 position add;
    DL:134-147 -> TOK:278-310 -> MM:509-541).  Backward: the patch matrix saved by the kernel gives the weight gradient."""

    @staticmethod
    def forward(ctx, wave, weight, bias, pos_embed, cls_token, fe, dtype, cls_pos, time_major):
        import aum_hip
        Dm = weight.shape[0]
        w16 = weight.detach().reshape(Dm, -1).to(dtype).contiguous()
        pe = pos_embed.detach().float()
        cls_row = (cls_token.detach().float() + pe[:, :1]).reshape(Dm).contiguous()
        need = any(ctx.needs_input_grad[1:5])
        tokens, patches = aum_hip.frontend_tokens(
            wave, fe.tables.tables, fe.target_length, fe.norm_mean, fe.norm_std, w16, bias.detach().float().contiguous(),
            pe[0, 1:].contiguous(), cls_row, cls_pos, time_major=time_major, save_patches=need, aug=fe.aug, noise=fe.noise)
        ctx.save_for_backward(patches)
        ctx.cfg = (weight.shape, weight.dtype, dtype, cls_pos, time_major, fe.target_length // 16)
        return tokens

    @staticmethod
    def backward(ctx, g):
        (patches,) = ctx.saved_tensors
        wshape, wdtype, dtype, cls_pos, time_major, nt = ctx.cfg
        Bsz, _, Dm = g.shape
        gp = torch.cat((g[:, :cls_pos], g[:, cls_pos + 1:]), dim=1)              # (B, N, Dm) in sequence order
        if time_major:                                                          # back to the cell order f * n_t + t
            gp = gp.reshape(Bsz, nt, -1, Dm).transpose(1, 2).reshape(Bsz, -1, Dm)
        g16 = gp.to(dtype).reshape(-1, Dm)                                      # gradient of the 16-bit conv output
        import aum_hip
        if g16.is_cuda and aum_hip.gemm_wgrad_supported(g16, patches):          # 3 output tiles x 64 token splits instead of a one-round library GEMM over 32 768 tokens
            dweight = aum_hip.gemm_wgrad(g16, patches).to(wdtype).reshape(wshape)
        else:
            dweight = (g16.t() @ patches).to(wdtype).reshape(wshape)
        dbias = g16.sum(0).to(wdtype)
        dcls = g[:, cls_pos].sum(0)
        dpos = torch.cat((dcls[None], gp.sum(0)), dim=0)[None]
        return None, dweight, dbias, dpos.to(wdtype), dcls.reshape(1, 1, Dm).to(wdtype), None, None, None, None


class PosEmbed(nn.Module):
    """FlexiPosEmbed with pos_embed_prefix=True (TOK:330-451): row 0 belongs to the cls token, rows 1.. to the patches."""

    def __init__(self, n_tokens, embed_dim):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, n_tokens, embed_dim))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)


def drop_rates(drop_path_rate, depth):
    """depth + 1 rates.  Entry i < depth is block i's: inter_dpr[i] of MM:290-292, inter_dpr = [0.0] + linspace(0, rate, depth) (block 0
    never drops, block i >= 1 has rate (i - 1) / (depth - 1); at depth 1 the linspace is [0]).  The last entry is the rate itself, at
    every depth: that of the add in front of norm_f, DropPath(drop_path_rate) (MM:293, 650)."""
    inter_dpr = [0.0] + torch.linspace(0, drop_path_rate, depth, device="cpu").tolist()      # (on the host also under a device context)
    return inter_dpr[:depth] + [float(drop_path_rate)]


def drop_factors(keep):
    """timm's DropPath factors (training, scale_by_keep): one Bernoulli(keep) draw per element of the fp32 tensor `keep` (keep > 0) in
    ONE launch, from the default generator of its device; a kept element is 1 / keep, a dropped one 0."""
    return torch.bernoulli(keep) / keep


class Block(nn.Module):
    """MM:30-99 with fused_add_norm=True, residual_in_fp32=True.  drop_path (MM:51): the rate of stochastic depth on the incoming
    hidden_states -- the previous mixer's output -- in training; the factor is applied inside the add + norm kernels."""

    def __init__(self, dim, mixer, eps, drop_path=0.0):
        super().__init__()
        if not 0.0 <= drop_path < 1.0:
            raise ValueError(f"drop_path must be in [0, 1), not {drop_path}")
        self.mixer = mixer
        self.norm = RMSNorm(dim, eps=eps)
        self.drop_path = float(drop_path)

    def forward(self, hidden_states, residual=None, inference_params=None, *, time_reversed=False, row_scale=None):
        """MM:58-99 (the third positional slot is the reference's inference_params).  time_reversed (keyword only): the block on the
        time-reversed sequence, reversed back (the odd layers of `if_bidirectional`) -- add + norm is token-wise, the mixer takes the
        flag: no flipped copies of hidden_states / residual.  row_scale (keyword only): this forward's (batch,) fp32 stochastic-depth
        factors of the block (AudioMamba draws all blocks' at once); a block called on its own in training draws them itself.  No
        residual (the first block): no drop, MM:78-87."""
        if residual is None:
            row_scale = None
        elif row_scale is None and self.training and self.drop_path > 0:
            row_scale = drop_factors(torch.full((hidden_states.shape[0],), 1.0 - self.drop_path, device=hidden_states.device))
        hidden_states, residual = rms_norm_fn(hidden_states, self.norm.weight, self.norm.bias, residual=residual,
                                              prenorm=True, residual_in_fp32=True, eps=self.norm.eps, row_scale=row_scale)
        if time_reversed:
            return self.mixer(hidden_states, inference_params=inference_params, time_reversed=True), residual
        return self.mixer(hidden_states, inference_params=inference_params), residual


class ParkedSessions:
    """Streaming sessions off their pool (AudioMamba.stream_park makes it, stream_resume takes it):
      blob       (n, record) uint8, on the pool's device or in pinned host memory -- session i's rows of every pool tensor behind one
                 another (aum_hip.stream_park_layout: per layer conv window and scan state, then the sample tail), as the bytes they were
      columns    [n] time columns pushed so far
      wave       None, or with a WaveStream {tail_len, samples, frames, ended}: [n] each, the host counters of the sample tail
      signature  (depth, d_inner, d_conv, d_state, cache dtype, tail width; 0: no tail): what the record's layout depends on --
                 stream_resume refuses caches with another one
    len(state) sessions; state[i] one of them, state.select(idx) several, in that order (an index may repeat)."""
    WAVE_KEYS = ("tail_len", "samples", "frames", "ended")

    def __init__(self, blob, columns, wave, signature):
        self.blob, self.columns, self.wave, self.signature = blob, list(columns), wave, tuple(signature)

    def __len__(self):
        return len(self.columns)

    def select(self, idx):
        idx = [int(i) for i in idx]
        if not idx or min(idx) < -len(self) or max(idx) >= len(self):
            raise IndexError(f"ParkedSessions.select: {idx} of {len(self)} sessions")
        idx = [i % len(self) for i in idx]
        if len(set(idx)) == 1:                     # one record for all: a view, no copy (stream_resume reads it len(idx) times)
            blob = self.blob[idx[0]:idx[0] + 1].expand(len(idx), -1)
        else:
            blob = self.blob.index_select(0, torch.tensor(idx, dtype=torch.int64).to(self.blob.device))
        wave = None if self.wave is None else {k: [v[i] for i in idx] for k, v in self.wave.items()}
        return ParkedSessions(blob, [self.columns[i] for i in idx], wave, self.signature)

    def __getitem__(self, i):
        return self.select([i])


class StreamStack:
    """What aum_hip.stream_layers reads of a streamable AudioMamba, converted once (AudioMamba.stream_stack makes and caches it): per block
    Mamba.stream_params(dtype), the 16-bit in_proj / out_proj weights, the fp32 norm weight, and the HOST table of device pointers the C loop
    walks -- only its two pool pointers per block are written per call.  With it a hop through all blocks is ONE library call that
    enqueues 3 * depth launches (add + norm + in_proj, the one-launch middle, out_proj), no Python or torch dispatch between them.
    takes(total, max_len): which calls go that way -- sessions of at most 128 rows (the middle kernel's limit) and at most MAX_TOTAL rows
    in all; the others take the loop over the layers as without a stack.
    MAX_TOTAL = 512: the projection kernels accept any row count, but every workgroup recomputes the norm of ALL rows of the call for its
    32 output columns; at a few hundred rows that prologue is the size of the workgroup's weight slab, beyond it the prologue is the
    kernel and the library GEMMs of the loop are the better tool.  512 is four sessions at the middle kernel's limit and leaves room
    above the 288 rows of 32 sessions pushing one column with a peek row each.  The tensors are shared between calls: do not write to them.
    The workspace is ONE tensor, shared by every call through this stack: calls on different torch streams at the same time would
    overwrite one another's rows -- serve one stream per model, or give every stream a model (and so a stack) of its own.
    fresh(): whether the model still is what the stack was built from -- per source parameter one dict lookup for its identity and its
    _version, dtype and device, and per block the generation Mamba.invalidate_stream_params() moves: the only per-hop host work of the cache."""
    MAX_TOTAL = 512

    def __init__(self, model, dtype):
        import aum_hip
        self.dtype, self.depth = dtype, len(model.layers)
        self.sources = [(d, n, p, None if p is None else (p._version, p.dtype, p.device)) for d, n, p in model._stack_sources()]
        self.gens = [(layer.mixer.__dict__, layer.mixer.__dict__.get("_stream_gen", 0)) for layer in model.layers]
        m0 = model.layers[0].mixer
        self.d_model, self.dim, self.eps = m0.d_model, m0.d_inner, model.layers[0].norm.eps
        self.plans, self.keep, recs = [], [], []
        for layer in model.layers:
            mx = layer.mixer
            plan = mx.stream_params(dtype)
            w_in = aum_hip._al16(mx.in_proj.weight.detach().to(dtype).contiguous())
            w_out = aum_hip._al16(mx.out_proj.weight.detach().to(dtype).contiguous())
            nw = aum_hip._al16(aum_hip._f32c(layer.norm.weight))
            self.plans.append(plan)
            self.keep.append((w_in, w_out, nw))
            recs.append({"norm_weight": nw, "w_in": w_in, "conv_weight": plan.conv_w, "conv_bias": plan.conv_b, "wx": plan.w_x, "wdt": plan.w_dt,
                         "A": plan.A, "D": plan.D, "delta_bias": plan.dt_bias, "w_out": w_out, "conv_state": None, "state": None})
        p0 = self.plans[0]
        self.rank, self.ncols, self.ldwx, self.ldwdt = p0.w_dt.shape[1], p0.w_x.shape[0], p0.w_x.stride(0), p0.w_dt.stride(0)
        self.table = aum_hip.stream_layers_table(recs)
        self.records_ok = aum_hip.stream_layers_records_ok(self.table, self.depth)       # the parameter pointers: checked once, here
        self.workspace = None

    def fresh(self):
        for d, n, p, sig in self.sources:
            q = d.get(n)
            if q is not p or (p is not None and (p._version, p.dtype, p.device) != sig):
                return False
        return all(d.get("_stream_gen", 0) == g for d, g in self.gens)

    def takes(self, total, max_len):
        import aum_hip
        return 1 <= max_len <= aum_hip.STREAM_BLOCK_MAX_T and 1 <= total <= self.MAX_TOTAL

    def pools_ok(self, layer_caches):
        """the pools as the middle kernel takes them: fp32, contiguous, 16-byte aligned, (nrows, dim, 4) / (nrows, dim, 16), one size"""
        if len(layer_caches) != self.depth:
            return False
        n = layer_caches[0][0].shape[0]
        return all(c.dtype == torch.float32 and s.dtype == torch.float32 and c.is_contiguous() and s.is_contiguous()
                   and tuple(c.shape) == (n, self.dim, 4) and tuple(s.shape) == (n, self.dim, 16) and c.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
                   for c, s in (layer_caches[i] for i in range(self.depth)))

    def run(self, rows, layer_caches, smap, commit=True, peek=False):
        """rows (total, d_model) -> (hidden, residual fp32) of the last block; the pools of layer_caches advance in place"""
        import aum_hip
        rows = rows.to(self.dtype).contiguous()
        for i in range(self.depth):
            self.table[i].conv_state, self.table[i].state = layer_caches[i][0].data_ptr(), layer_caches[i][1].data_ptr()
        need = aum_hip.stream_layers_scratch_layout(rows.shape[0], self.d_model, self.dim, self.ncols)[2]
        if self.workspace is None or self.workspace.numel() < need or self.workspace.device != rows.device:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=rows.device)
        return aum_hip.stream_layers(rows, self.table, self.depth, layer_caches[0][0], smap, dim=self.dim, rank=self.rank, ncols=self.ncols,
                                     ldwx=self.ldwx, ldwdt=self.ldwdt, eps=self.eps, commit=commit, peek=peek, workspace=self.workspace,
                                     records_ok=self.records_ok)


class AudioMamba(nn.Module):
    def __init__(self, spectrogram_size=(128, 1024), patch_size=(16, 16), strides=(16, 16), depth=24, embed_dim=768,
                 channels=1, num_classes=527, norm_epsilon=1e-5, bimamba_type="v1", if_devide_out=True,
                 use_middle_cls_token=True, use_end_cls_token=False, transpose_token_sequence=False,
                 if_bidirectional=False, ssm_cfg=None, device=None, dtype=None, imagenet_pretrain=False,
                 imagenet_pretrain_path=None, imagenet_pretrain_modelkey="model", imagenet_load_middle_cls_token=True,
                 imagenet_load_double_cls_token=False, drop_path_rate=0.0, if_cls_token=True, use_double_cls_token=False,
                 final_pool_type="mean", **unsupported):
        super().__init__()
        on = {k: v for k, v in unsupported.items() if v not in (None, False, 0, 0.0, -1.0)
              and k not in ("rms_norm", "fused_add_norm", "residual_in_fp32", "if_abs_pos_embed", "use_PI_for_patch_embed")}
        if on:
            raise NotImplementedError(f"AudioMamba options outside the accelerated path: {sorted(on)}")
        # the cls layouts of MM:518-537: one cls token (middle / end / head), a head and a tail token, or none and a pool over the tokens
        self.if_cls_token, self.use_double_cls_token = bool(if_cls_token), bool(use_double_cls_token)
        if self.use_double_cls_token and not self.if_cls_token:
            raise ValueError("use_double_cls_token needs if_cls_token=True")
        if self.use_double_cls_token and (use_middle_cls_token or use_end_cls_token):
            raise ValueError("use_double_cls_token puts one cls token in front of the patches and one behind them: it excludes "
                             "use_middle_cls_token and use_end_cls_token (pass both as False)")
        if imagenet_load_double_cls_token and not self.use_double_cls_token:
            raise NotImplementedError("imagenet_load_double_cls_token loads a double-cls checkpoint: it needs use_double_cls_token=True")
        if final_pool_type == "all":
            raise NotImplementedError("final_pool_type='all' (every token's features as the model output) is off the accelerated path")
        if final_pool_type not in ("none", "mean", "max"):
            raise ValueError(f"final_pool_type must be 'none', 'mean' or 'max', not {final_pool_type!r}")
        self.final_pool_type = final_pool_type                    # read only without a cls token (MM:666-675)
        if tuple(patch_size) != tuple(strides):
            raise NotImplementedError("overlapping patches are off the default path")
        self.embed_dim = self.d_model = embed_dim
        self.num_classes = num_classes
        self.use_middle_cls_token = use_middle_cls_token
        self.use_end_cls_token = use_end_cls_token
        self.transpose_token_sequence = transpose_token_sequence
        self.if_bidirectional = if_bidirectional
        if if_bidirectional and depth % 2:
            raise ValueError("if_bidirectional pairs the layers: depth must be even")
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1), not {drop_path_rate}")
        self.drop_path_rate = float(drop_path_rate)
        self._drop_rates = drop_rates(self.drop_path_rate, depth)      # [block 0 .. block depth - 1, the add in front of norm_f]
        self._drop_keep = {}                                            # device -> (depth + 1, 1) fp32 keep probabilities
        fdim = (spectrogram_size[0] - patch_size[0]) // strides[0] + 1
        tdim = (spectrogram_size[1] - patch_size[1]) // strides[1] + 1
        self.patch_grid_size = (fdim, tdim)
        self.num_patches = fdim * tdim
        self.num_tokens = 0 if not self.if_cls_token else (2 if self.use_double_cls_token else 1)
        cls_names = {0: (), 1: ("cls_token",), 2: ("cls_token_head", "cls_token_tail")}[self.num_tokens]      # MM:243-252
        for name in cls_names:
            setattr(self, name, nn.Parameter(torch.zeros(1, 1, embed_dim)))
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self.layers = nn.ModuleList([
            Block(embed_dim, Mamba(embed_dim, layer_idx=i, bimamba_type=bimamba_type, if_devide_out=if_devide_out,
                                   **(ssm_cfg or {})), norm_epsilon, drop_path=self._drop_rates[i])
            for i in range(depth)])
        self.norm_f = RMSNorm(embed_dim, eps=norm_epsilon)
        if isinstance(self.head, nn.Linear):                       # segm_init_weights, MM:179-184
            nn.init.trunc_normal_(self.head.weight, std=0.02)
            nn.init.zeros_(self.head.bias)
        for name in cls_names:
            nn.init.trunc_normal_(getattr(self, name), std=0.02)
        self.apply(lambda m: _init_weights(m, depth))              # MM:146-176
        self.patch_embed = PatchEmbed(tuple(patch_size), tuple(strides), channels, embed_dim)
        self.pos_embed = PosEmbed(self.num_patches + self.num_tokens, embed_dim)
        if imagenet_pretrain:                                      # MM:348-395: after the model's own init, the loaded values win
            from .checkpoint import load_imagenet_checkpoint
            print(load_imagenet_checkpoint(self, imagenet_pretrain_path, imagenet_pretrain_modelkey,
                                           imagenet_load_middle_cls_token, imagenet_load_double_cls_token))
        if device is not None or dtype is not None:
            self.to(device=device, dtype=dtype)

    def no_weight_decay(self):
        return {"pos_embed", "cls_token", "cls_token_head", "cls_token_tail"}

    def _cls_pos(self, cls_pos=None):
        """where the single cls token goes (MM:526-533): cls_pos where given (a random position of this forward), else by the flags"""
        Np = self.num_patches
        return cls_pos if cls_pos is not None else (Np // 2 if self.use_middle_cls_token else (Np if self.use_end_cls_token else 0))

    def tokens(self, x, cls_pos=None):
        """(B, T, F) spectrogram -> ((B, N + num_tokens, Dm) token sequence, where the cls rows are) (MM:509-562).  One cls token: in
        the middle / at the end / in front, or at cls_pos; position row 0 is its.  Two: [head | patches | tail], position rows 0 and 1
        are the head's and the tail's and rows 2.. the patches' (FlexiPosEmbed.insert_to_prefix, TOK:389-399), the place is
        (0, N + 1).  None: the patches alone, place None.  transpose_token_sequence reorders the patches only."""
        x = x.unsqueeze(1).transpose(2, 3)                         # B x 1 x F x T
        x = self.patch_embed(x)                                    # token index = f * n_t + t
        Bsz, Np, _ = x.shape
        pe = self.pos_embed.pos_embed
        x = x + pe[:, self.num_tokens:]                            # position embedding belongs to the (f, t) cell
        if self.transpose_token_sequence:                          # MM:545-566: patches in time-major order, cls stays put
            nf, nt = self.patch_grid_size
            x = x.reshape(Bsz, nf, nt, -1).transpose(1, 2).reshape(Bsz, nt * nf, -1)
        if self.num_tokens == 0:
            return x, None
        if self.num_tokens == 2:
            head = (self.cls_token_head + pe[:, :1]).expand(Bsz, -1, -1)
            tail = (self.cls_token_tail + pe[:, 1:2]).expand(Bsz, -1, -1)
            return torch.cat((head.to(x.dtype), x, tail.to(x.dtype)), dim=1), (0, Np + 1)
        pos = self._cls_pos(cls_pos)                               # MM:526-535
        cls = (self.cls_token + pe[:, :1]).expand(Bsz, -1, -1)
        return torch.cat((x[:, :pos], cls.to(x.dtype), x[:, pos:]), dim=1), pos

    def tokens_from_wave(self, wave, fe, cls_pos=None):
        """(B, n_samples) mean-removed waveform + aum.frontend.WaveInput -> the same token sequence as tokens(spectrogram), in one
        launch when the configuration is the 16 kHz / 128-mel / 16 x 16 autocast one; otherwise log-mel kernel + tokens()."""
        import aum_hip
        dtype = torch.get_autocast_dtype(wave.device.type) if torch.is_autocast_enabled(wave.device.type) else None
        ps = self.patch_embed.proj
        # (the one-launch kernel writes the single-cls layout, at any position; double-cls and cls-free models take the log-mel kernel)
        if (dtype is None or self.num_tokens != 1 or tuple(ps.kernel_size) != (16, 16) or ps.in_channels != 1 or self.patch_grid_size[0] != 8
                or self.patch_grid_size[1] * 16 != fe.target_length
                or not aum_hip.frontend_tokens_supported(fe.tables.tables, fe.target_length, self.embed_dim, dtype)):
            return self.tokens(fe.spectrogram(wave), cls_pos)
        pos = self._cls_pos(cls_pos)
        tok = FrontendTokensFn.apply(wave, ps.weight, ps.bias, self.pos_embed.pos_embed, self.cls_token, fe, dtype, pos,
                                     self.transpose_token_sequence)
        return tok, pos

    def drop_scales(self, batch, device):
        """The stochastic-depth factors of ONE forward, (depth + 1, batch) fp32 on `device`: row i is block i's (row 0: ones, block 0
        never drops), row `depth` the add's in front of norm_f; an entry is 0 (the sample skips that block's input) or 1 / keep.  All
        rows are one Bernoulli launch from the device's default generator (reproducible under torch.manual_seed; every rank of a
        data-parallel run draws its own, as the reference's DropPath modules do)."""
        device = torch.device(device)
        keep = self._drop_keep.get(device)
        if keep is None:
            keep = self._drop_keep[device] = (1.0 - torch.tensor(self._drop_rates, dtype=torch.float64)).to(torch.float32)[:, None].to(device)
        return drop_factors(keep.expand(-1, batch))

    def _drop(self, hidden):
        """this forward's drop_scales, or None (eval, rate 0): then no factor exists and the unscaled add + norm kernels run"""
        return self.drop_scales(hidden.shape[0], hidden.device) if self.training and self.drop_path_rate > 0 else None

    def forward_features(self, x, frontend=None, if_random_cls_token_position=False):
        """if_random_cls_token_position (MM:526-527, the training loop's argument): the single cls token at one random.randint(0, N)
        position for this forward"""
        cls_pos = None
        if if_random_cls_token_position:
            if self.num_tokens != 1:
                raise ValueError("if_random_cls_token_position moves the single cls token: not with use_double_cls_token or if_cls_token=False")
            cls_pos = random.randint(0, self.num_patches)
        hidden, pos = self.tokens(x, cls_pos) if frontend is None else self.tokens_from_wave(x, frontend, cls_pos)
        scales = self._drop(hidden)
        with step_cache([layer.mixer for layer in self.layers], _autocast_dtype()):     # all blocks' 16-bit weights and A in a few launches
            hidden, residual = self._run_layers(hidden, scales)
        # MM:646-657, then the cls row (MM:660-680).  add + RMSNorm is row-wise and only the cls row is read: the final norm runs on
        # those `batch` rows instead of on all 513 per clip (same values, same gradients; 0.1 ms per step at the bench shape)
        last = None if scales is None or residual is None else scales[-1]
        norm = lambda h, r: rms_norm_fn(h, self.norm_f.weight, self.norm_f.bias, eps=self.norm_f.eps, residual=r, prenorm=False,
                                        residual_in_fp32=True, row_scale=last)
        rows = lambda t, idx: None if t is None else t[:, idx]
        if self.num_tokens == 2:                                   # MM:661-662: the mean of the two cls rows; the norm runs on those two
            f = norm(rows(hidden, list(pos)), rows(residual, list(pos)))
            return (f[:, 0] + f[:, 1]) / 2
        if self.num_tokens == 0 and self.final_pool_type != "none":        # MM:668-671
            if self.final_pool_type == "max":                      # every token's features: forward() takes the max of their logits
                return norm(hidden, residual)
            if last is None and residual is not None and hidden.dtype in (torch.bfloat16, torch.float16):
                # add + norm + mean in one pass (aum_rmsnorm_pool_fwd / _bwd): the normalised (B, L, D) rows and their gradient never exist
                return rms_norm_pool_fn(hidden, self.norm_f.weight, residual, self.norm_f.eps)
            # fp32 activations, or stochastic depth on the add in training: the norm kernels on all rows, then the mean
            return norm(hidden, residual).mean(dim=1)
        if self.num_tokens == 0:
            pos = hidden.shape[1] - 1                              # MM:667: 'none' reads the last token
        return norm(hidden[:, pos], rows(residual, pos))

    def _run_layers(self, hidden, scales=None):
        """scales: drop_scales() of this forward or None; block i takes row i (each layer of an `if_bidirectional` pair its own)"""
        residual = None
        row = (lambda i: None) if scales is None else (lambda i: scales[i])
        if not self.if_bidirectional:
            for i, layer in enumerate(self.layers):
                hidden, residual = layer(hidden, residual, row_scale=row(i))
        else:                                                      # MM:623-638: layer 2i forward, layer 2i+1 on the flipped sequence
            for i in range(len(self.layers) // 2):
                # flip(layer(flip(h), flip(r))) == layer(h, r, time_reversed=True): the four flipped copies per pair are direction
                # flags on the conv and scan kernels (a per-sample factor commutes with the flip)
                hf, rf = self.layers[2 * i](hidden, residual, row_scale=row(2 * i))
                hb, rb = self.layers[2 * i + 1](hidden, residual, time_reversed=True, row_scale=row(2 * i + 1))
                hidden, residual = hf + hb, rf + rb
        return hidden, residual

    # ---- streaming inference (causal models): feed a clip hop by hop -----------------------------
    def _check_streamable(self):
        """Streaming needs every token to depend on earlier tokens only and the cls token to come last: causal blocks, one direction,
        time-major token order, cls at the end."""
        if self.num_tokens != 1:
            raise ValueError("streaming inference needs the single end cls token (if_cls_token=True, use_double_cls_token=False, "
                             "use_end_cls_token=True): it is the row that reads the state behind the tokens pushed so far")
        bt = self.layers[0].mixer.bimamba_type if len(self.layers) else "none"
        if bt != "none":
            raise ValueError(f"streaming inference needs bimamba_type='none' (causal blocks), not {bt!r}")
        if self.if_bidirectional:
            raise ValueError("streaming inference needs if_bidirectional=False")
        if self.use_middle_cls_token:
            raise ValueError("streaming inference needs use_middle_cls_token=False (the cls token must close the sequence)")
        if not self.use_end_cls_token:
            raise ValueError("streaming inference needs use_end_cls_token=True (the cls token must close the sequence)")
        if not self.transpose_token_sequence:
            raise ValueError("streaming inference needs transpose_token_sequence=True (time-major token order)")

    def allocate_inference_cache(self, batch_size, max_seqlen=0, dtype=None, **kwargs):
        """Caches of a streaming session (MM:496-503): per layer the block's (conv_state, ssm_state), fp32 whatever the parameters' dtype
        (what the chunk kernels advance in place), plus the number of time columns pushed so far."""
        self._check_streamable()
        dtype = torch.float32 if dtype is None else dtype
        return {"layers": {i: layer.mixer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)
                           for i, layer in enumerate(self.layers)},
                "columns": 0, "batch": batch_size}

    def _stack_sources(self):
        """(the module's parameter dict, name, parameter or None) of everything a StreamStack is converted from"""
        out = []
        for layer in self.layers:
            mx = layer.mixer
            for mod, names in ((mx, ("A_log", "D")), (mx.conv1d, ("weight", "bias")), (mx.x_proj, ("weight",)), (mx.dt_proj, ("weight", "bias")),
                               (mx.in_proj, ("weight", "bias")), (mx.out_proj, ("weight", "bias")), (layer.norm, ("weight", "bias"))):
                out += [(mod._parameters, n, mod._parameters.get(n)) for n in names]
        return out

    @torch.no_grad()
    def stream_stack(self, dtype=None):
        """The StreamStack of this model for stream_push / stream_push_many / stream_read (..., stack=): every block's parameters as the
        one-call path reads them.  dtype: the working 16-bit dtype (default: the parameters').  Cached and keyed as Mamba.stream_params()
        is, on every source parameter's identity, _version, dtype and device: an optimizer step, load_state_dict or .to() rebuild it (a
        write through `p.data` does not: write under torch.no_grad(), or call Mamba.invalidate_stream_params() on the block behind it,
        which drops this cache as well).  A hit costs StreamStack.fresh() and nothing else; the model is examined on a miss.  Raises ValueError, with the reason, for a model the kernels do
        not take: not streamable, projection or norm biases, d_conv != 4, d_state != 16, widths other than (192, 384), (384, 768),
        (768, 1536), or a dtype that is not bf16 / fp16."""
        import aum_hip
        hit = self.__dict__.get("_stream_stack")
        if hit is not None and (dtype is None or dtype == hit.dtype) and hit.fresh() and (
                dtype is not None or hit.dtype == self.layers[0].mixer.in_proj.weight.dtype):
            return hit
        self._check_streamable()
        if not len(self.layers):
            raise ValueError("stream_stack: the model has no blocks")
        dtype = self.layers[0].mixer.in_proj.weight.dtype if dtype is None else dtype
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"stream_stack: the projection kernels run in bf16 or fp16, not {dtype}")
        for i, layer in enumerate(self.layers):
            mx = layer.mixer
            if mx.in_proj.bias is not None or mx.out_proj.bias is not None:
                raise ValueError(f"stream_stack: block {i} has projection biases (bias=True); the projection kernels add none")
            if getattr(layer.norm, "bias", None) is not None:
                raise ValueError(f"stream_stack: block {i}'s norm has a bias")
            if mx.d_conv != 4 or mx.d_state != 16:
                raise ValueError(f"stream_stack: block {i} has d_conv {mx.d_conv}, d_state {mx.d_state}; the middle kernel is built for 4 and 16")
            if (mx.d_model, mx.d_inner) not in aum_hip.STREAM_STACK_WIDTHS:
                raise ValueError(f"stream_stack: block {i} has widths ({mx.d_model}, {mx.d_inner}); the kernels are built for {aum_hip.STREAM_STACK_WIDTHS}")
            if layer.norm.eps != self.layers[0].norm.eps:
                raise ValueError("stream_stack: the blocks' norms differ in eps")
        stack = StreamStack(self, dtype)
        if not aum_hip.xdt_fwd_shape_ok(stack.ncols, stack.dim) or stack.rank % 8 or stack.rank + 32 > stack.ncols:
            raise ValueError(f"stream_stack: dt_rank {self.layers[0].mixer.dt_rank} gives x/dt rows of {stack.ncols} columns, which the middle kernel does not take")
        self.__dict__["_stream_stack"] = stack
        return stack

    def _stack_for(self, stack, hidden, layer_caches, seq_map, prefill, peek_every):
        """the stack a pass goes through, or None: the loop over the layers"""
        if stack is None or prefill or peek_every is not None:
            return None
        if not isinstance(stack, StreamStack):
            raise TypeError("stack= takes what AudioMamba.stream_stack() returns")
        stack = self.stream_stack(stack.dtype)                          # the cached one, or rebuilt where the parameters have moved on
        total = hidden.shape[0] * hidden.shape[1]
        max_len = hidden.shape[1] if seq_map is None else max(seq_map.lens)
        return stack if stack.takes(total, max_len) and stack.pools_ok(layer_caches) else None

    def _stream_layers(self, hidden, layer_caches, seq_map=None, commit=True, peek=False, prefill=False, peek_every=None, stack=None):
        """Block.forward (MM:58-99) for every layer on T new tokens, the mixers advancing `layer_caches` in place.  seq_map: hidden is
        (1, total, Dm), the packed tokens of several sessions, and the caches are pools (Mamba.step_chunk).  commit=False: the caches
        are read and not written.  peek=True: the last row of every session is computed and the caches advance by the rows before it.
        prefill=True (no peek row): the mixers take the tokens as a backlog (Mamba.prefill_chunk; with seq_map the packed backlogs of
        several sessions over pools).  peek_every=P (not with the others): a peek row behind every P committed rows of every session.
        stack (AudioMamba.stream_stack()): the whole loop as ONE aum_hip.stream_layers call where StreamStack.takes() the pass."""
        st = self._stack_for(stack, hidden, layer_caches, seq_map, prefill, peek_every)
        if st is not None:
            return self._run_stack(st, hidden, layer_caches, seq_map, commit, peek)
        residual = None
        for i, layer in enumerate(self.layers):
            hidden, residual = rms_norm_fn(hidden, layer.norm.weight, layer.norm.bias, residual=residual, prenorm=True,
                                           residual_in_fp32=True, eps=layer.norm.eps)
            conv_state, ssm_state = layer_caches[i]
            if prefill:
                hidden, _, _ = (layer.mixer.prefill_chunk(hidden, conv_state, ssm_state) if seq_map is None else
                                layer.mixer.prefill_chunk(hidden, conv_state, ssm_state, seq_map=seq_map))
            else:
                hidden, _, _ = layer.mixer.step_chunk(hidden, conv_state, ssm_state, seq_map=seq_map, commit=commit, peek=peek,
                                                      **({} if peek_every is None else {"peek_every": peek_every}))
        return hidden, residual

    @staticmethod
    def _run_stack(st, hidden, layer_caches, seq_map, commit, peek):
        """the pass of _stream_layers through a StreamStack that _stack_for has chosen"""
        import aum_hip
        batch, T, Dm = hidden.shape
        if seq_map is not None:
            aum_hip.check_seq_map("stream_layers", seq_map, T, layer_caches[0][0].shape[0], hidden.device)
        smap = seq_map if seq_map is not None else aum_hip.fixed_seq_map(batch, T, hidden.device)
        h, r = st.run(hidden.reshape(batch * T, Dm), layer_caches, smap, commit=commit, peek=peek)
        return h.view(batch, T, Dm), r.view(batch, T, Dm)

    def _read_in_place(self, cls, cache, rows):
        """stream_read without copies: the cls row of each session through the blocks ON the caches themselves, as one-token sessions on
        the rows read with nothing written back.  None where a block does not take the one-launch path (Mamba.step_chunk(commit=False)
        says so before it touches anything, and an uncommitted pass leaves no trace: the caller reads from copies instead)."""
        import aum_hip
        n = cls.shape[0]
        if cls.device.type != "cuda" or not aum_hip.debug.stream_fused:
            return None
        smap = aum_hip.fixed_seq_map(n, 1, cls.device) if rows is None else aum_hip.seq_map((1,) * n, rows, device=cls.device)
        try:
            hidden, residual = self._stream_layers(cls.reshape(1, n, -1), cache["layers"], smap, commit=False)
        except NotImplementedError:
            return None
        return hidden.reshape(n, 1, -1), residual.reshape(n, 1, -1)

    # ---- many sessions at different positions: a pool of caches, one pass per push -----------------
    def allocate_stream_pool(self, sessions, dtype=None):
        """Caches for `sessions` independent streaming sessions: per layer (conv_state, ssm_state) with one row per session, and one
        column count per session.  Rows are advanced by stream_push_many, read by stream_read(..., sessions=) and emptied for the
        next clip by stream_reset."""
        if int(sessions) < 1:
            raise ValueError("allocate_stream_pool: at least one session")
        pool = self.allocate_inference_cache(int(sessions), dtype=dtype)
        pool["columns"] = [0] * int(sessions)
        return pool

    @staticmethod
    def _is_pool(cache):
        return isinstance(cache["columns"], list)

    def _check_sessions(self, what, cache, sessions, writes=True):
        """the rows `sessions` names; writes: of a pool, and distinct (stream_read takes any cache and may read a row twice)"""
        if writes and not self._is_pool(cache):
            raise ValueError(f"{what} takes a pool from allocate_stream_pool")
        rows = [int(r) for r in sessions]
        if writes and len(set(rows)) != len(rows):
            raise ValueError(f"{what}: the sessions {rows} are not distinct")
        if rows and (min(rows) < 0 or max(rows) >= cache["batch"]):
            raise ValueError(f"{what}: the sessions {rows} are not all rows of a cache of {cache['batch']}")
        return rows

    def _embed_columns(self, spec4d, cols):
        """(B, 1, n_mels, 16 k) frames of k time columns -> their (B, k * nf, Dm) tokens, time-major, each with the position row of its
        (f, t) cell.  cols: where the k columns sit in the clip -- a slice, or an int64 index vector on the frames' device."""
        nf, nt = self.patch_grid_size
        x = self.patch_embed(spec4d)                                             # (B, nf * k, Dm), token index f * k + t
        Bsz, k = x.shape[0], x.shape[1] // nf
        pe = self.pos_embed.pos_embed[:, 1:].reshape(1, nf, nt, -1)
        pe = pe[:, :, cols] if isinstance(cols, slice) else pe.index_select(2, cols)
        return (x.reshape(Bsz, nf, k, -1) + pe).transpose(1, 2).reshape(Bsz, k * nf, -1)

    def _cls_row(self):
        return self.cls_token + self.pos_embed.pos_embed[:, :1]                  # (1, 1, Dm)

    def _head_rows(self, hidden, residual, return_features, row_scale=None):
        """final norm and head on (n, Dm) rows of the last block's output and residual.  row_scale (batch,): the stochastic-depth
        factors of the add (training); the n rows are then batch runs of n / batch rows, sample by sample"""
        if row_scale is not None:
            hidden, residual = (t.reshape(row_scale.shape[0], -1, t.shape[-1]) for t in (hidden, residual))
        f = rms_norm_fn(hidden, self.norm_f.weight, self.norm_f.bias, eps=self.norm_f.eps, residual=residual, prenorm=False,
                        residual_in_fp32=True, row_scale=row_scale)
        if row_scale is not None:
            f = f.reshape(-1, f.shape[-1])
        return f if return_features else self.head(f)

    @torch.no_grad()
    def stream_push_many(self, specs, pool, sessions, read=False, return_features=False, stack=None):
        """specs[i]: (16 k_i, n_mels), k_i >= 1 -- the next k_i time columns of the clip of session sessions[i] (distinct rows of a pool from
        allocate_stream_pool), every session at its own column offset and with its own hop size.  One patch-embed GEMM over the frames
        concatenated in time, each session's position rows gathered from its own offset, tokens time-major within a session, then ONE pass
        through all blocks on the packed tokens (Mamba.step_chunk(seq_map=): only the conv and the scan see the session boundaries).
        Returns the per-session column counts.  Every argument is checked before any cache is touched: a refused call changes nothing.
        read=True: the logits "if the clip ended now" of every session with the same pass -- the cls row rides behind each session's new
        tokens as a peek row (Mamba.step_chunk(peek=True): it sees the state the tokens produced, the caches do not take it in).
        Returns (column counts, logits (len(sessions), classes) in the order of `sessions`; features with return_features).
        stack (stream_stack()): the pass through the blocks as one library call (StreamStack); the patch embedding and the head stay."""
        import aum_hip
        ks, c0s, rows, specs = self._check_push("stream_push_many", specs, pool, sessions)
        nf, dev = self.patch_grid_size[0], specs[0].device
        smap = aum_hip.seq_map([k * nf + (1 if read else 0) for k in ks], rows, device=dev)
        x = self._pack_columns(specs, ks, c0s)
        out = None
        if read:                # a session's tokens, then its cls row; the last row of session i is row cu[i + 1] - 1 of the pack
            cls = self._cls_row()[0].to(x.dtype)
            pieces, at = [], 0
            for k in ks:
                pieces += [x[0, at:at + k * nf], cls]
                at += k * nf
            last = torch.tensor([sum(smap.lens[:i + 1]) - 1 for i in range(len(ks))], dtype=torch.int64)
            if dev.type == "cuda":
                last = last.pin_memory()
            last = last.to(dev, non_blocking=True)
            hidden, residual = self._stream_layers(torch.cat(pieces, dim=0).unsqueeze(0), pool["layers"], smap, peek=True, stack=stack)
            out = self._head_rows(hidden[0].index_select(0, last), residual[0].index_select(0, last), return_features)
        else:
            self._stream_layers(x, pool["layers"], smap, stack=stack)
        counts = self._commit_columns(pool, ks, rows)
        return (counts, out) if read else counts

    def stream_reset(self, pool, sessions):
        """Empty the caches and the column counts of those rows of a pool: the slots are free for new clips."""
        rows = self._check_sessions("stream_reset", pool, sessions)
        if rows:
            idx = torch.tensor(rows, dtype=torch.int64)
            for c, s in pool["layers"].values():
                ix = idx.to(c.device)
                c.index_fill_(0, ix, 0)
                s.index_fill_(0, ix, 0)
            for r in rows:
                pool["columns"][r] = 0

    def _check_push(self, what, specs, cache, sessions=None):
        """The checks of every call that advances caches (`what`: stream_push / stream_prefill and their _many forms), made before
        anything is touched -> (ks, c0s, rows, specs): the new columns and the columns so far of every session, its cache row and its
        piece.  sessions None: the fixed-batch form -- specs is ONE (batch, 16 k, n_mels) tensor for all rows of a cache from
        allocate_inference_cache (one k, one c0, rows None).  Else the pool form: specs[i] (16 k_i, n_mels) for row sessions[i] of a
        pool from allocate_stream_pool."""
        self._check_streamable()
        ph, pw = self.patch_embed.proj.kernel_size
        nf, nt = self.patch_grid_size
        if sessions is None:
            spec = specs
            if self._is_pool(cache):
                raise ValueError(f"{what} advances all rows of a cache from allocate_inference_cache together; a pool from "
                                 f"allocate_stream_pool is advanced by {what}_many(specs, pool, sessions)")
            if spec.dim() != 3 or spec.shape[0] != cache["batch"] or spec.shape[1] == 0 or spec.shape[1] % pw or spec.shape[2] // ph != nf:
                raise ValueError(f"{what} takes (batch={cache['batch']}, a positive multiple of {pw} frames, {nf * ph} mel bins), got {tuple(spec.shape)}")
            k, c0 = spec.shape[1] // pw, cache["columns"]
            if c0 + k > nt:
                raise ValueError(f"the clip has {nt} time columns: {c0} pushed, {k} more do not fit")
            return [k], [c0], None, [spec]
        rows = self._check_sessions(what, cache, sessions)
        specs = list(specs)
        if not rows or len(specs) != len(rows):
            raise ValueError(f"{what}: one spectrogram piece per session, got {len(specs)} for the sessions {rows}")
        ks = []
        for sp, r in zip(specs, rows):
            if sp.dim() != 2 or sp.shape[0] == 0 or sp.shape[0] % pw or sp.shape[1] // ph != nf:
                raise ValueError(f"{what} takes (a positive multiple of {pw} frames, {nf * ph} mel bins) per session, got "
                                 f"{tuple(sp.shape)} for session {r}")
            k = sp.shape[0] // pw
            if cache["columns"][r] + k > nt:
                raise ValueError(f"the clip has {nt} time columns: session {r} pushed {cache['columns'][r]}, {k} more do not fit")
            ks.append(k)
        return ks, [cache["columns"][r] for r in rows], rows, specs

    def _pack_columns(self, specs, ks, c0s):
        """The frames of several sessions, specs[i] (16 k_i, n_mels) from column c0s[i] on, concatenated in time -> their (1, sum k_i nf, Dm)
        packed tokens, a session's tokens contiguous and time-major, each with the position row of its own (f, t) cell: one patch-embed
        GEMM, the position rows gathered by one host-built index vector, uploaded like the sequence map"""
        dev = specs[0].device
        cols = torch.tensor([c0 + j for c0, k in zip(c0s, ks) for j in range(k)], dtype=torch.int64)
        if dev.type == "cuda":
            cols = cols.pin_memory()
        cols = cols.to(dev, non_blocking=True)
        return self._embed_columns(torch.cat(specs, dim=0).unsqueeze(0).unsqueeze(1).transpose(2, 3), cols)

    @staticmethod
    def _commit_columns(cache, ks, rows):
        """the column counts behind a pass -> the new counts (rows None: the one count of a fixed-batch cache)"""
        if rows is None:
            cache["columns"] += ks[0]
            return cache["columns"]
        for r, k in zip(rows, ks):
            cache["columns"][r] += k
        return [cache["columns"][r] for r in rows]

    @torch.no_grad()
    def stream_prefill(self, spec, cache, read=False, return_features=False):
        """stream_push for a BACKLOG: spec (batch, 16 k, n_mels), the next k time columns of the clip -- seconds or minutes of audio a
        client arrives with, or the part of a long-form clip recorded so far -- through all blocks from the carried caches, which advance
        by the k columns exactly as under stream_push (the same checks, the same column count; a refused call changes nothing), and
        stream_push / stream_read go on from there.  The blocks take the tokens through Mamba.prefill_chunk: the time-parallel conv and
        the token-major scan of the offline forward, long rows cut into time segments, instead of one serial chain of k n_f steps per
        wave.  The results agree with stream_push to the kernels' tolerance, not bitwise.
        It pays from about 64 columns (512 tokens) per session.  Measured on AuM-Base, bf16, batch 1, ONE run per size
        (profiles/r13_stream_prefill.txt): 64 columns 6.0 ms against 8.6 ms through stream_push, 512 columns (L = 4097) 6.6 ms against
        52.6 ms, but 31 columns 5.7 ms against 5.3 ms -- up to the 128 tokens of stream_push's one-launch path and a little beyond,
        stream_push is the faster call, and it keeps the live hops.  The crossing point lies between 248 and 512 tokens and has not been
        located more finely; a pass costs about 5.7 ms whatever the backlog (per block: a [window ; x] copy, a copy of the conv output
        and the window write-back next to the kernels -- not profiled).
        No peek row: read=True is stream_read behind the push -> (columns, logits)."""
        (k,), (c0,), _, _ = self._check_push("stream_prefill", spec, cache)
        x = self._embed_columns(spec.unsqueeze(1).transpose(2, 3), slice(c0, c0 + k))
        self._stream_layers(x, cache["layers"], prefill=True)
        n = self._commit_columns(cache, [k], None)
        return (n, self.stream_read(cache, return_features)) if read else n

    @torch.no_grad()
    def stream_prefill_many(self, specs, pool, sessions, packed=False):
        """The backlog path of a pool (not the per-hop path: that is stream_push_many, one packed pass): specs[i] (16 k_i, n_mels), the
        next k_i columns of session sessions[i] (distinct rows of a pool from allocate_stream_pool).  Every argument is checked before
        any cache is touched.  Returns the per-session column counts.  No peek row and no read=: callers use stream_read.
        packed=False: a loop over the sessions on the host -- each one's cache rows are gathered (index_select), advanced by
        stream_prefill's pass at batch 1 and scattered back (index_copy_); the other rows are not touched.  Bit for bit stream_prefill
        of each session alone.
        packed=True: ONE pass for all sessions -- one patch-embed GEMM over the frames concatenated in time, each session's position
        rows gathered from its own offset (as stream_push_many does), then all blocks once on the packed tokens through
        Mamba.prefill_chunk(seq_map=): only the conv and the scan see the session boundaries, and they advance the pool rows in place
        (no gather, no scatter).  The same caches and counts to the kernels' tolerance, not bitwise: the GEMMs see another M."""
        ks, c0s, rows, specs = self._check_push("stream_prefill_many", specs, pool, sessions)
        if packed:
            import aum_hip
            smap = aum_hip.seq_map([k * self.patch_grid_size[0] for k in ks], rows, device=specs[0].device)
            self._stream_layers(self._pack_columns(specs, ks, c0s), pool["layers"], smap, prefill=True)
            return self._commit_columns(pool, ks, rows)
        for sp, r, k, c0 in zip(specs, rows, ks, c0s):
            ix = torch.tensor([r], dtype=torch.int64, device=sp.device)
            one = {i: (c.index_select(0, ix), s.index_select(0, ix)) for i, (c, s) in pool["layers"].items()}
            x = self._embed_columns(sp.unsqueeze(0).unsqueeze(1).transpose(2, 3), slice(c0, c0 + k))
            self._stream_layers(x, one, prefill=True)
            for i, (c, s) in pool["layers"].items():
                c.index_copy_(0, ix, one[i][0])
                s.index_copy_(0, ix, one[i][1])
            self._commit_columns(pool, [k], [r])
        return [pool["columns"][r] for r in rows]

    @torch.no_grad()
    def stream_push(self, spec, cache, read=False, return_features=False, stack=None):
        """spec: (batch, 16 k, n_mels) -- the next k time columns of the clip's normalised log-mel spectrogram.  Embeds their
        k x n_f tokens (time-major, each with the position row of its (f, t) cell), runs them through all blocks from the carried caches
        and advances the caches.  Returns the number of columns pushed so far.
        This is the call for LIVE hops -- a few columns at a time, up to 128 tokens per session in one launch per block; a backlog
        (a client that joins with buffered audio, a long-form clip to be continued) goes through stream_prefill, which takes the same
        arguments and leaves the same caches.
        read=True: what stream_read would say behind this push, from the same pass -- the cls row rides behind the new tokens as a peek
        row (Mamba.step_chunk(peek=True)), goes through the final norm and the head, and the caches advance by the tokens only.
        Returns (columns, logits (batch, classes); features with return_features).
        stack (stream_stack()): the pass through the blocks as one library call (StreamStack), opt-in; the default path is unchanged."""
        (k,), (c0,), _, _ = self._check_push("stream_push", spec, cache)
        x = self._embed_columns(spec.unsqueeze(1).transpose(2, 3), slice(c0, c0 + k))
        if not read:
            self._stream_layers(x, cache["layers"], stack=stack)
            return self._commit_columns(cache, [k], None)
        x = torch.cat((x, self._cls_row().to(x.dtype).expand(x.shape[0], -1, -1)), dim=1)
        hidden, residual = self._stream_layers(x, cache["layers"], peek=True, stack=stack)
        return self._commit_columns(cache, [k], None), self._head_rows(hidden[:, -1], residual[:, -1], return_features)

    # ---- streaming from raw audio: PCM hops of any size, the log-mel stage carried by a WaveStream ----
    def allocate_wave_stream(self, sessions, frontend):
        """The state stream_push_wave / stream_push_wave_many carry next to a cache of `sessions` rows (allocate_inference_cache or
        allocate_stream_pool): an aum.frontend.WaveStream -- the pool of sample tails and the host counters.  frontend: an
        aum.frontend.WaveInput without aug / noise whose target_length is the model's clip (16 n_t frames), padded == 512 tables."""
        from .frontend import WaveStream
        self._check_streamable()
        return WaveStream(sessions, frontend, self.patch_embed.proj.kernel_size[1] * self.patch_grid_size[1], self.pos_embed.pos_embed.device)

    def _plan_wave(self, what, waves, cache, wave_stream, rows, end):
        """The checks of a push of raw audio, made before anything is touched -> the aum_hip.WaveMap of the call (host lists checked, one
        upload) and the whole new columns of every session.  waves[i] (m_i,) fp32 on the tails' device for row rows[i] (rows None: row i)."""
        import aum_hip
        from .frontend import WaveStream
        ws = wave_stream
        if not isinstance(ws, WaveStream):
            raise TypeError(f"{what}: wave_stream must come from allocate_wave_stream")
        if ws.sessions != cache["batch"]:
            raise ValueError(f"{what}: the wave stream was built for {ws.sessions} sessions, the cache has {cache['batch']} rows")
        pw, (nf, nt) = self.patch_embed.proj.kernel_size[1], self.patch_grid_size
        if ws.target_length != pw * nt or ws.frontend.tables.tables["mel_w"].shape[0] // self.patch_embed.proj.kernel_size[0] != nf:
            raise ValueError(f"{what}: the wave stream was built for clips of {ws.target_length} frames, the model's clip has {pw * nt}")
        idx = list(range(len(waves))) if rows is None else rows
        ends = [bool(end)] * len(idx) if isinstance(end, (bool, int)) else [bool(e) for e in end]
        if len(ends) != len(idx):
            raise ValueError(f"{what}: one end flag per session, got {len(ends)} for {len(idx)} sessions")
        ms, frames, n_real = [], [], []
        for w, r, e in zip(waves, idx, ends):
            if not torch.is_tensor(w) or w.dim() != 1 or w.dtype != torch.float32 or w.device != ws.tails.device:
                got = f"{tuple(w.shape)} {w.dtype} on {w.device}" if torch.is_tensor(w) else type(w).__name__
                raise ValueError(f"{what} takes (samples,) fp32 on {ws.tails.device} per session, got {got} for session {r}")
            if ws.ended[r]:
                raise ValueError(f"{what}: the clip of session {r} has ended; stream_reset and wave_stream.reset free the row")
            done = cache["columns"][r] if self._is_pool(cache) else cache["columns"]
            if done * pw != ws.frames[r]:
                raise ValueError(f"{what}: session {r} has {done} columns in the cache and {ws.frames[r]} frames in the wave stream: they "
                                 "do not belong together")
            n = ws.samples[r] + w.shape[0]
            if n > ws.max_samples:
                raise ValueError(f"the clip has {ws.max_samples} samples ({nt} time columns): session {r} pushed {ws.samples[r]}, "
                                 f"{w.shape[0]} more do not fit")
            avail = 0 if n < ws.win else 1 + (n - ws.win) // ws.shift
            ms.append(w.shape[0])
            frames.append(ws.target_length - ws.frames[r] if e else (avail - ws.frames[r]) // pw * pw)
            n_real.append(avail if e else -1)
        wmap = aum_hip.wave_map(ms, [ws.tail_len[r] for r in idx], frames, [ws.frames[r] for r in idx], n_real, rows, device=ws.tails.device,
                                win=ws.win, shift=ws.shift)
        return wmap, [f // pw for f in frames], ends

    def _wave_frames(self, wave, wmap, wave_stream, idx, ends):
        """the one fbank_stream launch of a push and the host counters behind it -> the new frames (total, n_mels)"""
        import aum_hip
        ws, fe = wave_stream, wave_stream.frontend
        frames = aum_hip.fbank_stream(wave, wmap, ws.tails, fe.tables.tables, fe.norm_mean, fe.norm_std)
        for i, r in enumerate(idx):
            ws.tail_len[r], ws.samples[r], ws.frames[r] = wmap.new_tail_lens[i], ws.samples[r] + wmap.samples[i], ws.frames[r] + wmap.frames[i]
            ws.ended[r] = ws.ended[r] or ends[i]
        return frames.to(self.patch_embed.proj.weight.dtype)        # a model held in 16 bits takes its frames in 16 bits (no-op in fp32)

    @torch.no_grad()
    def stream_push_wave_many(self, waves, pool, wave_stream, sessions, read=False, end=False, return_features=False, stack=None):
        """stream_push_many from RAW AUDIO: waves[i] (m_i,) fp32 on the device, m_i >= 0 -- the next samples of the clip of session
        sessions[i] (distinct rows of a pool from allocate_stream_pool), in hops of any size.  wave_stream (allocate_wave_stream) holds
        what the hops leave over: the 240 samples neighbouring frames share and the samples of a column that is not whole yet.  The host
        works out how many whole new columns k_i every session covers; their frames come from ONE fbank_stream launch (every frame
        bit-identical to the same row of fbank_fwd on the whole clip, however the stream is cut), the sessions with k_i >= 1 go through
        stream_push_many unchanged, the others only grow their tail.  Returns what stream_push_many returns, in the order of `sessions`;
        with read=True a session without a new column is read by stream_read.
        end (a bool, or one per session): the clip ends with these samples -- its remaining real frames (1 + (n - win) // shift of
        the n samples pushed, none if n < win) and the padding rows up to the clip's 16 n_t frames are pushed, stream_read then equals the
        model on fbank_fwd(whole wave, target_length), and the session refuses further pushes until stream_reset(pool, rows) and
        wave_stream.reset(rows).  Samples beyond the clip's frame grid (n > win + (16 n_t - 1) shift) do not fit, with or without end.
        Every argument is checked before anything is written: a refused call changes neither tails nor counters nor caches.
        The offline loader subtracts the clip's mean before the kernel, which a stream cannot; the kernel removes each frame's own mean
        first, so a constant offset cancels in exact arithmetic (the fp32 residual measured on a test tone is stated in DESIGN.md)."""
        self._check_streamable()
        rows = self._check_sessions("stream_push_wave_many", pool, sessions)
        waves = list(waves)
        if not rows or len(waves) != len(rows):
            raise ValueError(f"stream_push_wave_many: one waveform piece per session, got {len(waves)} for the sessions {rows}")
        wmap, ks, ends = self._plan_wave("stream_push_wave_many", waves, pool, wave_stream, rows, end)
        frames = self._wave_frames(waves[0] if len(waves) == 1 else torch.cat(waves), wmap, wave_stream, rows, ends)
        pieces = frames.split(list(wmap.frames), dim=0)
        go = [i for i, k in enumerate(ks) if k >= 1]
        out = None
        if go:
            out = self.stream_push_many([pieces[i] for i in go], pool, [rows[i] for i in go], read=read, return_features=return_features, stack=stack)
        counts = [pool["columns"][r] for r in rows]
        if not read:
            return counts
        if len(go) == len(rows):
            return counts, out[1]
        stay = [i for i, k in enumerate(ks) if k < 1]
        quiet = self.stream_read(pool, return_features, sessions=[rows[i] for i in stay], stack=stack)
        if not go:
            return counts, quiet
        order = torch.tensor(go + stay, dtype=torch.int64).argsort().to(quiet.device)
        return counts, torch.cat((out[1].to(quiet.dtype), quiet), dim=0).index_select(0, order)

    @torch.no_grad()
    def stream_push_wave(self, wave, cache, wave_stream, read=False, end=False, return_features=False, stack=None):
        """stream_push from raw audio, the fixed-batch, lockstep form: wave (batch, m) fp32, the next m >= 0 samples of every row of a
        cache from allocate_inference_cache; the same kernel as stream_push_wave_many under a map in which session b owns row b.  Whole
        new columns go through stream_push; returns the columns pushed so far, with read=True (columns, logits) -- stream_read where no
        column was completed.  end (one bool): the clips end here, as in stream_push_wave_many."""
        self._check_streamable()
        if self._is_pool(cache):
            raise ValueError("stream_push_wave advances all rows of a cache from allocate_inference_cache together; a pool from "
                             "allocate_stream_pool is advanced by stream_push_wave_many(waves, pool, wave_stream, sessions)")
        if not torch.is_tensor(wave) or wave.dim() != 2 or wave.shape[0] != cache["batch"] or not isinstance(end, (bool, int)):
            raise ValueError(f"stream_push_wave takes (batch={cache['batch']}, samples) fp32 and one end flag, got "
                             f"{tuple(wave.shape) if torch.is_tensor(wave) else type(wave).__name__}")
        wave = wave.contiguous()
        wmap, ks, ends = self._plan_wave("stream_push_wave", list(wave), cache, wave_stream, None, end)
        frames = self._wave_frames(wave.reshape(-1), wmap, wave_stream, range(wave.shape[0]), ends)
        if ks[0] >= 1:
            return self.stream_push(frames.reshape(wave.shape[0], wmap.frames[0], -1), cache, read=read, return_features=return_features, stack=stack)
        return (cache["columns"], self.stream_read(cache, return_features, stack=stack)) if read else cache["columns"]

    # ---- parking sessions: a session's rows off a pool and back, into any free rows of any pool of the same model --------
    def _park_tensors(self, cache, wave_stream):
        """the pool tensors a session has a row in, in record order: per layer (conv_state, ssm_state), then the sample tails"""
        ts = [t for i in sorted(cache["layers"]) for t in cache["layers"][i]]
        return ts + ([wave_stream.tails] if wave_stream is not None else [])

    def _park_signature(self, what, cache, wave_stream):
        """(depth, d_inner, d_conv, d_state, cache dtype, tail width) of a cache (and its wave stream): what a record's layout depends on"""
        from .frontend import WaveStream
        if not cache["layers"]:
            raise ValueError(f"{what}: the cache has no layers")
        c, s = cache["layers"][min(cache["layers"])]
        if any(cc.shape[1:] != c.shape[1:] or ss.shape[1:] != s.shape[1:] or cc.dtype != c.dtype or ss.dtype != s.dtype or s.dtype != c.dtype
               for cc, ss in cache["layers"].values()):
            raise ValueError(f"{what}: the layers' caches differ in shape or dtype")
        if wave_stream is not None:
            if not isinstance(wave_stream, WaveStream):
                raise TypeError(f"{what}: wave_stream must come from allocate_wave_stream")
            if wave_stream.sessions != cache["batch"] or wave_stream.tails.device != c.device:
                raise ValueError(f"{what}: the wave stream was built for {wave_stream.sessions} sessions on {wave_stream.tails.device}, the cache "
                                 f"has {cache['batch']} rows on {c.device}")
        return (len(cache["layers"]), c.shape[1], c.shape[2], s.shape[2], c.dtype, 0 if wave_stream is None else wave_stream.cap)

    def _check_park_rows(self, what, cache, sessions):
        """_check_sessions for a park / resume / fork: a pool or a fixed-batch cache (its rows are sessions too), at least one row, distinct"""
        rows = self._check_sessions(what, cache, sessions, writes=self._is_pool(cache))
        if not rows:
            raise ValueError(f"{what}: at least one session")
        if len(set(rows)) != len(rows):
            raise ValueError(f"{what}: the sessions {rows} are not distinct")
        return rows

    @staticmethod
    def _park_kernel(tensors):
        """the library whose aum_stream_park moves the rows, or None: plain indexed copies (CPU tensors without a host-pointer library).
        Device tensors always take the kernel: a missing library is an error there, as everywhere."""
        import aum_hip
        if tensors[0].device.type == "cuda":
            return aum_hip.get()
        lib = aum_hip._product
        return lib if lib is not None and lib.host else None

    @staticmethod
    def _park_copies(tensors, rows, blob, restore):
        """The un-fused twin of aum_hip.stream_park, one indexed copy per pool tensor: the same records byte for byte."""
        import aum_hip
        lay = aum_hip.stream_park_layout(tensors)
        n = len(rows)
        if blob is None:
            blob = torch.zeros((n, lay.record), dtype=torch.uint8, device=tensors[0].device)
        idx = torch.tensor(rows, dtype=torch.int64).to(tensors[0].device)
        for t, off, nb in zip(tensors, lay.offsets, lay.row_bytes):
            if restore:
                t.index_copy_(0, idx, blob[:, off:off + nb].contiguous().view(t.dtype).reshape((n,) + tuple(t.shape[1:])))
            else:
                blob[:, off:off + nb] = t.index_select(0, idx).reshape(n, -1).view(torch.uint8)
        return blob

    def _park_move(self, tensors, rows, blob, restore):
        import aum_hip
        lib = self._park_kernel(tensors)
        if lib is None:
            return self._park_copies(tensors, rows, blob, restore)
        return aum_hip.stream_park(tensors, rows, blob, restore=restore, lib=lib)

    @torch.no_grad()
    def stream_park(self, cache, sessions, wave_stream=None, to_host=False):
        """Take sessions off a pool: everything the rows `sessions` of `cache` (a pool from allocate_stream_pool, or a fixed-batch cache
        from allocate_inference_cache, whose rows are sessions too) carry -- per layer the conv window and the scan state, the column
        counts and, with wave_stream= (the WaveStream carried next to the cache), the sample tails and their counters -- as one
        ParkedSessions, in the order of `sessions`.  ONE launch (aum_hip.stream_park) whatever the depth; to_host=True: plus one copy
        of the blob into pinned host memory (the call then waits for the stream).  Parking is a read: the pool keeps the rows, the caller
        decides when to stream_reset them.  The kernels that advance a session give the same bits under any pool row, so a session
        resumed from its record continues bit for bit.  Every argument is checked first: a refused call changes nothing."""
        self._check_streamable()
        rows = self._check_park_rows("stream_park", cache, sessions)
        sig = self._park_signature("stream_park", cache, wave_stream)
        pool_cols = cache["columns"]
        columns = [pool_cols[r] for r in rows] if self._is_pool(cache) else [pool_cols] * len(rows)
        wave = None
        if wave_stream is not None:
            ws, pw = wave_stream, self.patch_embed.proj.kernel_size[1]
            for r, c in zip(rows, columns):
                if c * pw != ws.frames[r]:
                    raise ValueError(f"stream_park: session {r} has {c} columns in the cache and {ws.frames[r]} frames in the wave stream: they "
                                     "do not belong together")
            wave = {k: [getattr(ws, k)[r] for r in rows] for k in ParkedSessions.WAVE_KEYS}
        blob = self._park_move(self._park_tensors(cache, wave_stream), rows, None, False)
        if to_host and blob.device.type == "cuda":
            host = torch.empty(blob.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(blob)
            blob = host
        return ParkedSessions(blob, columns, wave, sig)

    @torch.no_grad()
    def stream_resume(self, state, cache, sessions, wave_stream=None):
        """Bring parked sessions back: state[i] into row sessions[i] of `cache` -- any cache of the same layout (depth, d_inner, d_conv,
        d_state, cache dtype; with a sample tail, wave_stream= and the same tail width), any distinct rows, whatever they hold -- with
        its column count and, with wave_stream=, its tail and counters.  ONE launch; a host blob is uploaded with one copy first.
        Refused before anything is written: another layout, a blob of another record size, rows that are not distinct or not rows of
        the cache, a session count other than len(state), a wave stream missing or unexpected.  A fixed-batch cache keeps ONE column
        count for all rows: it takes sessions that are at its own count, or all of its rows at once at one count."""
        import aum_hip
        self._check_streamable()
        if not isinstance(state, ParkedSessions):
            raise TypeError("stream_resume: state must come from stream_park")
        rows = self._check_park_rows("stream_resume", cache, sessions)
        sig = self._park_signature("stream_resume", cache, wave_stream)
        if sig != state.signature:
            raise ValueError(f"stream_resume: the sessions were parked from caches of layout {state.signature}, these are {sig} "
                             "(depth, d_inner, d_conv, d_state, cache dtype, tail width)")
        if len(rows) != len(state):
            raise ValueError(f"stream_resume: {len(state)} parked sessions for the rows {rows}")
        tensors = self._park_tensors(cache, wave_stream)
        record = aum_hip.stream_park_layout(tensors).record
        if state.blob.dim() != 2 or state.blob.dtype != torch.uint8 or tuple(state.blob.shape) != (len(rows), record):
            raise ValueError(f"stream_resume: the blob is {tuple(state.blob.shape)} {state.blob.dtype}, these caches take ({len(rows)}, {record}) uint8")
        if not self._is_pool(cache) and any(c != cache["columns"] for c in state.columns) and not (
                len(rows) == cache["batch"] and len(set(state.columns)) == 1):
            raise ValueError(f"stream_resume: a cache from allocate_inference_cache keeps one column count ({cache['columns']}) for all rows; "
                             f"the sessions are at {state.columns}")
        dev = tensors[0].device
        blob = state.blob if state.blob.device == dev else state.blob.to(dev, non_blocking=True)
        self._park_move(tensors, rows, blob, True)
        if self._is_pool(cache):
            for r, c in zip(rows, state.columns):
                cache["columns"][r] = c
        else:
            cache["columns"] = state.columns[0]
        if wave_stream is not None:
            for k in ParkedSessions.WAVE_KEYS:
                for r, v in zip(rows, state.wave[k]):
                    getattr(wave_stream, k)[r] = v

    @torch.no_grad()
    def stream_fork(self, cache, src, dst, wave_stream=None):
        """Copy session `src` of a cache into the rows `dst` of the same cache (distinct, not src): a park of one session and a resume
        of every dst row from that one record, two launches on the device, src untouched.  The forks continue bit for bit as src
        would -- to score several continuations of one prefix."""
        rows = self._check_park_rows("stream_fork", cache, list(dst))
        (s,) = self._check_park_rows("stream_fork", cache, [src])
        if s in rows:
            raise ValueError(f"stream_fork: the source session {s} is among the destinations {rows}")
        state = self.stream_park(cache, [s], wave_stream=wave_stream)
        self.stream_resume(state.select([0] * len(rows)), cache, rows, wave_stream=wave_stream)

    def _with_cls_rows(self, x):
        """(B, K n_f, Dm) time-major tokens of K columns -> (B, K (n_f + 1), Dm): the cls row behind every column's n_f tokens"""
        nf = self.patch_grid_size[0]
        Bsz, K = x.shape[0], x.shape[1] // nf
        cls = self._cls_row().to(x.dtype).reshape(1, 1, 1, -1).expand(Bsz, K, 1, -1)
        return torch.cat((x.reshape(Bsz, K, nf, -1), cls), dim=2).reshape(Bsz, K * (nf + 1), -1)

    def _timeline_rows(self, hidden, residual, return_features, row_scale=None):
        """the cls rows of _with_cls_rows' layout out of the last block's output and residual -> (B K, classes): final norm and head"""
        nf = self.patch_grid_size[0]
        pick = lambda t: t.reshape(-1, nf + 1, t.shape[-1])[:, nf]
        return self._head_rows(pick(hidden), pick(residual), return_features, row_scale)

    def forward_timeline(self, spec, return_features=False, frontend=None):
        """The differentiable counterpart of stream_timeline from column 0 -- TRAINING for the per-column logits: spec (batch, 16 K,
        n_mels) frames of the first K time columns of a clip (1 <= K <= the grid's column count) -> logits (batch, K, classes);
        logits[:, j] is the model's output "if the clip ended behind column j", the last of a full clip is model(spec).  One pass over
        the rows [column 0's n_f tokens | cls | column 1's tokens | cls | ...]: every block runs Mamba.forward(peek_every=n_f), whose cls
        rows read the conv window and the state and enter neither (HIP kernels both ways).  Causal models only (_check_streamable).
        frontend=aum.frontend.WaveInput: spec is the (batch, n_samples) waveform; it goes through the log-mel kernel first (the fused
        waveform -> tokens kernel writes the offline token layout, cls once).
        In eval mode and at drop_path_rate 0 the path is deterministic, as the offline forward is; in training with a rate it draws
        drop_scales once, as the offline forward does (a dropped sample skips a block's input at all of its rows)."""
        self._check_streamable()
        if frontend is not None:
            spec = frontend.spectrogram(spec)
        nf, nt = self.patch_grid_size
        if spec.dim() != 3 or spec.shape[1] < 16 or spec.shape[1] % 16 or spec.shape[1] > 16 * nt or spec.shape[2] != 16 * nf:
            raise ValueError(f"forward_timeline: spec must be (batch, 16 K, {16 * nf}) frames of K = 1 .. {nt} time columns, not {tuple(spec.shape)}")
        K = spec.shape[1] // 16
        hidden = self._with_cls_rows(self._embed_columns(spec.unsqueeze(1).transpose(2, 3), slice(0, K)))
        scales = self._drop(hidden)
        residual = None
        for i, layer in enumerate(self.layers):
            hidden, residual = rms_norm_fn(hidden, layer.norm.weight, layer.norm.bias, residual=residual, prenorm=True,
                                           residual_in_fp32=True, eps=layer.norm.eps,
                                           row_scale=None if scales is None or residual is None else scales[i])
            hidden = layer.mixer(hidden, peek_every=nf)
        out = self._timeline_rows(hidden, residual, return_features, None if scales is None else scales[-1])
        return out.reshape(spec.shape[0], K, -1)

    @torch.no_grad()
    def stream_timeline(self, spec, cache, return_features=False):
        """The logits "if the clip ended now" after EVERY one of the next k time columns, in one pass: spec (batch, 16 k, n_mels) as
        stream_push takes it (the same checks; a refused call changes nothing).  The rows of a batch entry are
        [column c0's n_f tokens | cls | column c0 + 1's tokens | cls | ...]: every cls row is a peek row (Mamba.step_chunk(peek_every=n_f))
        -- it sees the state the columns up to its own produced and is not taken into the caches.  Returns (columns, logits
        (batch, k, classes); features with return_features): logits[:, j] is what stream_push(column c0 + j, read=True) would have
        returned, to the kernels' tolerance (the GEMMs see another row count).  The caches and the column count advance as under
        stream_push of the k columns: stream_push / stream_read / stream_prefill / stream_timeline go on from there."""
        (k,), (c0,), _, _ = self._check_push("stream_timeline", spec, cache)
        x = self._with_cls_rows(self._embed_columns(spec.unsqueeze(1).transpose(2, 3), slice(c0, c0 + k)))
        hidden, residual = self._stream_layers(x, cache["layers"], peek_every=self.patch_grid_size[0])
        out = self._timeline_rows(hidden, residual, return_features)
        return self._commit_columns(cache, [k], None), out.reshape(x.shape[0], k, -1)

    @torch.no_grad()
    def stream_timeline_many(self, specs, pool, sessions, return_features=False):
        """stream_timeline on a pool: specs[i] (16 k_i, n_mels), the next k_i columns of session sessions[i] (distinct rows of a pool from
        allocate_stream_pool), every session at its own offset and with its own k_i, in ONE packed pass -- packer, position rows and
        sequence map as in stream_push_many, the sessions k_i (n_f + 1) rows long.  Returns (the per-session column counts,
        [logits_i (k_i, classes)] in the order of `sessions`)."""
        import aum_hip
        ks, c0s, rows, specs = self._check_push("stream_timeline_many", specs, pool, sessions)
        nf = self.patch_grid_size[0]
        smap = aum_hip.seq_map([k * (nf + 1) for k in ks], rows, device=specs[0].device)
        x = self._with_cls_rows(self._pack_columns(specs, ks, c0s))
        hidden, residual = self._stream_layers(x, pool["layers"], smap, peek_every=nf)
        out = self._timeline_rows(hidden, residual, return_features)
        return self._commit_columns(pool, ks, rows), list(out.split(ks, dim=0))

    @torch.no_grad()
    def stream_read(self, cache, return_features=False, sessions=None, stack=None):
        """Logits if the clip ended now: the cls row run through the blocks from the caches, which are NOT advanced (read in place where
        every block takes the one-launch path, Mamba.step_chunk(commit=False); otherwise from a copy -- also where a row is named
        twice), then the final norm and the head.  After all columns of a clip have been pushed this is model(spec).  sessions: read
        those rows only, (len(sessions), ...) in that order; None: every row (of a pool too).
        stack (stream_stack()): the uncommitted in-place pass as one library call where the stack takes it (distinct rows)."""
        self._check_streamable()
        rows = None
        if sessions is not None:
            rows = self._check_sessions("stream_read", cache, sessions, writes=False)
            if not rows:
                raise ValueError("stream_read: at least one session")
        cls = self._cls_row().expand(cache["batch"] if rows is None else len(rows), -1, -1)
        done = None
        if stack is not None and (rows is None or len(set(rows)) == len(rows)):
            import aum_hip
            n = cls.shape[0]
            smap = aum_hip.fixed_seq_map(n, 1, cls.device) if rows is None else aum_hip.seq_map((1,) * n, rows, device=cls.device)
            st = self._stack_for(stack, cls.reshape(1, n, -1), cache["layers"], smap, False, None)
            if st is not None:
                hidden, residual = self._run_stack(st, cls.reshape(1, n, -1), cache["layers"], smap, False, False)
                done = hidden.reshape(n, 1, -1), residual.reshape(n, 1, -1)
        if done is None:
            done = self._read_in_place(cls, cache, rows) if rows is None or len(set(rows)) == len(rows) else None
        if done is not None:
            hidden, residual = done
        else:
            if rows is None:
                copies = {i: (c.clone(), s.clone()) for i, (c, s) in cache["layers"].items()}
            else:
                idx = torch.tensor(rows, dtype=torch.int64)
                copies = {i: (c.index_select(0, idx.to(c.device)), s.index_select(0, idx.to(s.device))) for i, (c, s) in cache["layers"].items()}
            hidden, residual = self._stream_layers(cls, copies)
        return self._head_rows(hidden[:, 0], residual[:, 0], return_features)

    def forward(self, x, return_features=False, frontend=None, timeline=False, if_random_cls_token_position=False):
        """x: (B, T, F) normalised log-mel spectrogram, or -- with frontend=aum.frontend.WaveInput -- (B, n_samples) waveform.
        timeline=True: forward_timeline on the same arguments, (B, K, classes) (so that a DistributedDataParallel wrapper reaches it)"""
        if timeline:
            return self.forward_timeline(x, return_features, frontend)
        f = self.forward_features(x, frontend, if_random_cls_token_position)
        if return_features:
            return f
        out = self.head(f)
        return out.max(dim=1)[0] if f.dim() == 3 else out          # MM:683-684: final_pool_type 'max' over the tokens' logits


def _init_weights(module, n_layer):
    """MM:146-176: zero Linear biases (unless _no_reinit), rescale out_proj by 1/sqrt(n_layer)."""
    if isinstance(module, nn.Linear) and module.bias is not None and not getattr(module.bias, "_no_reinit", False):
        nn.init.zeros_(module.bias)
    if isinstance(module, Mamba):
        nn.init.kaiming_uniform_(module.out_proj.weight, a=math.sqrt(5))
        with torch.no_grad():
            module.out_proj.weight /= math.sqrt(n_layer)


def build_aum(size="base", **kw):
    return AudioMamba(embed_dim=AUM_SIZES[size], **kw)
