"""Loading pretrained weights into aum.model.AudioMamba.

`--aum_pretrain` -- the reference's published AuM checkpoints (/root/reference/src/models/mamba_models.py = "MM":397-446),
load_aum_checkpoint:

  * DDP/accelerate `module.` prefixes are stripped (MM:400);
  * the absolute position embedding is re-gridded when the clip length differs from the checkpoint's: the cls row is
    kept, the patch rows are bilinearly resampled with antialiasing on the (freq, time) grid
    (/root/reference/src/utilities/tokenization.py = "TOK":26-66, 357-369); the old grid is recovered from the row count
    assuming 128 mel bins and a power-of-two clip length, as the reference does (MM:419-429);
  * a head with a different class count is dropped (MM:440-444);
  * the patch projection must have the model's patch size (the pseudo-inverse patch resize belongs to the
    flexible-patch path, which is out of scope).

`--imagenet_pretrain` -- an ImageNet Vim checkpoint (e.g. vim_s_midclstok: 3-channel 16 x 16 patches at 224 x 224, the cls
position row in the middle of the sequence) as the backbone of AuM-Small (MM:348-395), load_imagenet_checkpoint:

  * the state dict under `modelkey` ("model") is read; `pos_embed` is the model's `pos_embed.pos_embed`;
  * a 1-channel model takes the patch weight averaged over the input channels;
  * the cls position row is moved from the middle (row N // 2 of N + 1) -- or, with load_middle_cls_token=False, taken
    from row 0 -- to the front, and the square source grid (14 x 14 for 224 x 224) is re-gridded to the model's
    (8 x 64 for 1024 frames, 8 x 8 for 128) by resample_pos_embed;
  * the patch and position weights are written into the model's own parameters; every other key but `head.*` (always
    dropped: ImageNet's classifier is no use here) goes through load_state_dict(strict=False), so a Vim Bi-Bi checkpoint
    also initialises a Fo-Bi model (the backward-direction conv / x_proj / dt_proj / D_b are reported as unexpected).
    The returned missing and unexpected keys are those the reference prints.
  * load_double_cls_token=True (a double-cls Vim checkpoint into a use_double_cls_token model): the first and the last position row
    go to the prefix (rows 0 and 1), cls_token_head / cls_token_tail load by name; mismatched cls layouts are refused.
  * refused: another patch size.
"""
import math

import torch
import torch.nn.functional as F
from torch.nn.modules.module import _IncompatibleKeys


def _grid(fstride, tstride, patch, fdim, tdim):
    return (fdim - patch[0]) // fstride + 1, (tdim - patch[1]) // tstride + 1


def resample_pos_embed(pos_embed, old_grid, new_grid, n_prefix=1):
    if tuple(old_grid) == tuple(new_grid):
        return pos_embed
    prefix, grid = pos_embed[:, :n_prefix], pos_embed[:, n_prefix:]
    grid = grid.reshape(1, old_grid[0], old_grid[1], -1).permute(0, 3, 1, 2).float()
    grid = F.interpolate(grid, size=tuple(new_grid), mode="bilinear", antialias=True)
    grid = grid.permute(0, 2, 3, 1).reshape(1, new_grid[0] * new_grid[1], -1).to(pos_embed.dtype)
    return torch.cat([prefix, grid], dim=1)


def load_aum_checkpoint(model, weights, pretrain_fstride=None, pretrain_tstride=None, strict_backbone=True):
    """weights: path or state dict.  Returns torch's load_state_dict result (missing / unexpected keys)."""
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu")
    weights = {k.replace("module.", ""): v for k, v in weights.items()}

    proj_w = weights["patch_embed.proj.weight"]
    patch_load = tuple(proj_w.shape[-2:])
    if patch_load != tuple(model.patch_embed.proj.kernel_size):
        raise NotImplementedError(f"checkpoint patch size {patch_load} != model {model.patch_embed.proj.kernel_size}")
    strides_load = (pretrain_fstride or patch_load[0], pretrain_tstride or patch_load[1])

    pe = weights["pos_embed.pos_embed"]
    n_prefix = model.num_tokens
    if pe.shape[1] != model.pos_embed.pos_embed.shape[1]:
        old = None
        for log_len in range(6, 20):
            g = _grid(*strides_load, patch_load, 128, 2 ** log_len)
            if g[0] * g[1] == pe.shape[1] - n_prefix:
                old = g
                break
        if old is None:
            raise ValueError("Could not find matching audio length")
        weights["pos_embed.pos_embed"] = resample_pos_embed(pe, old, model.patch_grid_size, n_prefix)

    if "head.weight" in weights and weights["head.weight"].shape[0] != model.num_classes:
        print("Num classes differ! Can only load the backbone weights.")
        del weights["head.weight"], weights["head.bias"]

    result = model.load_state_dict(weights, strict=False)
    if strict_backbone:
        bad = [k for k in result.missing_keys if not k.startswith("head.")] + list(result.unexpected_keys)
        if bad:
            raise RuntimeError(f"checkpoint does not match the AuM backbone: {bad[:8]}")
    return result


def load_imagenet_checkpoint(model, weights, modelkey="model", load_middle_cls_token=True, load_double_cls_token=False):
    """weights: path or the checkpoint's dict (the state dict under `modelkey`).  Returns torch's load_state_dict result with
    the missing / unexpected keys of the reference's own load (MM:393-394: the patch and position weights are not part of it)."""
    if weights is None:
        raise ValueError("ImageNet init needs a checkpoint: --imagenet_pretrain_path / imagenet_pretrain_path is not set")
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu")
    if not isinstance(weights, dict) or modelkey not in weights:
        found = sorted(weights) if isinstance(weights, dict) else type(weights).__name__
        raise KeyError(f"ImageNet checkpoint has no {modelkey!r} entry (found: {found}); set --imagenet_pretrain_modelkey")
    weights = dict(weights[modelkey])
    for k in ("pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"):
        if k not in weights:
            raise KeyError(f"ImageNet checkpoint has no {k!r}: not a Vim state dict")

    double_ckpt = "cls_token_head" in weights or "cls_token_tail" in weights
    if load_double_cls_token and model.num_tokens != 2:
        raise NotImplementedError("load_double_cls_token=True loads a double-cls Vim checkpoint: the model needs use_double_cls_token=True "
                         f"(it has {model.num_tokens} cls token(s))")
    if double_ckpt != bool(load_double_cls_token) or (model.num_tokens == 2) != bool(load_double_cls_token):
        raise ValueError(f"cls layouts do not match: the checkpoint is {'double' if double_ckpt else 'single'}-cls, the model has "
                         f"{model.num_tokens} cls token(s), load_double_cls_token={bool(load_double_cls_token)}")

    proj = model.patch_embed.proj
    proj_w = weights.pop("patch_embed.proj.weight").float()
    proj_b = weights.pop("patch_embed.proj.bias").float()
    if proj.in_channels == 1:
        proj_w = proj_w.mean(1, keepdim=True)
    if tuple(proj_w.shape[-2:]) != tuple(proj.kernel_size):
        raise NotImplementedError(f"checkpoint patch size {tuple(proj_w.shape[-2:])} != model {proj.kernel_size}")

    pe = weights.pop("pos_embed").float()
    if pe.dim() != 3 or pe.shape[0] != 1:
        raise ValueError(f"ImageNet pos_embed has shape {tuple(pe.shape)}, expected (1, rows, dim)")
    if load_double_cls_token:                                  # FlexiPosEmbed.insert_to_prefix(pe, [0, last]): head row, tail row, patches
        last = pe.shape[1] - 1
        pe = torch.cat([pe[:, :1], pe[:, last:], pe[:, 1:last]], dim=1)
    elif load_middle_cls_token:                                # FlexiPosEmbed.insert_to_prefix(pe, N // 2), TOK:411-422
        mid = (pe.shape[1] - 1) // 2
        pe = torch.cat([pe[:, mid:mid + 1], pe[:, :mid], pe[:, mid + 1:]], dim=1)
    n_prefix = model.num_tokens
    side = math.isqrt(max(pe.shape[1] - n_prefix, 0))
    if side * side != pe.shape[1] - n_prefix or side == 0:
        raise ValueError(f"ImageNet pos_embed has {pe.shape[1] - n_prefix} patch rows: not a square grid")
    pe = resample_pos_embed(pe, (side, side), model.patch_grid_size, n_prefix)

    for k in [k for k in weights if k.startswith("head.")]:     # the backbone only (MM:387-389)
        del weights[k]
    own = model.state_dict()
    bad = [(k, tuple(v.shape), tuple(own[k].shape)) for k, v in weights.items() if k in own and v.shape != own[k].shape]
    for name, got, want in (("patch_embed.proj.weight", proj_w, proj.weight), ("patch_embed.proj.bias", proj_b, proj.bias),
                            ("pos_embed.pos_embed", pe, model.pos_embed.pos_embed)):
        if got.shape != want.shape:
            bad.insert(0, (name, tuple(got.shape), tuple(want.shape)))
    if bad:
        raise ValueError("ImageNet checkpoint does not fit the model (key, checkpoint shape, model shape): %s" % bad[:8])

    with torch.no_grad():
        proj.weight.copy_(proj_w)
        proj.bias.copy_(proj_b)
        model.pos_embed.pos_embed.copy_(pe)
    result = model.load_state_dict(weights, strict=False)
    own_written = ("patch_embed.", "pos_embed.")                 # not yet built when the reference loads (MM:449-476)
    return _IncompatibleKeys([k for k in result.missing_keys if not k.startswith(own_written)], list(result.unexpected_keys))
