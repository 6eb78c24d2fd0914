"""A synthetic ImageNet Vim-S checkpoint (the layout of vim_s_midclstok_80p5acc.pth), rebuilt from a seed wherever it is needed
and never stored: the package's own seeded AuM-Small Bi-Bi at 224 x 224 with 1000 classes -- realistic weight statistics, so 24
blocks of outputs stay finite -- relabelled into Vim's layout:

  * the position embedding is `pos_embed`, its cls row at the middle of the sequence (row 98 of 197);
  * the patch projection has 3 input channels: the 1-channel weight times a seeded factor per channel, so the channel mean that
    ImageNet init takes is not the weight itself; its bias (zero at init) gets seeded values;
  * the state dict sits under "model", next to an "epoch" entry.

`python vim_ckpt.py OUT.pth` writes it (the fixture generator runs the reference's model on the file)."""
import os
import sys

import numpy as np
import torch

SEED = 20240
ROWS = 197                          # 14 x 14 patches of 224 x 224 + the cls row
MID = (ROWS - 1) // 2               # 98: the cls row of a middle-cls Vim


def channel_factors(seed=SEED):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 1.5, 3).astype(np.float32))


def patch_bias(dim, seed=SEED):
    return torch.from_numpy(np.random.default_rng(seed + 1).normal(0, 0.02, dim).astype(np.float32))


def vim_small_state(seed=SEED):
    """(the AuM-Small Bi-Bi state it was made from, the checkpoint dict {"model": vim state dict, "epoch": 0})"""
    from aum.model import build_aum
    rng_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        src = build_aum("small", bimamba_type="v2", spectrogram_size=(224, 224), num_classes=1000)
    finally:
        torch.random.set_rng_state(rng_state)
    src_sd = {k: v.detach().clone() for k, v in src.state_dict().items()}
    sd = dict(src_sd)
    pe = sd.pop("pos_embed.pos_embed")
    assert pe.shape[1] == ROWS
    sd["pos_embed"] = torch.cat([pe[:, 1:MID + 1], pe[:, :1], pe[:, MID + 1:]], dim=1).contiguous()
    w = sd["patch_embed.proj.weight"]
    sd["patch_embed.proj.weight"] = (w * channel_factors(seed).view(1, 3, 1, 1)).contiguous()
    sd["patch_embed.proj.bias"] = patch_bias(w.shape[0], seed)
    return src_sd, {"model": sd, "epoch": 0}


def vim_small_checkpoint(seed=SEED):
    return vim_small_state(seed)[1]


def checksum(ckpt):
    """fp64 sum over a few tensors of the checkpoint: tells a drifted generator from a wrong conversion"""
    sd = ckpt["model"]
    return float(sum(sd[k].double().sum().item() * (i + 1) for i, k in
                     enumerate(("pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "layers.0.mixer.in_proj.weight",
                                "layers.23.mixer.x_proj_b.weight", "norm_f.weight"))))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "audio-mamba-aum_amd"))
    torch.save(vim_small_checkpoint(), sys.argv[1])
