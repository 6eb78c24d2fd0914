"""Double-cls, cls-free (mean / none / max) and randomly placed cls models; shared by tests/test_cls_layouts.py (CPU, lane-array library)
and tests/test_gpu_cls_layouts.py (device library).

`reference_forward` restates, in plain torch on the model's own parameters, what the reference's AudioMamba does around the layer stack:
the token layout and position rows of mamba_models.py:518-562 (with FlexiPosEmbed's insert_to_prefix / insert_from_prefix written out
below) and the tail of forward_features / forward, mamba_models.py:659-685 -- the final add + norm on ALL rows, then the cls rows, the
last row, the mean over the tokens, or the max over the tokens' logits.  The layer stack in between is the model's own."""
import random

import numpy as np
import pytest
import torch

from conftest import rel_err

KW = dict(spectrogram_size=(32, 64), depth=2, embed_dim=192, num_classes=7, bimamba_type="v1")
BATCH = 3
VARIANTS = {
    "double": dict(use_double_cls_token=True, use_middle_cls_token=False),
    "mean": dict(if_cls_token=False, final_pool_type="mean"),
    "none": dict(if_cls_token=False, final_pool_type="none"),
    "max": dict(if_cls_token=False, final_pool_type="max"),
    "random": dict(),
}


def insert_to_prefix(x, poses):
    for i, p in enumerate(poses):
        x = torch.cat([x[:, :i], x[:, p:p + 1], x[:, i:p], x[:, p + 1:]], dim=1)
    return x


def insert_from_prefix(x, poses):
    pre, x = x[:, :len(poses)], x[:, len(poses):]
    for i, p in enumerate(poses):
        x = torch.cat([x[:, :p], pre[:, i:i + 1], x[:, p:]], dim=1)
    return x


def reference_tokens(model, x, cls_pos=None):
    """mamba_models.py:510-562 -> (sequence, token_position)"""
    t = model.patch_embed(x.unsqueeze(1).transpose(2, 3))
    B, N, _ = t.shape
    if model.num_tokens == 2:
        tp = [0, N + 1]
        t = torch.cat((model.cls_token_head.expand(B, -1, -1), t, model.cls_token_tail.expand(B, -1, -1)), dim=1)
    elif model.num_tokens == 1:
        tp = cls_pos if cls_pos is not None else (N // 2 if model.use_middle_cls_token else (N if model.use_end_cls_token else 0))
        t = torch.cat((t[:, :tp], model.cls_token.expand(B, -1, -1), t[:, tp:]), dim=1)
    else:
        tp = None
    poses = tp if isinstance(tp, list) else ([tp] if tp is not None else [])
    t = insert_from_prefix(insert_to_prefix(t, poses) + model.pos_embed.pos_embed, poses)
    if model.transpose_token_sequence:
        if model.num_tokens == 2:
            head, tail, t = t[:, :1], t[:, -1:], t[:, 1:-1]
        elif model.num_tokens == 1:
            c, t = t[:, tp:tp + 1], torch.cat((t[:, :tp], t[:, tp + 1:]), dim=1)
        nf, nt = model.patch_grid_size
        t = t.reshape(B, nf, nt, -1).transpose(1, 2).reshape(B, nt * nf, -1)
        if model.num_tokens == 2:
            t = torch.cat((head, t, tail), dim=1)
        elif model.num_tokens == 1:
            t = torch.cat((t[:, :tp], c, t[:, tp:]), dim=1)
    return t, tp


def reference_forward(model, x, cls_pos=None):
    from mamba_ssm.ops.triton.layernorm import rms_norm_ref
    seq, tp = reference_tokens(model, x, cls_pos)
    hidden, residual = model._run_layers(seq)
    h = rms_norm_ref(hidden, model.norm_f.weight, None, residual=residual, eps=model.norm_f.eps, upcast=True)    # :648-657, every row
    if model.num_tokens == 2:
        f = (h[:, tp[0]] + h[:, tp[1]]) / 2                                                                      # :662
    elif model.num_tokens == 1:
        f = h[:, tp]
    elif model.final_pool_type == "none":
        f = h[:, -1]
    elif model.final_pool_type == "mean":
        f = h.mean(dim=1)
    else:
        f = h
    out = model.head(f)
    return out.max(dim=1)[0] if model.final_pool_type == "max" and model.num_tokens == 0 else out               # :683-684


def build(variant, transpose, dev):
    import aum.model as M
    torch.manual_seed(21)
    model = M.AudioMamba(transpose_token_sequence=transpose, **dict(KW, **VARIANTS[variant])).to(dev).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("norm.weight") or n.endswith("norm_f.weight"):
                p.add_(0.2 * torch.randn_like(p))
    return model


def check_model(dev, variant, transpose, autocast=False):
    model = build(variant, transpose, dev)
    N = model.num_patches
    assert model.num_tokens == {"double": 2, "random": 1}.get(variant, 0) and model.pos_embed.pos_embed.shape[1] == N + model.num_tokens
    assert ("cls_token" in dict(model.named_parameters())) == (variant == "random")
    assert ("cls_token_head" in dict(model.named_parameters())) == (variant == "double")
    x = torch.randn(BATCH, 64, 32, device=dev)
    dl = torch.randn(BATCH, 7, device=dev)
    rnd = variant == "random"
    if rnd:
        random.seed(5)
        cls_pos = random.randint(0, N)

    def go(ref):
        model.zero_grad()
        random.seed(5)
        with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16, enabled=autocast):
            logits = reference_forward(model, x, cls_pos if rnd else None) if ref else model(x, if_random_cls_token_position=rnd)
        (logits.float() * dl).sum().backward()
        return logits.detach().float(), {k: p.grad.clone() for k, p in model.named_parameters()}

    got, ref = go(False), go(True)
    assert got[0].shape == (BATCH, 7)
    tol = 1e-2 if autocast else 1e-4
    e = rel_err(got[0].cpu().numpy(), ref[0].cpu().numpy())
    print(f"{variant} transpose={transpose} autocast={autocast} logits: {e:.3e}")
    assert e < tol, e
    for k in got[1]:
        e = rel_err(got[1][k].float().cpu().numpy(), ref[1][k].float().cpu().numpy())
        print(f"  grad {k}: {e:.3e}")
        assert e < tol, (k, e)


def check_layout_rules():
    import aum.model as M
    with pytest.raises(ValueError, match="use_middle_cls_token"):
        M.AudioMamba(**dict(KW, use_double_cls_token=True))                     # the middle flag is on by default
    with pytest.raises(NotImplementedError):
        M.AudioMamba(**dict(KW, if_cls_token=False, final_pool_type="all"))
    double = M.AudioMamba(**dict(KW, **VARIANTS["double"]))
    assert {"cls_token_head", "cls_token_tail"} <= double.no_weight_decay()
    free = M.AudioMamba(**dict(KW, **VARIANTS["mean"]))
    x = torch.randn(2, 64, 32)
    for m in (double, free):
        with pytest.raises(ValueError, match="if_random_cls_token_position"):
            m(x, if_random_cls_token_position=True)
        with pytest.raises(ValueError, match="single end cls token"):
            m._check_streamable()


def check_mean_head_is_fused(dev, monkeypatch):
    """under bf16 autocast the cls-free 'mean' head is one rmsnorm_pool_fwd / _bwd pair and no other norm launch on the final rows"""
    import aum_hip
    model = build("mean", False, dev)
    n = {"fwd": 0, "bwd": 0}
    for k in n:
        real = getattr(aum_hip, "rmsnorm_pool_" + k)
        monkeypatch.setattr(aum_hip, "rmsnorm_pool_" + k, lambda *a, _k=k, _r=real, **kw: (n.__setitem__(_k, n[_k] + 1), _r(*a, **kw))[1])
    x = torch.randn(BATCH, 64, 32, device=dev)
    with torch.autocast(torch.device(dev).type, dtype=torch.bfloat16):
        y = model(x)
    y.float().sum().backward()
    assert n == {"fwd": 1, "bwd": 1}, n


def check_double_cls_checkpoint():
    """a synthetic double-cls Vim state dict on a 3 x 3 grid: position row 0 -> the head's row, row 10 -> the tail's, rows 1..9 -> the patches"""
    import aum.model as M
    from aum.checkpoint import load_imagenet_checkpoint
    kw = dict(spectrogram_size=(48, 48), depth=2, embed_dim=192, num_classes=7, bimamba_type="v1")
    model = M.AudioMamba(**dict(kw, **VARIANTS["double"]))
    sd = {k: v.clone() for k, v in model.state_dict().items() if not k.startswith(("pos_embed.", "head."))}
    sd["pos_embed"] = torch.arange(11, dtype=torch.float32).reshape(1, 11, 1).repeat(1, 1, 192)      # distinct rows 0 .. 10
    sd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].repeat(1, 3, 1, 1)
    sd["cls_token_head"] = torch.full((1, 1, 192), 5.0)
    sd["cls_token_tail"] = torch.full((1, 1, 192), -5.0)
    load_imagenet_checkpoint(model, {"model": sd}, "model", True, True)
    pe = model.pos_embed.pos_embed.detach()[0, :, 0]
    assert pe.tolist() == [0.0, 10.0] + [float(i) for i in range(1, 10)], pe.tolist()            # same 3 x 3 grid: no resampling
    assert float(model.cls_token_head[0, 0, 0]) == 5.0 and float(model.cls_token_tail[0, 0, 0]) == -5.0
    single = M.AudioMamba(**kw)
    with pytest.raises(NotImplementedError, match="use_double_cls_token"):
        load_imagenet_checkpoint(single, {"model": dict(sd)}, "model", True, True)               # double checkpoint, single model
    with pytest.raises(ValueError):
        load_imagenet_checkpoint(single, {"model": dict(sd)}, "model", True, False)
    ssd = {k: v.clone() for k, v in single.state_dict().items() if not k.startswith(("pos_embed.", "head."))}
    ssd["pos_embed"] = sd["pos_embed"][:, :10]
    ssd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"]
    with pytest.raises(ValueError):
        load_imagenet_checkpoint(model, {"model": ssd}, "model", True, True)                     # single checkpoint, double model


def check_scope():
    from aum import train as T
    parse = T.build_parser().parse_args
    T.check_scope(parse(["--use_double_cls_token", "True", "--use_middle_cls_token", "False"]))
    for pool in ("mean", "none", "max"):
        T.check_scope(parse(["--if_cls_token", "False", "--final_pool_type", pool]))
    T.check_scope(parse(["--if_random_cls_token_position", "True"]))
    with pytest.raises(NotImplementedError):
        T.check_scope(parse(["--if_random_token_rank", "True"]))
    with pytest.raises(ValueError):
        T.check_scope(parse(["--if_random_cls_token_position", "True", "--if_cls_token", "False"]))
    args = parse(["--if_cls_token", "False", "--final_pool_type", "max", "--depth", "2", "--model_type", "tiny", "--n_class", "4", "--audio_length", "64"])
    model = T.build_model(args)
    assert model.num_tokens == 0 and model.final_pool_type == "max"


def check_launcher_trains(tmp_path, flags):
    import os
    import subprocess
    import sys
    import aum.train as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = str(tmp_path / "toy")
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_toy_audioset.py"), data, "--clips", "8", "--val-clips", "2", "--seconds", "0.7",
                    "--classes", "4"], check=True)
    files = sorted(os.listdir(data))
    pick = lambda *keys: os.path.join(data, next(f for f in files if all(k in f for k in keys)))
    exp = str(tmp_path / "exp")
    T.main(["--model", "aum", "--model_type", "tiny", "--aum_type", "Fo-Bi", "--depth", "2", "--n_class", "4",
            "--label-csv", pick(".csv"), "--data-train", pick("train", ".json"), "--data-val", pick("val", ".json"), "--audio_length", "64",
            "--num-workers", "0", "-b", "4", "--exp-dir", exp, "--n-epochs", "1", "--max-steps", "2", "--n-print-steps", "1000", "--lr", "1e-3",
            "--lrscheduler_start", "10", "--save_model", "False"] + flags)
    result = np.loadtxt(os.path.join(exp, "result.csv"), delimiter=",", ndmin=2)
    assert result.shape == (1, 8) and np.isfinite(result[0, [5, 6]]).all(), result
