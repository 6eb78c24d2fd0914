"""ImageNet Vim initialisation of AuM (`--imagenet_pretrain`, aum.checkpoint.load_imagenet_checkpoint) against the reference's own
`AudioMamba(imagenet_pretrain=True)` on the synthetic Vim-S checkpoint of vim_ckpt.py (golden/imagenet_init.npz, written by
golden/make_golden_imagenet.py): the converted patch / position weights, the load report, the untouched head, the launcher's
command line of the published ImageNet-init recipes, and -- on the GPU -- the converted 24-block AuM-S through the HIP path and
the launcher end to end."""
import functools
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest
import torch

import make_golden_imagenet as MGI
import vim_ckpt
from conftest import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c[0]: c for c in MGI.CASES}

# exps/audioset/aum-small_imgnet-audioset.sh and exps/speechcommands/aum-small_imgnet-spc_v2.sh: the arguments their
# `accelerate launch --mixed_precision=fp16 ../../src/run.py` line passes, with the scripts' variables filled in
RECIPES = {
    "audioset": (
        "--model aum --dataset audioset --data-train ./data/datafiles/unbalanced.json --data-val ./data/datafiles/eval.json "
        "--exp-dir {exp} --label-csv ./data/class_labels_indices.csv --n_class 527 --lr 0.00001 --n-epochs 5 --batch-size 12 "
        "--save_model True --freqm 48 --timem 192 --mixup 0.5 --bal bal --tstride 16 --fstride 16 --imagenet_pretrain True "
        "--imagenet_pretrain_path {ckpt} --dataset_mean -4.2677393 --dataset_std 4.5689974 --audio_length 1024 --noise False "
        "--metrics mAP --loss BCE --warmup True --lrscheduler_start 2 --lrscheduler_step 1 --lrscheduler_decay 0.5 "
        "--exp-name aum-small_imgnet-audioset --model_type small --aum_type Bi-Bi"),
    "spc_v2": (
        "--model aum --dataset speechcommands --data-train ./data/datafiles/speechcommand_train_data.json "
        "--data-val ./data/datafiles/speechcommand_valid_data.json --data-eval ./data/datafiles/speechcommand_eval_data.json "
        "--exp-dir {exp} --label-csv ./data/speechcommands_class_labels_indices.csv --n_class 35 --lr 2.5e-4 --n-epochs 30 "
        "--batch-size 128 --save_model True --freqm 48 --timem 48 --mixup 0.6 --bal none --tstride 16 --fstride 16 "
        "--imagenet_pretrain True --imagenet_pretrain_path {ckpt} --metrics acc --loss BCE --warmup False --lrscheduler_start 5 "
        "--lrscheduler_step 1 --lrscheduler_decay 0.85 --dataset_mean -6.845978 --dataset_std 5.5654526 --audio_length 128 "
        "--noise True --exp-name aum-small_imgnet-spc_v2 --model_type small --aum_type Bi-Bi"),
}
RECIPE_SHAPES = {"audioset": ((128, 1024), 527), "spc_v2": ((128, 128), 35)}


@functools.lru_cache(maxsize=1)
def _vim():
    return vim_ckpt.vim_small_state()


def _ckpt():
    return _vim()[1]


@pytest.fixture(scope="module")
def ckpt_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vim") / "vim_s_synthetic.pth")
    torch.save(_ckpt(), path)
    return path


def _aum_small(case, seed=0, **kw):
    from aum.model import build_aum
    torch.manual_seed(seed)
    name, btype, spec, ncls = case[:4]
    return build_aum("small", bimamba_type=btype, spectrogram_size=spec, num_classes=ncls, **kw)


def _loaded(case, **kw):
    from aum.checkpoint import load_imagenet_checkpoint
    model = _aum_small(case)
    return model, load_imagenet_checkpoint(model, _ckpt(), **kw)


def _np(t):
    return t.detach().cpu().float().numpy()


# ---- command line -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_imagenet_recipe_command_line_parses_and_is_in_scope(recipe):
    from aum.train import build_parser, check_scope
    args = build_parser().parse_args(shlex.split(RECIPES[recipe].format(exp="/tmp/exp", ckpt="vim_s_midclstok_80p5acc.pth")))
    check_scope(args)
    assert args.imagenet_pretrain is True and args.imagenet_pretrain_path == "vim_s_midclstok_80p5acc.pth"
    assert args.imagenet_pretrain_modelkey == "model"                       # RUN:69-87 defaults
    assert args.imagenet_load_middle_cls_token is True and args.imagenet_load_double_cls_token is False
    assert args.aum_type == "Bi-Bi" and args.model_type == "small"


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_build_model_on_recipe_loads_imagenet_weights(recipe, ckpt_path):
    """build_model(args) of the parsed recipe (checkpoint path -> the synthetic file) == a seeded AuM-Small + load_imagenet_checkpoint"""
    from aum.checkpoint import load_imagenet_checkpoint
    from aum.train import build_model, build_parser, EXP_SEED
    args = build_parser().parse_args(shlex.split(RECIPES[recipe].format(exp="/tmp/exp", ckpt=ckpt_path)))
    torch.manual_seed(EXP_SEED)
    got = build_model(args).state_dict()
    spec, ncls = RECIPE_SHAPES[recipe]
    want = _aum_small(("x", "v2", spec, ncls), seed=EXP_SEED)
    load_imagenet_checkpoint(want, _ckpt())
    want = want.state_dict()
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, bad[:8]


def test_audio_mamba_imagenet_pretrain_keyword(ckpt_path):
    """AudioMamba(imagenet_pretrain=True, imagenet_pretrain_path=...) -- the reference's keywords -- loads after its own init"""
    from aum.model import AudioMamba
    case = CASES["b_bibi_l65"]
    torch.manual_seed(0)
    got = AudioMamba(spectrogram_size=case[2], embed_dim=384, num_classes=case[3], bimamba_type="v2", imagenet_pretrain=True,
                     imagenet_pretrain_path=ckpt_path, imagenet_pretrain_modelkey="model", imagenet_load_middle_cls_token=True,
                     imagenet_load_double_cls_token=False).state_dict()
    want = _loaded(case)[0].state_dict()
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, bad[:8]


# ---- the conversion against the reference --------------------------------------------------------------------------------------


def test_synthetic_checkpoint_is_the_fixtures():
    g = load_golden("imagenet_init")
    assert abs(vim_ckpt.checksum(_ckpt()) - float(g["ckpt_checksum"])) <= 1e-9 * abs(float(g["ckpt_checksum"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_converted_weights_match_reference(name):
    g = load_golden("imagenet_init")
    case = CASES[name]
    model, _ = _loaded(case)
    got = MGI.summarise(case, _np(model.patch_embed.proj.weight), _np(model.patch_embed.proj.bias), _np(model.pos_embed.pos_embed))
    assert sorted(got) == sorted(k for k in g if k.startswith(name + ".") and k.split(".", 1)[1] not in
                                 ("missing", "unexpected", "logits"))
    for k, v in got.items():
        assert v.shape == g[k].shape, k
        if v.dtype.kind in "iu":
            assert (v == g[k]).all(), k
        else:
            assert rel_err(v, g[k]) <= 1e-6, (k, rel_err(v, g[k]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_load_report_matches_reference(name):
    g = load_golden("imagenet_init")
    _, res = _loaded(CASES[name])
    assert list(res.missing_keys) == list(g[name + ".missing"])
    assert list(res.unexpected_keys) == list(g[name + ".unexpected"])
    assert list(res.missing_keys) == ["head.weight", "head.bias"]
    if CASES[name][1] == "v1":            # a Bi-Bi checkpoint into Fo-Bi blocks: the backward-direction weights are left over
        assert {k.split(".", 3)[3] for k in res.unexpected_keys} == {
            "D_b", "conv1d_b.weight", "conv1d_b.bias", "x_proj_b.weight", "dt_proj_b.weight", "dt_proj_b.bias"}
    else:
        assert not res.unexpected_keys


@pytest.mark.parametrize("name", ["a_bibi_l513", "c_fobi_l513"])
def test_backbone_equals_checkpoint_and_head_is_fresh(name):
    case = CASES[name]
    model, _ = _loaded(case)
    vim = _ckpt()["model"]
    sd = model.state_dict()
    keys = [k for k in sd if k == "cls_token" or k.startswith(("layers.", "norm_f."))]
    assert len(keys) == len(sd) - 5                                     # all but patch_embed.proj.*, pos_embed, head.*
    bad = [k for k in keys if not torch.equal(sd[k], vim[k])]
    assert not bad, bad[:8]
    if case[1] == "v1":
        assert torch.equal(sd["layers.7.mixer.A_b_log"], vim["layers.7.mixer.A_b_log"])
    fresh = _aum_small(case).state_dict()                               # same seed, no checkpoint
    assert torch.equal(sd["head.weight"], fresh["head.weight"]) and torch.equal(sd["head.bias"], fresh["head.bias"])
    assert not torch.equal(sd["cls_token"], fresh["cls_token"])


@pytest.mark.parametrize("middle", [True, False])
def test_cls_row_source(middle):
    """At Vim's own 14 x 14 grid nothing is resampled: the model's position rows are the checkpoint's, the cls row taken from the
    middle (row 98) or -- with --imagenet_load_middle_cls_token False -- from row 0"""
    case = ("vim_grid", "v2", (224, 224), 10)
    model, _ = _loaded(case, load_middle_cls_token=middle)
    pe = _ckpt()["model"]["pos_embed"]
    got = model.pos_embed.pos_embed.detach()
    if middle:
        assert torch.equal(got[:, 0], pe[:, vim_ckpt.MID])
        assert torch.equal(got[:, 1:], torch.cat([pe[:, :vim_ckpt.MID], pe[:, vim_ckpt.MID + 1:]], dim=1))
        assert torch.equal(got, _vim()[0]["pos_embed.pos_embed"])      # the row order the checkpoint was made from
    else:
        assert torch.equal(got, pe)
    w = _ckpt()["model"]["patch_embed.proj.weight"]
    assert torch.equal(model.patch_embed.proj.weight.detach(), w.mean(1, keepdim=True))


def test_resampled_grid_keeps_cls_row():
    model, _ = _loaded(CASES["a_bibi_l513"])
    pe = _ckpt()["model"]["pos_embed"]
    assert model.pos_embed.pos_embed.shape == (1, 513, 384)
    assert torch.equal(model.pos_embed.pos_embed.detach()[:, 0], pe[:, vim_ckpt.MID])


# ---- refusals ------------------------------------------------------------------------------------------------------------------


def _vim_with(**changes):
    sd = dict(_ckpt()["model"])
    sd.update(changes)
    return {"model": sd}


def test_refusals():
    from aum.checkpoint import load_imagenet_checkpoint
    from aum.model import AudioMamba, build_aum
    case = CASES["b_bibi_l65"]
    model = _aum_small(case)
    with pytest.raises(KeyError, match="state_dict.*found.*'epoch', 'model'"):
        load_imagenet_checkpoint(model, _ckpt(), modelkey="state_dict")
    pe = _ckpt()["model"]["pos_embed"]
    with pytest.raises(ValueError, match="square"):
        load_imagenet_checkpoint(model, _vim_with(pos_embed=pe[:, :1 + 14 * 13]))
    w = _ckpt()["model"]["patch_embed.proj.weight"]
    with pytest.raises(NotImplementedError, match="patch size"):
        load_imagenet_checkpoint(model, _vim_with(**{"patch_embed.proj.weight": w[:, :, :8, :8]}))
    with pytest.raises(ValueError, match="does not fit.*patch_embed.proj.weight"):          # Vim-S into AuM-Tiny
        load_imagenet_checkpoint(build_aum("tiny", spectrogram_size=case[2]), _ckpt())
    xw = _ckpt()["model"]["layers.3.mixer.x_proj.weight"]
    with pytest.raises(ValueError, match="does not fit.*layers.3.mixer.x_proj.weight"):
        load_imagenet_checkpoint(model, _vim_with(**{"layers.3.mixer.x_proj.weight": xw[:40]}))
    with pytest.raises(NotImplementedError, match="double-cls"):
        load_imagenet_checkpoint(model, _ckpt(), load_double_cls_token=True)
    with pytest.raises(NotImplementedError, match="imagenet_load_double_cls_token"):
        AudioMamba(spectrogram_size=case[2], embed_dim=384, imagenet_pretrain=True, imagenet_load_double_cls_token=True)
    with pytest.raises(ValueError, match="imagenet_pretrain_path"):
        AudioMamba(spectrogram_size=case[2], embed_dim=384, imagenet_pretrain=True)
    # nothing was written by a refused load
    fresh = _aum_small(case).state_dict()
    assert all(torch.equal(v, fresh[k]) for k, v in model.state_dict().items())
    from aum.train import build_parser, check_scope
    base = shlex.split(RECIPES["spc_v2"].format(exp="/tmp/exp", ckpt="vim.pth"))
    with pytest.raises(NotImplementedError, match="double-cls"):
        check_scope(build_parser().parse_args(base + ["--imagenet_load_double_cls_token", "True"]))
    no_path = [a for a in base if a not in ("--imagenet_pretrain_path", "vim.pth")]
    with pytest.raises(ValueError, match="imagenet_pretrain_path"):
        check_scope(build_parser().parse_args(no_path))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_bibi_l513", "b_bibi_l65"])
def test_imagenet_init_aum_small_on_gpu_vs_reference(name, ckpt_path):
    """The converted 24-block AuM-S Bi-Bi on the HIP path: fp32 logits at the fp32 model bar of test_gpu_model (1e-3), and under fp16
    autocast (the recipes' precision) finite and within the depth-scaled autocast model bar (1e-2 x sqrt(depth / 4))"""
    from aum.model import AudioMamba
    g = load_golden("imagenet_init")
    case = CASES[name]
    torch.manual_seed(0)
    model = AudioMamba(spectrogram_size=case[2], depth=MGI.DEPTH, embed_dim=MGI.DIM, num_classes=case[3], bimamba_type=case[1],
                       imagenet_pretrain=True, imagenet_pretrain_path=ckpt_path)
    head = MGI.head_state(case)
    with torch.no_grad():
        model.head.weight.copy_(torch.tensor(head["head.weight"]))
        model.head.bias.copy_(torch.tensor(head["head.bias"]))
    model = model.to("cuda")
    x = torch.tensor(MGI.inputs(case), device="cuda")
    ref = g[name + ".logits"]
    with torch.no_grad():
        l32 = model(x)
        with torch.autocast("cuda", dtype=torch.float16):
            l16 = model(x)
    assert l16.dtype == torch.float16
    e32 = rel_err(_np(l32), ref)
    assert e32 < 1e-3, e32
    assert torch.isfinite(l16).all()
    e16 = rel_err(_np(l16), ref)
    assert e16 < 1e-2 * (MGI.DEPTH / 4) ** 0.5, e16


@pytest.mark.gpu
def test_launcher_imagenet_recipe_end_to_end_on_gpu(tmp_path, ckpt_path):
    """python -m aum.train with the ImageNet recipe's flags (AuM-S Bi-Bi, 24 blocks, fp16, B = 12, 1024 frames) on toy data"""
    from aum.model import build_aum
    data = str(tmp_path / "toy")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_audioset.py"), data, "--clips", "36",
                    "--val-clips", "8", "--seconds", "2.0", "--classes", "6"], check=True, timeout=300)
    exp = str(tmp_path / "exp")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "audio-mamba-aum_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "aum.train", "--model_type", "small", "--aum_type", "Bi-Bi", "--imagenet_pretrain", "True",
           "--imagenet_pretrain_path", ckpt_path, "--mixed_precision", "fp16", "-b", "12", "--n_class", "6",
           "--label-csv", data + "/class_labels_indices.csv", "--data-train", data + "/train.json", "--data-val", data + "/val.json",
           "--num-workers", "2", "--lr", "1e-5", "--n-epochs", "1", "--max-steps", "3", "--exp-dir", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "_IncompatibleKeys(missing_keys=['head.weight', 'head.bias'], unexpected_keys=[])" in r.stdout, r.stdout[-2000:]
    res = np.loadtxt(exp + "/result.csv", delimiter=",", ndmin=2)
    assert res.shape == (1, 8) and np.isfinite(res).all(), res
    sd = torch.load(exp + "/models/latest_audio_model.1.pth", map_location="cpu")
    want = build_aum("small", bimamba_type="v2", num_classes=6).state_dict()
    assert sorted(k.replace("module.", "") for k in sd) == sorted(want)
    assert all(torch.isfinite(v).all() for v in sd.values())
