#!/usr/bin/env python3
"""Generate tests/golden/imagenet_init.npz: the REFERENCE's own ImageNet initialisation (`AudioMamba(imagenet_pretrain=True,
imagenet_pretrain_path=...)`, MM:348-395 + TOK:26-66) of AuM-Small on the synthetic Vim-S checkpoint of tests/vim_ckpt.py, run on
the CPU through make_golden's import recipe.  Runs only where the reference is present (no-op elsewhere).

Cases (name, bimamba_type, spectrogram size, classes, logits?):
  (a) Bi-Bi at 128 x 1024 (L = 513), (b) Bi-Bi at 128 x 128 with 35 classes (L = 65), (c) Fo-Bi at 128 x 1024.
Stored per case: the converted patch weight (in full for (b); a seeded sample of output channels plus fp64 sums of every
channel for (a) and (c)) and bias, the re-gridded position embedding (in full for (b); a seeded row sample plus fp64 row sums for
(a) and (c)), the missing / unexpected keys of the reference's load_state_dict, and for (a) and (b) the fp32 logits of a seeded
B = 2 spectrogram through the whole 24-block model.  ImageNet init drops Vim's head, so the head is fresh: both sides set it to
the seeded values of head_state() before the logits.  Inputs are regenerated from seeds; only outputs are stored."""
import contextlib
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)

DEPTH, DIM = 24, 384
CASES = [
    ("a_bibi_l513", "v2", (128, 1024), 527, True),
    ("b_bibi_l65", "v2", (128, 128), 35, True),
    ("c_fobi_l513", "v1", (128, 1024), 527, False),
]
FULL = ("b_bibi_l65",)                  # cases stored in full; the others as samples + sums
N_SAMPLE = 16


def _rng(tag):
    return np.random.default_rng(int.from_bytes(tag.encode(), "little") % (2 ** 32))


def head_state(case):
    name, ncls = case[0], case[3]
    r = _rng("imagenet_head_" + name)
    return {"head.weight": (r.normal(0, 1, (ncls, DIM)) / np.sqrt(DIM)).astype(np.float32),
            "head.bias": r.normal(0, 0.1, ncls).astype(np.float32)}


def inputs(case):
    name, spec = case[0], case[2]
    return (0.5 * _rng("imagenet_x_" + name).normal(0, 1, (2, spec[1], spec[0]))).astype(np.float32)


def sample_rows(case, n_rows):
    return np.sort(_rng("imagenet_rows_" + case[0]).choice(n_rows, N_SAMPLE, replace=False))


def summarise(case, patch_w, patch_b, pos_embed):
    """the stored form of a conversion result (numpy float32 arrays in, dict of fixture entries out)"""
    name = case[0]
    out = {name + ".patch_b": patch_b}
    if name in FULL:
        out[name + ".patch_w"] = patch_w
        out[name + ".pos_embed"] = pos_embed
        return out
    w = patch_w.reshape(patch_w.shape[0], -1)
    out[name + ".patch_w_rows"] = w[sample_rows(case, w.shape[0])]
    out[name + ".patch_w_sums"] = w.astype(np.float64).sum(1)
    pe = pos_embed.reshape(pos_embed.shape[1], -1)
    out[name + ".pos_embed_shape"] = np.array(pos_embed.shape)
    out[name + ".pos_embed_rows"] = pe[sample_rows(case, pe.shape[0])]
    out[name + ".pos_embed_sums"] = pe.astype(np.float64).sum(1)
    return out


def main():
    import torch
    import vim_ckpt
    from make_golden import import_reference, import_reference_model
    out = {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "vim_s_synthetic.pth")
        # the checkpoint is made by the package, in a process of its own: the reference's import recipe rebinds `mamba_ssm`
        subprocess.run([sys.executable, os.path.join(TESTS, "vim_ckpt.py"), path], check=True)
        out["ckpt_checksum"] = np.float64(vim_ckpt.checksum(torch.load(path, map_location="cpu")))
        torch_, ssi, ln, _ = import_reference()
        torch_.set_num_threads(8)
        mm = import_reference_model(torch_, ssi, ln)
        loads = []
        module_load = torch.nn.Module.load_state_dict

        def recording_load(self, *a, **k):          # the result the reference prints (MM:394)
            res = module_load(self, *a, **k)
            loads.append(res)
            return res
        mm.AudioMamba.load_state_dict = recording_load
        for case in CASES:
            name, btype, spec, ncls, with_logits = case
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                model = mm.AudioMamba(spectrogram_size=spec, depth=DEPTH, embed_dim=DIM, num_classes=ncls, bimamba_type=btype,
                                      imagenet_pretrain=True, imagenet_pretrain_path=path)
            res = loads.pop()
            assert not loads
            out[name + ".missing"] = np.array(res.missing_keys, dtype=str)
            out[name + ".unexpected"] = np.array(res.unexpected_keys, dtype=str)
            out.update(summarise(case, model.patch_embed.proj.weight.detach().numpy(), model.patch_embed.proj.bias.detach().numpy(),
                                 model.pos_embed.pos_embed.detach().numpy()))
            if with_logits:
                with torch.no_grad():
                    hs = head_state(case)
                    model.head.weight.copy_(torch.tensor(hs["head.weight"]))
                    model.head.bias.copy_(torch.tensor(hs["head.bias"]))
                    out[name + ".logits"] = model(torch.tensor(inputs(case))).float().numpy()
            print(name, "done", flush=True)
    np.savez_compressed(os.path.join(HERE, "imagenet_init.npz"), **out)
    print("imagenet_init.npz", len(out))


if __name__ == "__main__":
    from make_golden import REF
    if os.path.isdir(REF):
        main()
