"""Training goldens for 4- and 16-head models (head_dim 128 / 32), produced by the reference.

The train_image.py:103-139 sequence of make_train_goldens.py (whose reference loader and helpers this
script imports; see its docstring for the stand-ins the reference's imports need) at 64 x 64, B = 2,
with ``num_heads`` = 4 and 16 passed to both ViTs and the AdaFormer, as make_goldens_heads.py builds
its models.  ``mhada_hip.recipe`` is shape-driven, so the per-head [D][D] convolutions get their
own deterministic weights under the same tags.  Only the five losses, cs and the per-parameter
gradient norms are stored.

Usage:  python tests/golden/make_train_goldens_heads.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_train_goldens import grad_summary, load_reference, np32  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402

SEEDS = (101, 102)  # content, style: the seeds of train_64_b2


def train_case(ref, heads):
    R, L = ref, ref["lossfn"]
    vit_c = load_recipe(R["vit"].VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").train()
    vit_s = load_recipe(R["vit"].VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").train()
    ada = load_recipe(R["adaDecoder"].AdaAttnTransformerMultiHead(num_heads=heads), "ada").train()
    vgg = R["vgg19"].VGG19()
    load_recipe(vgg, "vgg")
    vgg.eval()
    noLearn = nn.ModuleList([R["adaDecoder"].AdaAttnForLoss(256, 64 + 128 + 256),
                             R["adaDecoder"].AdaAttnForLoss(512, 64 + 128 + 256 + 512),
                             R["adaDecoder"].AdaAttnForLoss(512, 64 + 128 + 256 + 512 + 512)]).eval()
    mse = nn.MSELoss(reduction="mean")
    content = seeded_image(2, 64, 64, SEEDS[0])
    style = seeded_image(2, 64, 64, SEEDS[1])

    # train_image.py:103-139
    fc_vc = vit_c(content)
    fs_vs = vit_s(style)
    _, cs = ada(fc_vc, fs_vs)
    fc_vs = vit_s(content)
    fs_vc = vit_c(style)
    _, cc = ada(fc_vc, fc_vs)
    _, ss = ada(fs_vc, fs_vs)
    vgg_fs = vgg(style)
    vgg_fc = vgg(content)
    vgg_fcs = vgg(cs)
    vgg_fcc = vgg(cc)
    vgg_fss = vgg(ss)
    loss_gs = L.global_style_loss(vgg_fcs, vgg_fs, mse) * 70
    loss_lf = L.local_feature_loss(vgg_fc, vgg_fs, vgg_fcs, noLearn, mse) * 15
    loss_id1 = L.identity_loss_1(cc, content, ss, style, mse) * 5e-2
    loss_id2 = L.identity_loss_2(vgg_fcc, vgg_fc, vgg_fss, vgg_fs, mse) * 1e-1
    loss = loss_gs + loss_lf + loss_id1 + loss_id2
    loss.backward()

    out = {
        "heads": np.array(heads), "content_seed": np.array(SEEDS[0]), "style_seed": np.array(SEEDS[1]),
        "losses": np.array([float(loss_gs), float(loss_lf), float(loss_id1), float(loss_id2), float(loss)]),
        "cs": np32(cs),
        "grad_vit_c": grad_summary(vit_c), "grad_vit_s": grad_summary(vit_s), "grad_ada": grad_summary(ada),
    }
    path = os.path.join(HERE, f"train_64_b2_h{heads}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: losses {out['losses']}")


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    for heads in (4, 16):
        train_case(ref, heads)


if __name__ == "__main__":
    main()
