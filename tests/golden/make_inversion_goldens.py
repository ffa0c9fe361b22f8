"""Feature-inversion goldens, produced by the reference's own modules.

The first iteration of the reference's two inversion scripts at 64 x 64, B = 1, on the recipe weights
(frozen, eval): the loss and its gradient with respect to the optimised image, for
  (a) visual_vit.py:88-112   — sum over the three layers of mse(vit_c(recon)[l], vit_c(content)[l]);
  (b) visual_mhada.py:111-127 — mse(fcs(recon), fcs(content)) with fcs the output of the six MHAda
      blocks on the content ViT's features and the style ViT's features of a no-grad call.
content / style = seeded_image(1, 64, 64, 101 / 102); recon = torch.randn from generator seed 7.
Case (b) is evaluated on the image stacked twice along the batch axis (recon, fs and the target each
concatenated with themselves): aten's CPU instance_norm backward misreads a non-contiguous incoming
gradient when B = 1 (the permuted q and S * IN(fcs) paths of every block; finite differences disagree
with it at B = 1 and agree at B = 2), which would make the stored gradient wrong.  Two identical
samples leave every feature and the loss unchanged (the ViT's batch-axis softmax over two equal keys,
per-sample blocks, a mean over equal terms), and by symmetry the gradient reaching the single leaf
through both copies is exactly the B = 1 gradient.
The reference modules are loaded by path through make_train_goldens.load_reference (see its
docstring for the stand-ins the reference's imports need); this script holds none of their text.

Usage:  python tests/golden/make_inversion_goldens.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_train_goldens import load_reference, np32  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402

SEEDS = (101, 102, 7)  # content, style, initial image


def blocks(ada, fc, fs):
    """The six MHAda blocks in the order of the reference's forward, without the decoder."""
    fcs = fc[0]
    for i, blk in enumerate(ada.adaAttnHead):
        fcs = blk(fc[i // 2] if i % 2 == 0 else fcs, fs[i // 2], fcs)
    return fcs


def main():
    torch.set_num_threads(8)
    R = load_reference()
    vit_c = load_recipe(R["vit"].VisionTransformer(pos_embedding=True), "vit_c").eval().requires_grad_(False)
    vit_s = load_recipe(R["vit"].VisionTransformer(pos_embedding=False), "vit_s").eval().requires_grad_(False)
    ada = load_recipe(R["adaDecoder"].AdaAttnTransformerMultiHead(), "ada").eval().requires_grad_(False)
    content = seeded_image(1, 64, 64, SEEDS[0])
    style = seeded_image(1, 64, 64, SEEDS[1])
    init = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(SEEDS[2]))
    with torch.no_grad():
        target_vit = vit_c(content)
        fs = vit_s(style)
        target_ada = blocks(ada, target_vit, fs)

    recon = init.clone().requires_grad_(True)
    loss_vit = sum(F.mse_loss(f, t) for f, t in zip(vit_c(recon), target_vit))
    (grad_vit,) = torch.autograd.grad(loss_vit, recon)

    twice = lambda t: torch.cat([t, t])  # noqa: E731  (see the docstring: B = 1 through B = 2)
    recon = init.clone().requires_grad_(True)
    loss_ada = F.mse_loss(blocks(ada, vit_c(twice(recon)), [twice(f) for f in fs]), twice(target_ada))
    (grad_ada,) = torch.autograd.grad(loss_ada, recon)

    out = {"seeds": np.array(SEEDS), "losses": np.array([loss_vit.item(), loss_ada.item()], dtype=np.float64),
           "grad_vit": np32(grad_vit), "grad_ada": np32(grad_ada)}
    path = os.path.join(HERE, "inversion_64.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: losses {out['losses']}, |grad| {float(grad_vit.norm()):.6g} {float(grad_ada.norm()):.6g}")


if __name__ == "__main__":
    main()
