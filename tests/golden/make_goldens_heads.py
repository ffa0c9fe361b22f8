"""Generate the 4-head and 16-head golden fixtures (head_dim 128 / 32) by running the REFERENCE
modules, in the way of make_goldens.py (whose helpers this script imports; see its docstring for
how the reference's network/ modules are loaded by path and for the weight / input recipes).
``mhada_hip.recipe`` is shape-driven, so the per-head [D][D] convolutions get their own
deterministic weights under the same tags.

Usage:  python tests/golden/make_goldens_heads.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import load_reference_network, np32  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402


def full_case_heads(ref, name, c_shape, s_shape, seeds, heads, activation="softmax"):
    """full_case with ``num_heads`` passed to both ViTs and the AdaFormer, store_feats=False."""
    vit_c = load_recipe(ref["vit"].VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").eval()
    vit_s = load_recipe(ref["vit"].VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").eval()
    ada = load_recipe(ref["adaDecoder"].AdaAttnTransformerMultiHead(num_heads=heads, activation=activation),
                      "ada").eval()
    c = seeded_image(c_shape[0], c_shape[1], c_shape[2], seeds[0])
    s = seeded_image(s_shape[0], s_shape[1], s_shape[2], seeds[1])
    with torch.no_grad():
        fcs, cs = ada(vit_c(c), vit_s(s))
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, content_shape=np.array(c_shape), style_shape=np.array(s_shape), seeds=np.array(seeds),
                        activation=np.array(activation), heads=np.array(heads), cs=np32(cs), content=np32(c),
                        style=np32(s), fcs=np32(fcs))
    print(f"wrote {path}  cs range [{cs.min():.3f}, {cs.max():.3f}] mean {cs.mean():.3f}")


def block_case_heads(ref, name, bsz, hc, wc, hs, ws, seed, heads, activation="softmax"):
    """block_case (same inputs for the same seed) on AdaAttnMultiHead(512, heads)."""
    blk = ref["adaDecoder"].AdaAttnMultiHead(512, heads, activation)
    load_recipe(blk, "blk")
    g = torch.Generator().manual_seed(seed)
    fc = torch.randn(bsz, 512, hc, wc, generator=g) * 2.0 + 0.5
    fs = torch.randn(bsz, 512, hs, ws, generator=g) * 1.5 - 0.25
    fcs = torch.randn(bsz, 512, hc, wc, generator=g)
    with torch.no_grad():
        out = blk(fc, fs, fcs)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), fc=np32(fc), fs=np32(fs), fcs=np32(fcs), out=np32(out),
                        activation=np.array(activation), heads=np.array(heads))
    print(f"wrote {name}.npz  out range [{out.min():.3f}, {out.max():.3f}]")


def main():
    torch.set_num_threads(8)
    ref = load_reference_network()
    block_case_heads(ref, "block_h4_b2_4x4_s3x5", 2, 4, 4, 3, 5, 11, 4)
    block_case_heads(ref, "block_h16_b2_4x4_s3x5", 2, 4, 4, 3, 5, 11, 16)
    block_case_heads(ref, "block_cos_h16_b1_4x4", 1, 4, 4, 4, 4, 12, 16, activation="cosine")
    full_case_heads(ref, "full_64_b2_h4", (2, 64, 64), (2, 64, 64), (3, 4), 4)
    full_case_heads(ref, "full_64_b2_h16", (2, 64, 64), (2, 64, 64), (3, 4), 16)
    # Nq != Nk (content 2:1, square style)
    full_case_heads(ref, "full_64x128_s64_b1_h16", (1, 64, 128), (1, 64, 64), (7, 8), 16)


if __name__ == "__main__":
    main()
