"""Generate the single-head golden fixtures (AdaAttN(512) / AdaAttnTransformer, head width 512) by running
the REFERENCE modules, in the way of make_goldens.py and make_goldens_heads.py (whose helpers this script
imports; see make_goldens.py's docstring for how the reference's network/ modules are loaded by path and
for the weight / input recipes).  ``mhada_hip.recipe`` is shape-driven, so the 512 x 512 convolutions f, g, h
get their own deterministic weights under the same tags.  Only data is stored: key / shape lists, constructor
signatures as text, seeded inputs and the reference's outputs.

Usage:  python tests/golden/make_goldens_single.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import load_reference_network, np32  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402


def state_dict_keys_single(ref):
    """Reference state_dict key -> shape and the constructor signatures, for the drop-in's parity tests."""
    ada = ref["adaDecoder"]
    mods = {"ada1": ada.AdaAttnTransformer(), "block1_512": ada.AdaAttN(512)}
    out = {k: {n: list(t.shape) for n, t in m.state_dict().items()} for k, m in mods.items()}
    out["signatures"] = {"AdaAttnTransformer": str(inspect.signature(ada.AdaAttnTransformer.__init__)),
                         "AdaAttN": str(inspect.signature(ada.AdaAttN.__init__))}
    with open(os.path.join(HERE, "state_dict_keys_single.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote state_dict_keys_single.json")


def block_case_single(ref, name, bsz, hc, wc, hs, ws, seed, activation="softmax"):
    """block_case_heads (same inputs for the same seed) on AdaAttN(512)."""
    blk = ref["adaDecoder"].AdaAttN(512, activation)
    load_recipe(blk, "blk")
    g = torch.Generator().manual_seed(seed)
    fc = torch.randn(bsz, 512, hc, wc, generator=g) * 2.0 + 0.5
    fs = torch.randn(bsz, 512, hs, ws, generator=g) * 1.5 - 0.25
    fcs = torch.randn(bsz, 512, hc, wc, generator=g)
    with torch.no_grad():
        out = blk(fc, fs, fcs)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), fc=np32(fc), fs=np32(fs), fcs=np32(fcs), out=np32(out),
                        activation=np.array(activation))
    print(f"wrote {name}.npz  out range [{out.min():.3f}, {out.max():.3f}]")


def full_case_single(ref, name, c_shape, s_shape, seeds, activation="softmax"):
    """AdaAttnTransformer on the 8-head recipe ViTs; stores cs and the inputs."""
    vit_c = load_recipe(ref["vit"].VisionTransformer(pos_embedding=True), "vit_c").eval()
    vit_s = load_recipe(ref["vit"].VisionTransformer(pos_embedding=False), "vit_s").eval()
    ada = load_recipe(ref["adaDecoder"].AdaAttnTransformer(activation=activation), "ada").eval()
    c = seeded_image(c_shape[0], c_shape[1], c_shape[2], seeds[0])
    s = seeded_image(s_shape[0], s_shape[1], s_shape[2], seeds[1])
    with torch.no_grad():
        cs = ada(vit_c(c), vit_s(s))
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, content_shape=np.array(c_shape), style_shape=np.array(s_shape), seeds=np.array(seeds),
                        activation=np.array(activation), cs=np32(cs), content=np32(c), style=np32(s))
    print(f"wrote {path}  cs range [{cs.min():.3f}, {cs.max():.3f}] mean {cs.mean():.3f}")


def main():
    torch.set_num_threads(8)
    ref = load_reference_network()
    state_dict_keys_single(ref)
    block_case_single(ref, "block1_b2_4x4_s3x5", 2, 4, 4, 3, 5, 11)
    block_case_single(ref, "block1_cos_b1_4x4", 1, 4, 4, 4, 4, 12, activation="cosine")
    full_case_single(ref, "full1_64_b2", (2, 64, 64), (2, 64, 64), (3, 4))
    # Nq != Nk (content 2:1, square style)
    full_case_single(ref, "full1_64x128_s64_b1", (1, 64, 128), (1, 64, 64), (7, 8))


if __name__ == "__main__":
    main()
