"""LPIPS golden, produced by the reference's own lpips package.

Runs in the build container only.  lpips/pretrained_networks.py imports torchvision at module level,
which is not installed; this script puts a stand-in into sys.modules before importing the package:
  * torchvision.models.vgg16(weights=...) -> an object whose .features is the cfg-"D" layer stack
    (Conv3x3 pad 1 / ReLU(inplace) / MaxPool 2x2) that pretrained_networks.py:101-117 slices, built
    here and holding the test weights of tests/lpips_ref.py (the "vgg16" recipe with every conv weight
    times sqrt(6); the ImageNet weights are a remote download this environment cannot make);
  * tqdm (imported by lpips/trainer.py) gets an inert stand-in if it is missing.
Then the reference's own LPIPS(net="vgg", version="0.1").forward(im2tensor(a), im2tensor(b),
retPerLayer=True) runs in fp32 on the CPU, with the linear layers it loads from its own
weights/v0.1/vgg.pth; those five vectors are stored as data beside its results.  This script holds none
of the package's text.

Inputs, u8 RGB [2][48][48][3] (48: relu5_3 is 3 x 3, an odd pixel count, and no pool floors):
a = seeded noise (default_rng(5)), b = lpips_ref.golden_b()'s arithmetic pattern.
Stored: a, b, lin0 .. lin4, ref_layers [5][2], ref_total [2] (the reference's forward), fp64_layers
[5][2] (lpips_ref.lpips64 on fp64 aten features of lpips_ref.scaling64), ref_vs_fp64 [5] (the larger
relative difference of the two over the images, per layer: the reference's own fp32 error, which the
CPU test's tie of the restatement to the reference is scaled by).

Usage:  python tests/golden/make_lpips_goldens.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/MHAdaSTr"
for p in (os.path.join(REPO, "mhada-style-transfer_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import lpips_ref as L  # noqa: E402
import network  # noqa: E402

VGG_CFG_D = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


def features_with_test_weights() -> nn.Sequential:
    layers, c = [], 3
    for v in VGG_CFG_D:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            c = v
    feats = nn.Sequential(*layers)
    sd = L.kaiming_state_dict(network.VGG16())  # slice{s}.{i}.* -> features index i
    feats.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items()}, strict=True)
    return feats


def load_reference_lpips():
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.vgg16 = lambda weights=None, **kw: types.SimpleNamespace(features=features_with_test_weights())
    tv.models = models
    sys.modules.update({"torchvision": tv, "torchvision.models": models})
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = tq
    sys.path.insert(0, REF)
    import lpips
    return lpips


def main():
    torch.set_num_threads(8)
    lpips = load_reference_lpips()
    model = lpips.LPIPS(net="vgg", version="0.1", verbose=False)
    a = np.random.default_rng(5).integers(0, 256, (2, 48, 48, 3), dtype=np.uint8)
    b = L.golden_b()
    with torch.no_grad():
        # im2tensor takes one [H][W][3] image
        ta = torch.cat([lpips.im2tensor(img) for img in a])
        tb = torch.cat([lpips.im2tensor(img) for img in b])
        total, layers = model.forward(ta, tb, retPerLayer=True)
    ref_layers = np.stack([r.reshape(-1).double().numpy() for r in layers])  # [5][2]
    ref_total = total.reshape(-1).double().numpy()
    lins = [model.lins[k].model[-1].weight.detach().reshape(-1).numpy().astype(np.float32) for k in range(5)]

    vgg = L.vgg16_kaiming()
    f64a = [L.nhwc(t) for t in L.vgg16_taps(vgg, L.scaling64(a))]
    f64b = [L.nhwc(t) for t in L.vgg16_taps(vgg, L.scaling64(b))]
    fp64_layers = L.lpips64(f64a, f64b, lins)
    ref_vs_fp64 = (np.abs(ref_layers - fp64_layers) / fp64_layers).max(axis=1)

    share = ref_layers / ref_layers.sum(axis=0)
    print("layer shares of the total, per image:\n", share)
    assert (share >= 0.02).all(), "every layer must carry at least 2 % of the total (a condition on the fixture)"
    assert all(np.all(np.abs(f).sum(axis=-1) > 0) for f in f64a + f64b), "no pixel vector may be all zero"
    print("ref_total", ref_total, "\nref_vs_fp64", ref_vs_fp64)

    out = {"a": a, "b": b, "ref_layers": ref_layers, "ref_total": ref_total, "fp64_layers": fp64_layers,
           "ref_vs_fp64": ref_vs_fp64}
    out.update({f"lin{k}": w for k, w in enumerate(lins)})
    path = os.path.join(HERE, "lpips_vgg16_48_b2.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
