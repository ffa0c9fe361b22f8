"""Frozen VGG16 trunk of LPIPS — drop-in for ``MHAdaSTr/lpips/pretrained_networks.py:98-136``.

The reference pulls ImageNet weights from torchvision at construction (a network fetch this
package cannot make); here the layers are built with the same indices, so the state_dict keys are
those of the reference's ``LPIPS.net``, ``slice{1..5}.{idx}.{weight,bias}``, and a local torchvision
checkpoint loads through ``load_torchvision_features``.  ``forward`` takes the image in [0, 255]
(what ``ops.frame_ingest`` returns and ``VGG19`` takes) and applies the ImageNet normalisation, which
is LPIPS's ScalingLayer after im2tensor; on a ROCm device it runs the HIP kernels of the VGG19 path
(fused normalising stem, Winograd / implicit-GEMM convs with fused ReLU, max-pool; inference only),
on the CPU aten.
"""
import torch.nn as nn

from . import _path  # noqa: F401
from mhada_hip import autograd_path

# torchvision vgg16 cfg "D" features[0:30]: (index, in, out) of each 3x3 conv; ReLU follows each
# conv, MaxPool2d(2) at 4, 9, 16, 23.  A pool opens the next slice: the taps are relu1_2 .. relu5_3.
_CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256),
          (14, 256, 256), (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512),
          (28, 512, 512)]
_POOLS = (4, 9, 16, 23)
_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))


class VGG16(nn.Module):
    def __init__(self):
        super().__init__()
        convs = {i: (ci, co) for i, ci, co in _CONVS}
        for s, (a, b) in enumerate(_SLICES, start=1):
            seq = nn.Sequential()
            for x in range(a, b):
                if x in convs:
                    seq.add_module(str(x), nn.Conv2d(convs[x][0], convs[x][1], 3, padding=1))
                elif x in _POOLS:
                    seq.add_module(str(x), nn.MaxPool2d(2, 2))
                else:
                    seq.add_module(str(x), nn.ReLU(inplace=True))
            setattr(self, f"slice{s}", seq)
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, x):
        return autograd_path.vgg16_forward(self, x)

    def load_torchvision_features(self, src) -> None:
        """ImageNet weights from a LOCAL torchvision VGG16 checkpoint — the file that
        ``torchvision.models.vgg16(weights="VGG16_Weights.IMAGENET1K_V1")`` (pretrained_networks.py:101)
        downloads (``vgg16-397923af.pth``), a path to it or its state_dict: ``features.{i}.{weight,bias}``
        load into ``slice{s}.{i}``; the classifier is ignored.  Loaded with ``weights_only=True``.  Every
        conv of the five slices must be present (strict), shapes must match."""
        import torch
        sd = torch.load(src, map_location="cpu", weights_only=True) if not isinstance(src, dict) else src
        convs = {c[0] for c in _CONVS}
        own = {}
        for s, (a, b) in enumerate(_SLICES, start=1):
            for i in (x for x in range(a, b) if x in convs):
                for t in ("weight", "bias"):
                    key = f"features.{i}.{t}"
                    if key not in sd:
                        raise KeyError(f"load_torchvision_features: {key} missing")
                    own[f"slice{s}.{i}.{t}"] = sd[key]
        self.load_state_dict(own, strict=True)
