"""fp64 restatements of LPIPS(net="vgg", version="0.1") (lpips/lpips.py:129-171, lpips/__init__.py:13-15,
86-88) for the LPIPS tests and the golden maker: plain numpy / aten on host memory, no device code.

  scaling64(u8)               im2tensor + ScalingLayer: (u / 127.5 - 1 - shift) / scale, NCHW fp64
  normalize64(f)              normalize_tensor over the channel axis of an NHWC map
  lpips_layer64(fa, fb, w)    one layer's distance per image from NHWC maps -> [B]
  lpips64(feats_a, feats_b, lins)   the five layers -> [5][B]
  bound_layer(fa, fb, w)      the a-priori fp32 error bound of one layer of the device head -> [B]
  vgg16_kaiming()             the test trunk: the "vgg16" recipe with every conv weight times sqrt(6)
  vgg16_taps(vgg, x, dtype)   aten VGG16 forward on an already normalised NCHW input, in `dtype`
"""
import math

import numpy as np
import torch

SHIFT = (-0.030, -0.088, -0.188)  # ScalingLayer, lpips.py:167-168
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
TAPS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
CHNS = (64, 128, 256, 512, 512)


def scaling64(u8) -> np.ndarray:
    """u8 RGB frames [B][H][W][3] -> the trunk's input [B][3][H][W] in fp64: im2tensor's u / (255 / 2) - 1
    (lpips/__init__.py:86-88), then ScalingLayer's (x - shift) / scale (lpips.py:170-171)."""
    x = np.asarray(u8).astype(np.float64) / (255.0 / 2.0) - 1.0
    x = (x - np.array(SHIFT)) / np.array(SCALE)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def normalize64(f) -> np.ndarray:
    """normalize_tensor (lpips/__init__.py:13-15) of an NHWC map: f / (sqrt(sum_c f^2) + 1e-10)."""
    f = np.asarray(f, dtype=np.float64)
    return f / (np.sqrt((f * f).sum(axis=-1, keepdims=True)) + EPS)


def _pixels(f) -> np.ndarray:
    f = np.asarray(f, dtype=np.float64)
    return f.reshape(f.shape[0], -1, f.shape[-1])


def lpips_layer64(fa, fb, w) -> np.ndarray:
    """mean over the pixels of sum_c w_c (a^_c - b^_c)^2 (lpips.py:140-147) -> [B]."""
    d = normalize64(_pixels(fa)) - normalize64(_pixels(fb))
    return (d * d * np.asarray(w, dtype=np.float64)).sum(axis=-1).mean(axis=-1)


def lpips64(feats_a, feats_b, lins) -> np.ndarray:
    return np.stack([lpips_layer64(fa, fb, w) for fa, fb, w in zip(feats_a, feats_b, lins)])


def bound_layer(fa, fb, w) -> np.ndarray:
    """(2C + 16) 2^-24 mean_p sum_c |w_c| (|a^_c| + |b^_c|)^2 -> [B]: the first-order bound of the fp32
    per-pixel arithmetic in any summation order.  The norm puts C / 2 + 3 roundings on each a^_c; the
    difference doubles that against |a^| + |b^|; the square, the weight and the C-term sum add C + 3; 6
    units more for a hardware reciprocal or square root of one ulp.  The fp64 pixel sum adds nothing
    visible.  Zero exactly where both vectors are zero at every pixel."""
    a, b = np.abs(normalize64(_pixels(fa))), np.abs(normalize64(_pixels(fb)))
    C = a.shape[-1]
    s = ((a + b) ** 2 * np.abs(np.asarray(w, dtype=np.float64))).sum(axis=-1).mean(axis=-1)
    return (2 * C + 16) * 2.0 ** -24 * s


def kaiming_state_dict(module) -> dict:
    """The "vgg16" recipe for `module`'s keys with every conv weight times sqrt(6) (biases as they are):
    with the recipe's plain U(+-1/sqrt(fan_in)) weights the activations shrink layer by layer until the
    biases dominate and layers 4 and 5 carry 1e-4 and less of the LPIPS total, so that a wrong lin3 or
    lin4 would be invisible; at the Kaiming scale every layer carries several per cent."""
    from mhada_hip.recipe import recipe_state_dict
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = recipe_state_dict("vgg16", shapes)
    return {k: v * math.sqrt(6.0) if k.endswith("weight") else v for k, v in sd.items()}


def vgg16_kaiming():
    import network
    vgg = network.VGG16()
    vgg.load_state_dict(kaiming_state_dict(vgg), strict=True)
    return vgg.eval()


@torch.no_grad()
def vgg16_taps(vgg, x, dtype=torch.float64):
    """The five taps of cfg D features[0:30] by aten, from `vgg`'s slice{s}.{i} weights cast to `dtype`, on
    the normalised NCHW input x -> list of NCHW tensors."""
    import torch.nn.functional as F
    x = torch.as_tensor(x).to(dtype)
    taps = []
    for s in range(1, 6):
        for m in getattr(vgg, f"slice{s}"):
            if isinstance(m, torch.nn.Conv2d):
                x = F.relu(F.conv2d(x, m.weight.detach().cpu().to(dtype), m.bias.detach().cpu().to(dtype), padding=1))
            elif isinstance(m, torch.nn.MaxPool2d):
                x = F.max_pool2d(x, 2, 2)
        taps.append(x)
    return taps


def nhwc(t) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy().transpose(0, 2, 3, 1))


def golden_b() -> np.ndarray:
    """The arithmetic pattern of the golden's second batch, u8 RGB [2][48][48][3]."""
    y, x = np.mgrid[0:48, 0:48]
    return np.stack([np.stack([(7 * x + 40 * n) % 256, (5 * y + 9 * x) % 256, (x * y // 4) % 256], -1)
                     for n in range(2)]).astype(np.uint8)
