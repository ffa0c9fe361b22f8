"""Score stylised frames on the device: ten of the twelve numbers of the reference's result tables
(eval.py, driven by exps_image.py; eight need no weights), on u8 frames [B][H][W][3] in device memory — what
``VideoStylizer.stylize_u8`` returns and what eval.py reads back from the PNG it wrote.

  ssim(a, b)                       SSIMMetric (eval.py:167-223)      mhada_ssim_u8, fp64 inside
  kl(a, b)                         kl_loss (eval.py:49-67)           mhada_hist_u8 + host fp64
  moment / uniformity / entropy    eval.py:111-164 on the gray image mhada_hist_u8 + host fp64
  gram(a, b, vgg)                  gram_loss (eval.py:78-108)        HIP VGG19, mhada_gemm_tn, mhada_feat_stats
  lpips(a, b, vgg16, lins)         lpips.LPIPS(net="vgg") (eval.py:22)  HIP VGG16, mhada_lpips_layer
  score(stylized, content, style)  the CSV row of exps_image.py:90-123, one value per image

LPIPS is here for callers who hand in a ``network.VGG16`` with ImageNet weights and the five linear
vectors of an lpips checkout (``lpips_weights``): the package ships and fetches no weights, so there
is no default, and without ``lpips=`` the two LPIPS keys are absent from ``score``, not NaN.  SIFID
needs Inception and is not here.  Frames may have padded rows; CPU tensors raise (no host fallback).  The
histogram metrics are finalised on the host from the 4 KB of exact counts, in numpy fp64 as the
reference computes them; the ``*_from_counts`` functions are that arithmetic and need no GPU.

The SSIM is held to the fp64 value of the reference's definition, not to its fp32 result: with
C2 = 0.03^2 applied to [0, 255] values the fp32 evaluation is rounding noise on smooth regions
("SSIM").
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops

SCORE_KEYS = ("ssim_content", "kl_c", "ssim_style", "kl_s", "gram", "moment", "uniformity", "entropy")
SCORE_KEYS_LPIPS = ("lpips_content", "ssim_content", "kl_c", "lpips_style", "ssim_style", "kl_s", "gram", "moment",
                    "uniformity", "entropy")  # the reference's CSV order, without sifid
_VGG_LAYERS = tuple(f"relu{i}_1" for i in range(1, 6))
_LPIPS_CHNS = (64, 128, 256, 512, 512)  # lpips.py:91


# ---- host finalisers: counts -> numbers (numpy fp64; no GPU, no scipy) ---------------------
def _counts(c) -> np.ndarray:
    c = np.asarray(c)
    if c.shape[-1] != 256:
        raise ValueError(f"counts must end in 256 bins, got {c.shape}")
    return c.astype(np.int64)


def kl_from_counts(ca, cb) -> np.ndarray:
    """kl_loss (eval.py:49-67) from the channel counts [..., >=3, 256] of the two images: per channel
    hist + 1, scipy.stats.entropy(p, q) = sum p ln(p / q) of the normalised histograms, mean of the
    first 3 planes."""
    p = (_counts(ca)[..., :3, :] + 1).astype(np.float64)
    q = (_counts(cb)[..., :3, :] + 1).astype(np.float64)
    p = p / p.sum(axis=-1, keepdims=True)
    q = q / q.sum(axis=-1, keepdims=True)
    return (p * np.log(p / q)).sum(axis=-1).sum(axis=-1) / 3.0


def _gray_hist(gray_counts):
    hist = _counts(gray_counts) + 1  # compute_histogram's + 1
    return hist, hist / np.sum(hist, axis=-1, keepdims=True)


def moment_from_counts(gray_counts) -> np.ndarray:
    """nth_order_moment (eval.py:111-129) from the gray counts [..., 256], as written there: the
    "normalised" histogram is the COUNTS / 255, its mean is taken over the 256 bins."""
    hist, hist_p = _gray_hist(gray_counts)
    hist = hist / 255.0
    mean = np.mean(hist, axis=-1, keepdims=True)
    return (((hist - mean) ** 2) * hist_p).sum(axis=-1)


def uniformity_from_counts(gray_counts) -> np.ndarray:
    """uniformity (eval.py:132-146): sum of p^2."""
    _, hist_p = _gray_hist(gray_counts)
    return (hist_p ** 2).sum(axis=-1)


def entropy_from_counts(gray_counts) -> np.ndarray:
    """average_entropy (eval.py:149-164): -sum p log2 p (every p > 0 after the + 1)."""
    _, hist_p = _gray_hist(gray_counts)
    return -(hist_p * np.log2(hist_p)).sum(axis=-1)


# ---- device metrics ------------------------------------------------------------------------
def _hist(frames: torch.Tensor, bgr: bool = True) -> np.ndarray:
    return ops.hist_u8(frames, bgr=bgr).cpu().numpy()


def ssim(a_u8: torch.Tensor, b_u8: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """SSIMMetric(11, 3, 1.5, reduction) on the u8 values: fp32 [B] for "none", their fp32 mean (0-dim)
    for "mean"."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"ssim: reduction must be 'mean' or 'none', got {reduction!r}")
    per_image = ops.ssim_u8(a_u8, b_u8)
    return per_image.mean() if reduction == "mean" else per_image


def kl(a_u8: torch.Tensor, b_u8: torch.Tensor) -> np.ndarray:
    """kl_loss per image -> float64 [B]."""
    ca, cb = _hist(a_u8), _hist(b_u8)
    if ca.shape != cb.shape:
        raise ValueError("kl: the two batches differ in size")
    return kl_from_counts(ca, cb)


def moment(a_u8: torch.Tensor, bgr: bool = True) -> np.ndarray:
    return moment_from_counts(_hist(a_u8, bgr)[:, 3])


def uniformity(a_u8: torch.Tensor, bgr: bool = True) -> np.ndarray:
    return uniformity_from_counts(_hist(a_u8, bgr)[:, 3])


def entropy(a_u8: torch.Tensor, bgr: bool = True) -> np.ndarray:
    return entropy_from_counts(_hist(a_u8, bgr)[:, 3])


@torch.no_grad()
def vgg_features(frames_u8: torch.Tensor, vgg, bgr: bool = True):
    """relu1_1 .. relu5_1 of u8 frames as contiguous NHWC fp32 tensors: cv2_to_tensor (BGR->RGB, 0..255
    fp32; ops.frame_ingest) then the HIP VGG19."""
    feats = vgg(ops.frame_ingest(frames_u8, bgr=bgr))
    return [feats[k].permute(0, 2, 3, 1).contiguous() for k in _VGG_LAYERS]


@torch.no_grad()
def gram_from_features(feats_a, feats_b) -> np.ndarray:
    """gram_loss (eval.py:92-103) per image from two lists of NHWC feature maps: the sum over the
    layers of F.mse_loss of the two Gram matrices, divided by 5 (the number of layers)."""
    B = feats_a[0].shape[0]
    per_layer = []
    for fa, fb in zip(feats_a, feats_b):
        ga, gb = ops.gram(fa), ops.gram(fb)  # [B][C][C]
        C = ga.shape[-1]
        per_layer.append(torch.stack([ops.feat_stats(ga[i].view(1, 1, C, C), gb[i].view(1, 1, C, C), stats=False)[2]
                                      for i in range(B)]))
    tot = torch.stack(per_layer).double().cpu().numpy()  # [layers][B]
    out = np.zeros(B)
    for layer in tot:  # the reference adds the layers in order
        out = out + layer
    return out / float(len(feats_a))


def gram(a_u8: torch.Tensor, b_u8: torch.Tensor, vgg=None, bgr: bool = True) -> np.ndarray:
    """gram_loss per image -> float64 [B].  ``vgg``: a ``network.VGG19`` on the frames' device — the
    reference's is torchvision's ImageNet VGG19 (``VGG19.load_torchvision_features`` loads it from a
    local file); there is no default, because this package cannot fetch those weights."""
    if vgg is None:
        raise ValueError("gram: pass vgg=network.VGG19() with its weights loaded (load_torchvision_features)")
    return gram_from_features(vgg_features(a_u8, vgg, bgr), vgg_features(b_u8, vgg, bgr))


def lpips_weights(src) -> List[torch.Tensor]:
    """The five linear-layer vectors of LPIPS(net="vgg", version="0.1") as fp32 CPU tensors [C], C = 64, 128,
    256, 512, 512, from a LOCAL ``weights/v0.1/vgg.pth`` of an lpips checkout, a path to it or its
    state_dict: exactly the keys ``lin{0..4}.model.1.weight`` of shape (1, C, 1, 1) (strict).  Loaded with
    ``weights_only=True`` onto the CPU (the shipped file was saved from a CUDA device)."""
    sd = torch.load(src, map_location="cpu", weights_only=True) if not isinstance(src, dict) else src
    want = {f"lin{k}.model.1.weight": (1, c, 1, 1) for k, c in enumerate(_LPIPS_CHNS)}
    if set(sd) != set(want):
        raise KeyError(f"lpips_weights: expected the keys {sorted(want)}, got {sorted(sd)}")
    for key, shape in want.items():
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"lpips_weights: {key} must be {shape}, got {tuple(sd[key].shape)}")
    return [sd[key].detach().to("cpu", torch.float32).reshape(-1).contiguous() for key in want]


@torch.no_grad()
def vgg16_features(frames_u8: torch.Tensor, vgg16, bgr: bool = True):
    """relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of u8 frames as contiguous NHWC fp32 tensors:
    ops.frame_ingest (BGR->RGB, 0..255 fp32) then the HIP VGG16, whose fused normalisation is LPIPS's
    im2tensor + ScalingLayer."""
    feats = vgg16(ops.frame_ingest(frames_u8, bgr=bgr))
    return [feats[k].permute(0, 2, 3, 1).contiguous() for k in ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")]


def _check_lins(lins) -> None:
    if len(lins) != len(_LPIPS_CHNS):
        raise ValueError(f"lpips: {len(_LPIPS_CHNS)} linear-layer vectors are needed (lpips_weights), got {len(lins)}")


def _lins_on(lins, device) -> List[torch.Tensor]:
    _check_lins(lins)
    return [w.to(device=device, dtype=torch.float32).contiguous() for w in lins]


@torch.no_grad()
def lpips_from_features(feats_a, feats_b, lins, per_layer: bool = False) -> np.ndarray:
    """LPIPS.forward (lpips.py:139-156) per image from two lists of the five NHWC feature maps: float64 [B],
    the layers' distances (ops.lpips_layer) added in order 0..4; per_layer: the [5][B] distances themselves."""
    if len(feats_a) != len(_LPIPS_CHNS) or len(feats_b) != len(_LPIPS_CHNS):
        raise ValueError(f"lpips: {len(_LPIPS_CHNS)} feature maps per image are needed")
    lins = _lins_on(lins, feats_a[0].device)
    layers = torch.stack([ops.lpips_layer(fa, fb, w) for fa, fb, w in zip(feats_a, feats_b, lins)]).cpu().numpy()
    if per_layer:
        return layers
    out = np.zeros(layers.shape[1])
    for layer in layers:  # the reference adds the layers in order
        out = out + layer
    return out


def lpips(a_u8: torch.Tensor, b_u8: torch.Tensor, vgg16=None, lins=None, bgr: bool = True,
          per_layer: bool = False) -> np.ndarray:
    """lpips.LPIPS(net="vgg")(im2tensor(a), im2tensor(b)) per image -> float64 [B] ([5][B] per layer).
    ``vgg16``: a ``network.VGG16`` on the frames' device with ImageNet weights
    (``VGG16.load_torchvision_features``); ``lins``: ``lpips_weights(...)``.  Neither has a default."""
    if vgg16 is None or lins is None:
        raise ValueError("lpips: pass vgg16=network.VGG16() with its weights loaded and lins=lpips_weights(path)")
    _check_lins(lins)  # before any launch
    return lpips_from_features(vgg16_features(a_u8, vgg16, bgr), vgg16_features(b_u8, vgg16, bgr), lins, per_layer)


def score(stylized_u8: torch.Tensor, content_u8: torch.Tensor, style_u8: torch.Tensor, bgr: bool = True,
          vgg=None, lpips=None) -> Dict[str, np.ndarray]:
    """The columns of exps_image.py's CSV for a batch, float64 [B] per key: the weight-free SCORE_KEYS, or
    with ``lpips=(vgg16, lins)`` (as in ``lpips``) the ten SCORE_KEYS_LPIPS in the CSV's order; the stylised
    frames' VGG16 features are computed once for both LPIPS columns.  ``vgg`` as in ``gram``; without one
    the ``gram`` key cannot be computed and the call raises."""
    if vgg is None:
        raise ValueError("score: pass vgg=network.VGG19() with its weights loaded (needed for 'gram')")
    lp = {}
    if lpips is not None:
        vgg16, lins = lpips
        _check_lins(lins)  # before any launch
        fs = vgg16_features(stylized_u8, vgg16, bgr)
        lp = {"lpips_content": lpips_from_features(fs, vgg16_features(content_u8, vgg16, bgr), lins),
              "lpips_style": lpips_from_features(fs, vgg16_features(style_u8, vgg16, bgr), lins)}
    hs = _hist(stylized_u8, bgr)
    out = {
        "ssim_content": ssim(stylized_u8, content_u8, "none").double().cpu().numpy(),
        "kl_c": kl_from_counts(hs, _hist(content_u8, bgr)),
        "ssim_style": ssim(stylized_u8, style_u8, "none").double().cpu().numpy(),
        "kl_s": kl_from_counts(hs, _hist(style_u8, bgr)),
        "gram": gram(stylized_u8, style_u8, vgg, bgr),
        "moment": moment_from_counts(hs[:, 3]),
        "uniformity": uniformity_from_counts(hs[:, 3]),
        "entropy": entropy_from_counts(hs[:, 3]),
    }
    assert tuple(out) == SCORE_KEYS
    if lp:
        out.update(lp)
        out = {k: out[k] for k in SCORE_KEYS_LPIPS}
    return out
