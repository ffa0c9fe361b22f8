"""Score stylised frames on the device: the eight weight-free numbers of the reference's result
tables (eval.py, driven by exps_image.py), on u8 frames [B][H][W][3] in device memory — what
``VideoStylizer.stylize_u8`` returns and what eval.py reads back from the PNG it wrote.

  ssim(a, b)                       SSIMMetric (eval.py:167-223)      mhada_ssim_u8, fp64 inside
  kl(a, b)                         kl_loss (eval.py:49-67)           mhada_hist_u8 + host fp64
  moment / uniformity / entropy    eval.py:111-164 on the gray image mhada_hist_u8 + host fp64
  gram(a, b, vgg)                  gram_loss (eval.py:78-108)        HIP VGG19, mhada_gemm_tn, mhada_feat_stats
  score(stylized, content, style)  the CSV row of exps_image.py:90-123, one value per image

LPIPS and SIFID need downloaded VGG16 / Inception weights and are not here (their keys are absent
from ``score``, not NaN).  Frames may have padded rows; CPU tensors raise (no host fallback).  The
histogram metrics are finalised on the host from the 4 KB of exact counts, in numpy fp64 as the
reference computes them; the ``*_from_counts`` functions are that arithmetic and need no GPU.

The SSIM is held to the fp64 value of the reference's definition, not to its fp32 result: with
C2 = 0.03^2 applied to [0, 255] values the fp32 evaluation is rounding noise on smooth regions
("SSIM").
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops

SCORE_KEYS = ("ssim_content", "kl_c", "ssim_style", "kl_s", "gram", "moment", "uniformity", "entropy")
_VGG_LAYERS = tuple(f"relu{i}_1" for i in range(1, 6))


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


def score(stylized_u8: torch.Tensor, content_u8: torch.Tensor, style_u8: torch.Tensor, bgr: bool = True,
          vgg=None) -> Dict[str, np.ndarray]:
    """The weight-free columns of exps_image.py's CSV (SCORE_KEYS) for a batch: float64 [B] per key.
    ``vgg`` as in ``gram``; without one the ``gram`` key cannot be computed and the call raises."""
    if vgg is None:
        raise ValueError("score: pass vgg=network.VGG19() with its weights loaded (needed for 'gram')")
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
    return out
