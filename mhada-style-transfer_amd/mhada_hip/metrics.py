"""Score stylised frames on the device: the twelve numbers of the reference's result tables
(eval.py, driven by exps_image.py; eight need no weights), on u8 frames [B][H][W][3] in device memory — what
``VideoStylizer.stylize_u8`` returns and what eval.py reads back from the PNG it wrote.

  ssim(a, b)                       SSIMMetric (eval.py:167-223)      mhada_ssim_u8, fp64 inside
  kl(a, b)                         kl_loss (eval.py:49-67)           mhada_hist_u8 + host fp64
  moment / uniformity / entropy    eval.py:111-164 on the gray image mhada_hist_u8 + host fp64
  gram(a, b, vgg)                  gram_loss (eval.py:78-108)        HIP VGG19, mhada_gemm_tn, mhada_feat_stats
  lpips(a, b, vgg16, lins)         lpips.LPIPS(net="vgg") (eval.py:22)  HIP VGG16, mhada_lpips_layer
  sifid(a, b, inception)           calculate_sifid_given_paths (eval.py:226-274)  HIP InceptionV3, mhada_sifid_*
  score(stylized, content, style)  the CSV row of exps_image.py:90-123, one value per image

LPIPS is here for callers who hand in a ``network.VGG16`` with ImageNet weights and the five linear
vectors of an lpips checkout (``lpips_weights``): the package ships and fetches no weights, so there
is no default, and without ``lpips=`` the two LPIPS keys are absent from ``score``, not NaN.  SIFID
follows the same rule: the caller hands in a ``network.InceptionV3`` with ImageNet weights
(``InceptionV3.load_torchvision``), and without ``sifid=`` its two keys are absent.  Frames may have padded rows; CPU tensors raise (no host fallback).  The
histogram metrics are finalised on the host from the 4 KB of exact counts, in numpy fp64 as the
reference computes them; the ``*_from_counts`` functions are that arithmetic and need no GPU.

The SSIM is held to the fp64 value of the reference's definition, not to its fp32 result: with
C2 = 0.03^2 applied to [0, 255] values the fp32 evaluation is rounding noise on smooth regions
("SSIM").

SIFID's input scale: exps_image.py hands SIFID PNG files, for which matplotlib's imread already returns
fp32 in [0, 1]; sifid_score.py:104 then divides by 255 again, so the trunk sees 2 (v / 255 / 255) - 1 in
[-1, -0.992].  That is the number in the reference's tables and the default here (``input_scale=
"reference"``); ``"unit"`` is v / 255, what a JPEG file gets there and what SIFID was designed for
("SIFID").
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops

SCORE_KEYS = ("ssim_content", "kl_c", "ssim_style", "kl_s", "gram", "moment", "uniformity", "entropy")
SCORE_KEYS_LPIPS = ("lpips_content", "ssim_content", "kl_c", "lpips_style", "ssim_style", "kl_s", "gram", "moment",
                    "uniformity", "entropy")  # the reference's CSV order, without sifid
SCORE_KEYS_FULL = ("lpips_content", "ssim_content", "sifid_content", "kl_c", "lpips_style", "ssim_style", "sifid_style",
                   "kl_s", "gram", "moment", "uniformity", "entropy")  # exps_image.py:108-125
_SIFID_DIMS = {64: 0, 192: 1, 768: 2, 2048: 3}  # inception.py:14-19
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


def frechet_from_moments(mu1, tr1: float, n1: int, mu2, tr2: float, n2: int, cross=None, scatter1=None,
                         scatter2=None) -> float:
    """calculate_frechet_distance (sifid_score.py:128-182), d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2),
    from fp64 moments of the two sets of feature rows (n1, n2 rows): ``mu`` the means [C], ``tr`` the
    centred sums of squares added over the channels (tr S = tr / (n - 1), np.cov's ddof 1), and either
      cross    = Xc1 Xc2^T [n1][n2]: the non-zero eigenvalues of S1 S2 are the squared singular values of
                 M = cross / sqrt((n1 - 1)(n2 - 1)), so tr sqrt(S1 S2) is M's nuclear norm — exact whatever the
                 rank, where sqrtm of the singular product S1 S2 returns a complex matrix with noise; or
      scatter1 = Xc1^T Xc1 and scatter2 [C][C]: sum sqrt(max(lambda, 0)) of eigvalsh(S1^(1/2) S2 S1^(1/2)).
    numpy fp64, no scipy, no GPU."""
    if n1 < 2 or n2 < 2:
        raise ValueError(f"frechet_from_moments: at least 2 feature rows per image are needed (np.cov of fewer is NaN), "
                         f"got {n1} and {n2}")
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    if mu1.shape != mu2.shape or mu1.ndim != 1:
        raise ValueError(f"frechet_from_moments: the means must be two [C] vectors, got {mu1.shape} and {mu2.shape}")
    if cross is not None:
        cross = np.asarray(cross, np.float64)
        if cross.shape != (n1, n2):
            raise ValueError(f"frechet_from_moments: cross must be [{n1}][{n2}], got {cross.shape}")
        tr_covmean = np.linalg.svd(cross / np.sqrt(float(n1 - 1) * float(n2 - 1)), compute_uv=False).sum()
    elif scatter1 is not None and scatter2 is not None:
        s1, s2 = np.asarray(scatter1, np.float64) / (n1 - 1), np.asarray(scatter2, np.float64) / (n2 - 1)
        if s1.shape != (mu1.size, mu1.size) or s2.shape != s1.shape:
            raise ValueError(f"frechet_from_moments: the scatter matrices must be [C][C], got {s1.shape} and {s2.shape}")
        lam, vec = np.linalg.eigh((s1 + s1.T) / 2)
        root = (vec * np.sqrt(np.maximum(lam, 0.0))) @ vec.T
        inner = root @ ((s2 + s2.T) / 2) @ root
        tr_covmean = np.sqrt(np.maximum(np.linalg.eigvalsh((inner + inner.T) / 2), 0.0)).sum()
    else:
        raise ValueError("frechet_from_moments: pass cross=, or scatter1= and scatter2=")
    diff = mu1 - mu2
    return float(diff.dot(diff) + tr1 / (n1 - 1) + tr2 / (n2 - 1) - 2.0 * tr_covmean)


def sifid_input_levels(input_scale: str = "reference") -> np.ndarray:
    """The fp32 trunk input of each of the 256 byte values, with the reference's own fp32 operations
    (sifid_score.py:97-104): "reference" = imread's v / 255 of a PNG (fp32) divided by 255 again; "unit" =
    v / 255, what a JPEG file gets there."""
    if input_scale not in ("reference", "unit"):
        raise ValueError(f"sifid: input_scale must be 'reference' or 'unit', got {input_scale!r}")
    v = np.arange(256, dtype=np.float32)
    v /= np.float32(255)
    if input_scale == "reference":
        v /= np.float32(255)
    return v


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


def _sifid_block(inception, dims: int) -> int:
    if dims not in _SIFID_DIMS:
        raise ValueError(f"sifid: dims must be one of {sorted(_SIFID_DIMS)}, got {dims!r}")
    if inception is None:
        raise ValueError("sifid: pass inception=network.InceptionV3() with its weights loaded (load_torchvision)")
    blk = _SIFID_DIMS[dims]
    if blk > inception.last_needed_block:
        raise ValueError(f"sifid: dims={dims} needs block {blk}, the InceptionV3 was built up to block "
                         f"{inception.last_needed_block}")
    return blk


@torch.no_grad()
def sifid_features(frames_u8: torch.Tensor, inception, dims: int = 2048, input_scale: str = "reference",
                   bgr: bool = True) -> torch.Tensor:
    """The Inception feature map of block ``dims`` of u8 frames as contiguous NHWC fp32 [B][H'][W'][dims]:
    the bytes go through the 256-entry table of ``sifid_input_levels`` (so the trunk's input is the
    reference's bit for bit), RGB order, then the HIP InceptionV3, which applies 2 x - 1."""
    blk = _sifid_block(inception, dims)
    levels = sifid_input_levels(input_scale)
    frames = ops._u8_input(frames_u8, "sifid")
    lut = torch.from_numpy(levels).to(frames.device)
    x = lut[frames.long()]  # [B][H][W][3], padded rows dropped by the view's shape
    if bgr:
        x = x.flip(-1)
    saved = inception.output_blocks
    inception.output_blocks = [blk]
    try:
        feat = inception(x.permute(0, 3, 1, 2))[0]
    finally:
        inception.output_blocks = saved
    return feat.permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def sifid_from_features(fa: torch.Tensor, fb: torch.Tensor) -> np.ndarray:
    """calculate_activation_statistics + calculate_frechet_distance (sifid_score.py:128-205) per image pair
    from two NHWC feature maps [B][H'][W'][C] (the two may differ in H', W'): float64 [B].  The moments are
    fp64 on the device (mhada_sifid_*); the cross form when an image has fewer positions than channels,
    else the covariance form."""
    if fa.dim() != 4 or fb.dim() != 4 or fa.shape[0] != fb.shape[0] or fa.shape[3] != fb.shape[3]:
        raise ValueError(f"sifid: two NHWC feature batches of one B and C, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    B, C = fa.shape[0], fa.shape[3]
    n1, n2 = fa.shape[1] * fa.shape[2], fb.shape[1] * fb.shape[2]
    if n1 < 2 or n2 < 2:
        raise ValueError(f"sifid: a feature map with fewer than 2 positions has no covariance (got {n1} and {n2}); "
                         "the images are too small for this dims")
    out = np.zeros(B)
    for i in range(B):
        x1, x2 = fa[i].reshape(n1, C), fb[i].reshape(n2, C)
        (m1, q1), (m2, q2) = ops.sifid_stats(x1), ops.sifid_stats(x2)
        kw = {}
        if min(n1, n2) < C:
            kw["cross"] = ops.sifid_cross(x1, m1, x2, m2).cpu().numpy()
        else:
            kw["scatter1"], kw["scatter2"] = ops.sifid_cov(x1, m1).cpu().numpy(), ops.sifid_cov(x2, m2).cpu().numpy()
        out[i] = frechet_from_moments(m1.cpu().numpy(), float(q1.cpu().numpy().sum()), n1, m2.cpu().numpy(),
                                      float(q2.cpu().numpy().sum()), n2, **kw)
    return out


def sifid(a_u8: torch.Tensor, b_u8: torch.Tensor, inception=None, dims: int = 2048, input_scale: str = "reference",
          bgr: bool = True) -> np.ndarray:
    """calculate_sifid_given_paths (eval.py:226-274, sifid_score.py:222-247) per image pair -> float64 [B]; the
    two batches may differ in H x W.  ``inception``: a ``network.InceptionV3`` on the frames' device with
    ImageNet weights (``load_torchvision``); there is no default.  ``input_scale``: see the module text."""
    _sifid_block(inception, dims)
    sifid_input_levels(input_scale)  # before any launch
    return sifid_from_features(sifid_features(a_u8, inception, dims, input_scale, bgr),
                               sifid_features(b_u8, inception, dims, input_scale, bgr))


def score(stylized_u8: torch.Tensor, content_u8: torch.Tensor, style_u8: torch.Tensor, bgr: bool = True,
          vgg=None, lpips=None, sifid=None) -> Dict[str, np.ndarray]:
    """The columns of exps_image.py's CSV for a batch, float64 [B] per key: the weight-free SCORE_KEYS, or
    with ``lpips=(vgg16, lins)`` (as in ``lpips``) the ten SCORE_KEYS_LPIPS in the CSV's order; the stylised
    frames' VGG16 features are computed once for both LPIPS columns.  ``sifid=inception`` (as in ``sifid``,
    dims 2048, the reference's input scale) adds ``sifid_content`` and ``sifid_style``, the stylised frames'
    trunk pass shared by both; with ``lpips=`` as well the row is the twelve SCORE_KEYS_FULL in the CSV's
    order.  ``vgg`` as in ``gram``; without one the ``gram`` key cannot be computed and the call raises."""
    if vgg is None:
        raise ValueError("score: pass vgg=network.VGG19() with its weights loaded (needed for 'gram')")
    lp = {}
    if lpips is not None:
        vgg16, lins = lpips
        _check_lins(lins)  # before any launch
        fs = vgg16_features(stylized_u8, vgg16, bgr)
        lp = {"lpips_content": lpips_from_features(fs, vgg16_features(content_u8, vgg16, bgr), lins),
              "lpips_style": lpips_from_features(fs, vgg16_features(style_u8, vgg16, bgr), lins)}
    sf = {}
    if sifid is not None:
        _sifid_block(sifid, 2048)  # before any launch
        fs = sifid_features(stylized_u8, sifid, bgr=bgr)
        sf = {"sifid_content": sifid_from_features(fs, sifid_features(content_u8, sifid, bgr=bgr)),
              "sifid_style": sifid_from_features(fs, sifid_features(style_u8, sifid, bgr=bgr))}
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
    if lp or sf:
        out.update(lp)
        out.update(sf)
        out = {k: out[k] for k in SCORE_KEYS_FULL if k in out}
    return out
