"""Image-path ingest, the twin of ``video.cv2_to_tensor``: the input preparation every image entry point of
the reference shares (infer_image.py:69,76, exps_image.py, exps_image_all.py, visual_*.py, and the style image
of infer_video.py:58),

    toTensor255(Image.open(p).convert("RGB").resize((W, H), Image.BILINEAR))

with the resize on the device, bit for bit as PIL computes it (``ops.image_resize``, csrc/image_ingest.hip).
The image is uploaded at full size and read once; decoding the file stays with the caller.

* ``pil_to_tensor(img, size, device)`` — the fp32 (3, H, W) model input in [0, 255];
* ``resize_u8(img, size, device)`` — the resized u8 (H, W, 3) R,G,B image, what the reference saves as
  content.png / style.png and what ``metrics.score(..., bgr=False)`` consumes;
* ``prepare(img, size, device)`` — both from one call.

``img`` is a ``PIL.Image`` (converted to RGB if it is not), a numpy (H, W, 3) uint8 array or a uint8 tensor
(on the device or not), R,G,B; ``size`` = (width, height) as ``Image.resize`` takes it.  The package does not need PIL: a PIL image
is recognised by its interface, so only a caller who passes one has imported it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops


def _to_device_u8(img, device: Optional[torch.device]) -> torch.Tensor:
    """``img`` as a uint8 (H, W, 3) tensor on ``device`` (default the current ROCm device); a host image goes up
    through pinned memory, a device tensor is taken as it is (its rows may be padded)."""
    if not isinstance(img, (torch.Tensor, np.ndarray)):
        if not (hasattr(img, "convert") and hasattr(img, "mode")):
            raise ValueError(f"expected a PIL image, a numpy array or a tensor, got {type(img).__name__}")
        # a PIL image (recognised by its interface: this module never imports PIL itself)
        img = np.array(img if img.mode == "RGB" else img.convert("RGB"))
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"expected a uint8 (H, W, 3) R,G,B image, got {t.dtype} {tuple(t.shape)}")
    if t.is_cuda and device is None:
        return t
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if t.is_cuda:
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


def _out_hw(size):
    return int(size[1]), int(size[0])


def prepare(img, size, device: Optional[torch.device] = None):
    """(the resized uint8 (H, W, 3) R,G,B image, the fp32 (3, H, W) tensor toTensor255 makes of it), both on the
    device, from one pass over the full-size image; ``size`` = (width, height)."""
    u8, f32 = ops.image_resize(_to_device_u8(img, device), _out_hw(size), bgr=False)
    return u8[0], f32[0]


def pil_to_tensor(img, size, device: Optional[torch.device] = None) -> torch.Tensor:
    """``toTensor255(img.resize(size, Image.BILINEAR))`` (infer_image.py:69,76) as the fp32 (3, H, W) tensor in
    [0, 255] on the device (the reference builds it on the CPU and moves it with ``.to(device)``)."""
    return ops.image_resize(_to_device_u8(img, device), _out_hw(size), bgr=False, want_u8=False)[1][0]


def resize_u8(img, size, device: Optional[torch.device] = None) -> torch.Tensor:
    """``img.resize(size, Image.BILINEAR)`` as the uint8 (H, W, 3) R,G,B device tensor, ready for
    ``metrics.score(..., bgr=False)``."""
    return ops.image_resize(_to_device_u8(img, device), _out_hw(size), bgr=False, want_f32=False)[0][0]
