"""Feature inversion: optimise an image until a frozen network's features match given targets.

The loop of the reference's ``visual_vit.py:97-112`` (the content ViT alone) and
``visual_mhada.py:112-127`` (the content ViT and the six MHAda blocks, style features from a
no-grad call): Adam on the image, loss = sum over the returned feature maps of their MSE against
the targets.  The networks are the ``network`` modules with ``requires_grad_(False)``; on a ROCm
device their forward and backward run on the HIP training kernels (``autograd_path``), the image
gradient from ``mhada_patch_embed_dgrad``.  No file I/O and no min-max normalisation: the caller
owns both.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import torch
import torch.nn.functional as F


def invert_features(forward_fn: Callable[[torch.Tensor], Sequence[torch.Tensor]], targets: Sequence[torch.Tensor],
                    init: torch.Tensor, steps: int, lr: float) -> Tuple[torch.Tensor, List[float]]:
    """Run ``steps`` Adam iterations (learning rate ``lr``) on a copy of ``init`` minimising
    ``sum_l mse(forward_fn(image)[l], targets[l])``.  ``forward_fn`` returns one feature map per
    target (a single tensor counts as a list of one).  Returns the optimised image (detached) and
    the loss of every iteration, evaluated before that iteration's update."""
    if isinstance(targets, torch.Tensor):
        targets = [targets]
    image = init.detach().clone().requires_grad_(True)
    optimizer = torch.optim.Adam([image], lr=lr)
    history: List[float] = []
    for _ in range(steps):
        optimizer.zero_grad()
        feats = forward_fn(image)
        if isinstance(feats, torch.Tensor):
            feats = [feats]
        if len(feats) != len(targets):
            raise ValueError(f"invert_features: forward_fn returned {len(feats)} feature maps for {len(targets)} targets")
        loss = sum(F.mse_loss(f, t) for f, t in zip(feats, targets))
        loss.backward()
        optimizer.step()
        history.append(loss.item())
    return image.detach(), history
