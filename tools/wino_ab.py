"""A/B timing of the fp32 Winograd conv kernels (s3: the SPLIT3 kernel on the bf16 MFMA, tuning
wino_split3 = 1; w4 / w8: the fp32-MFMA kernels, wino_split3 = 0 with wino4 = 1 / 0) on the
decoder / VGG / input-gradient shapes of the 512^2 batch-8 step and the training step, interleaved
rounds in one process.

    python tools/wino_ab.py

Ablations of the 4-wave kernel (profiles/r05_wino4_ablate.log) come from builds with
-DWINO4_DBG=<mask> (1 no DMA, 2 no transform, 4 no MFMA, 8 no DMA wait; results invalid).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd"), os.path.dirname(os.path.abspath(__file__))]

import torch

from mhada_hip import _lib, ops
from opbench import bench


def main():
    dev = "cuda"
    torch.manual_seed(0)
    # the decoder's eight launches are these six reflect shapes (256 -> 256 at 128^2 runs three
    # times); zero pad 1: VGG19 forward; zero pad 2: the training input gradients (full correlation)
    for (B, H, Ci, Co, pad_mode, pad) in [(8, 64, 512, 256, "reflect", 1), (8, 128, 256, 256, "reflect", 1),
                                          (8, 128, 256, 128, "reflect", 1), (8, 256, 128, 128, "reflect", 1),
                                          (8, 256, 128, 64, "reflect", 1), (8, 512, 64, 64, "reflect", 1),
                                          (8, 256, 64, 128, "zero", 1), (8, 128, 128, 256, "zero", 1),
                                          (8, 64, 256, 512, "zero", 1), (8, 126, 256, 128, "zero", 2),
                                          (8, 254, 128, 64, "zero", 2)]:
        x = torch.randn(B, H, H, Ci, device=dev)
        w = torch.randn(Co, 9 * Ci, device=dev) / (9 * Ci) ** 0.5
        b = torch.randn(Co, device=dev)
        u = ops.wino_weights(w)
        Ho = H + 2 * (pad - 1)
        out = torch.empty(B, Ho, Ho, Co, device=dev)

        def run(s3, k):
            with _lib.tuning(wino_split3=s3, wino4=k):
                ops.conv3x3_wino(x, u, b, True, pad_mode, pad, out=out)
        t = bench({"w8": lambda: run(0, 0), "w4": lambda: run(0, 1), "s3": lambda: run(1, 1)})
        fl = 2 * B * H * H * Co * 9 * Ci / 2.25  # Winograd products
        print(f"wino {pad_mode:7s}{pad} B={B} {H:3d}^2 {Ci:3d}->{Co:3d}: " + "  ".join(
            f"{k} {v * 1e3:7.1f} us {fl / v / 1e9:6.1f} TF(wino)" for k, v in t.items()), flush=True)


if __name__ == "__main__":
    main()
