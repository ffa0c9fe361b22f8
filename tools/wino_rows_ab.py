"""A/B timing of the two SPLIT3 Winograd conv layouts: wino_s3_kernel (tuning wino_s3_rows = 0: each wave all 16
positions of 32 tiles x 32 channels) against wino_s3_rows_kernel (1: one Winograd row per wave), interleaved
rounds in one process on the shapes of tools/wino_ab.py: the decoder's eight launches of the 512^2 batch-8 step
(six distinct shapes; 256 -> 256 at 128^2 runs three times), VGG19's three and the two input-gradient shapes.

    python tools/wino_rows_ab.py

Columns: rows0 and rows0' are the same kernel timed twice per round (their difference is the A-against-A spread of
this run), rows1 the new layout; gain = rows0 / rows1 and its spread counterpart rows0 / rows0'.  A shape counts
as faster only where |gain - 1| exceeds |A/A - 1|.  The outputs of the two layouts are compared with torch.equal.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd"), os.path.dirname(os.path.abspath(__file__))]

import torch

from mhada_hip import _lib, ops
from opbench import bench

SHAPES = [(8, 64, 512, 256, "reflect", 1, 1), (8, 128, 256, 256, "reflect", 1, 3), (8, 128, 256, 128, "reflect", 1, 1),
          (8, 256, 128, 128, "reflect", 1, 1), (8, 256, 128, 64, "reflect", 1, 1), (8, 512, 64, 64, "reflect", 1, 1),
          (8, 256, 64, 128, "zero", 1, 0), (8, 128, 128, 256, "zero", 1, 0), (8, 64, 256, 512, "zero", 1, 0),
          (8, 126, 256, 128, "zero", 2, 0), (8, 254, 128, 64, "zero", 2, 0)]


def main():
    dev = "cuda"
    torch.manual_seed(0)
    step = [0.0, 0.0, 0.0]
    for (B, H, Ci, Co, pad_mode, pad, per_step) in SHAPES:
        x = torch.randn(B, H, H, Ci, device=dev)
        w = torch.randn(Co, 9 * Ci, device=dev) / (9 * Ci) ** 0.5
        b = torch.randn(Co, device=dev)
        u = ops.wino_weights(w)
        Ho = H + 2 * (pad - 1)
        out = torch.empty(B, Ho, Ho, Co, device=dev)

        def run(rows):
            with _lib.tuning(wino_s3_rows=rows):
                return ops.conv3x3_wino(x, u, b, True, pad_mode, pad, out=out)
        same = torch.equal(run(0).clone(), run(1))
        t = bench({"rows0": lambda: run(0), "rows1": lambda: run(1), "rows0'": lambda: run(0)})
        for i, k in enumerate(("rows0", "rows0'", "rows1")):
            step[i] += per_step * t[k]
        fl = 2 * B * H * H * Co * 9 * Ci / 2.25  # Winograd products
        a, a2, n = t["rows0"], t["rows0'"], t["rows1"]
        print(f"wino {pad_mode:7s}{pad} B={B} {H:3d}^2 {Ci:3d}->{Co:3d} x{per_step}: rows0 {a * 1e3:7.1f} us  "
              f"rows0' {a2 * 1e3:7.1f} us  rows1 {n * 1e3:7.1f} us {fl / n / 1e9:6.1f} TF(wino)  gain {a / n:.3f}  "
              f"A/A {a / a2:.3f}  equal {same}", flush=True)
    print("decoder launches of one step: " + "  ".join(f"{k} {v:.3f} ms" for k, v in zip(("rows0", "rows0'", "rows1"), step)))


if __name__ == "__main__":
    main()
