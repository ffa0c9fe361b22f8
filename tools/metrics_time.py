"""Kernel time of mhada_ssim_u8 and mhada_hist_u8 at 512^2 and 1080p (one frame), device events around
the launches, one process, interleaved rounds (every candidate timed once per round, in turn), median of
rounds.  Each kernel is timed twice per round ("again"); the difference of its two medians is the
measurement's own A-against-A resolution.  Prints the HBM bytes each call has to move (the frames once;
the partials and counts are a few KB) and the bandwidth that time implies.

Then the LPIPS distance head, mhada_lpips_layer, on the five tap shapes of VGG16 at 512^2 (B = 1, random
non-negative NHWC features), beside the same expression written with torch ops on the same device tensors
(lpips/lpips.py:139-147 on the NHWC storage), under the same protocol; the two results are compared first.

    python tools/metrics_time.py [rounds]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import ops

SHAPES = [("512^2", 1, 512, 512), ("1080p", 1, 1080, 1920)]


def dev_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median(ts):
    return sorted(ts)[len(ts) // 2]


LPIPS_TAPS = [("relu1_2", 512, 512, 64), ("relu2_2", 256, 256, 128), ("relu3_3", 128, 128, 256), ("relu4_3", 64, 64, 512),
              ("relu5_3", 32, 32, 512)]


def lpips_layer_torch(fa, fb, w):
    """normalize_tensor, the squared difference, the 1 x 1 conv and the spatial mean, as aten ops on NHWC."""
    na = fa / (torch.sqrt(torch.sum(fa ** 2, dim=-1, keepdim=True)) + 1e-10)
    nb = fb / (torch.sqrt(torch.sum(fb ** 2, dim=-1, keepdim=True)) + 1e-10)
    return (((na - nb) ** 2) * w).sum(dim=-1).mean(dim=(1, 2))


def time_lpips(rounds):
    for name, H, W, C in LPIPS_TAPS:
        g = torch.Generator().manual_seed(C + H)
        fa = torch.rand(1, H, W, C, generator=g).to("cuda")
        fb = torch.rand(1, H, W, C, generator=g).to("cuda")
        w = torch.rand(C, generator=g).to("cuda")
        nbytes = 2 * fa.numel() * 4
        head, aten = ops.lpips_layer(fa, fb, w), lpips_layer_torch(fa, fb, w)
        diff = abs(head.item() - aten.item()) / head.item()
        cand = {"lpips_layer": lambda: ops.lpips_layer(fa, fb, w), "lpips_layer (again)": lambda: ops.lpips_layer(fa, fb, w),
                "torch ops": lambda: lpips_layer_torch(fa, fb, w), "torch ops (again)": lambda: lpips_layer_torch(fa, fb, w)}
        for fn in cand.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        ts = {n: [] for n in cand}
        for _ in range(rounds):
            for n, fn in cand.items():
                ts[n].append(dev_ms(fn))
        print(f"{name}: 1 x {H} x {W} x {C} fp32 NHWC, two maps, {rounds} interleaved rounds; head {head.item():.9g}, "
              f"torch ops {aten.item():.9g} (rel diff {diff:.1e})", flush=True)
        for n in cand:
            t = median(ts[n])
            print(f"    {n:20s} {t * 1e3:9.1f} us  (min {min(ts[n]) * 1e3:.1f} max {max(ts[n]) * 1e3:.1f})  "
                  f"{nbytes / 1e6:.2f} MB read once, {nbytes / (t * 1e-3) / 1e9:.1f} GB/s of that")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    for name, B, H, W in SHAPES:
        g = torch.Generator().manual_seed(3)
        a = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to("cuda")
        b = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to("cuda")
        frame = B * H * W * 3
        cand = {"ssim_u8": (lambda: ops.ssim_u8(a, b), 2 * frame), "ssim_u8 (again)": (lambda: ops.ssim_u8(a, b), 2 * frame),
                "hist_u8": (lambda: ops.hist_u8(a), frame), "hist_u8 (again)": (lambda: ops.hist_u8(a), frame)}
        for fn, _ in cand.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        ts = {n: [] for n in cand}
        for _ in range(rounds):
            for n, (fn, _) in cand.items():
                ts[n].append(dev_ms(fn))
        print(f"{name}: {B} x {H} x {W} x 3 u8, {rounds} interleaved rounds", flush=True)
        for n, (_, nbytes) in cand.items():
            t = median(ts[n])
            print(f"    {n:18s} {t * 1e3:9.1f} us  (min {min(ts[n]) * 1e3:.1f} max {max(ts[n]) * 1e3:.1f})  "
                  f"{nbytes / 1e6:.2f} MB read, {nbytes / (t * 1e-3) / 1e9:.1f} GB/s")
    time_lpips(rounds)


if __name__ == "__main__":
    main()
