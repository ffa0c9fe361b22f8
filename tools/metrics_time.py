"""Kernel time of mhada_ssim_u8 and mhada_hist_u8 at 512^2 and 1080p (one frame), device events around
the launches, one process, interleaved rounds (every candidate timed once per round, in turn), median of
rounds.  Each kernel is timed twice per round ("again"); the difference of its two medians is the
measurement's own A-against-A resolution.  Prints the HBM bytes each call has to move (the frames once;
the partials and counts are a few KB) and the bandwidth that time implies.

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


if __name__ == "__main__":
    main()
