"""Kernel time of mhada_ssim_u8 and mhada_hist_u8 at 512^2 and 1080p (one frame), device events around
the launches, one process, interleaved rounds (every candidate timed once per round, in turn), median of
rounds.  Each kernel is timed twice per round ("again"); the difference of its two medians is the
measurement's own A-against-A resolution.  Prints the HBM bytes each call has to move (the frames once;
the partials and counts are a few KB) and the bandwidth that time implies.

Then the LPIPS distance head, mhada_lpips_layer, on the five tap shapes of VGG16 at 512^2 (B = 1, random
non-negative NHWC features), beside the same expression written with torch ops on the same device tensors
(lpips/lpips.py:139-147 on the NHWC storage), under the same protocol; the two results are compared first.

Then SIFID at 512^2 (B = 1, random weights: the time does not depend on the values), dims 2048 and 64: the
HIP InceptionV3 trunk alone (device events), the same modules run by aten on the device (informative; "not
measured" if aten's conv fails here), and the whole metrics.sifid call of two frames, trunk passes, moment
kernels, copies and the host's SVD / eigenvalues included (wall clock around a synchronised call).

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


def time_sifid(rounds):
    import time

    import network
    from mhada_hip import metrics
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).to("cuda")
    b = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).to("cuda")
    x = torch.rand(1, 3, 512, 512, generator=g).to("cuda")
    for dims, blk in ((2048, 3), (64, 0)):
        inc = network.InceptionV3([blk]).to("cuda")

        def aten():
            y = 2 * x - 1
            for block in inc.blocks:
                y = block(y)
            return y

        cand = {"HIP trunk": lambda: inc(x), "HIP trunk (again)": lambda: inc(x)}
        try:
            with torch.no_grad():
                aten()
            torch.cuda.synchronize()
            cand.update({"aten trunk": aten, "aten trunk (again)": aten})
        except Exception as e:  # informative only
            print(f"SIFID dims {dims}: aten trunk not measured ({type(e).__name__})")
        ts = {n: [] for n in cand}
        wall = []
        with torch.no_grad():
            for fn in cand.values():  # warm-up
                fn()
            metrics.sifid(a, b, inc, dims=dims)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for n, fn in cand.items():
                    ts[n].append(dev_ms(fn))
                t0 = time.perf_counter()
                metrics.sifid(a, b, inc, dims=dims)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
        print(f"SIFID dims {dims}: 1 x 3 x 512 x 512, {rounds} interleaved rounds", flush=True)
        for n in cand:
            print(f"    {n:20s} {median(ts[n]):9.3f} ms  (min {min(ts[n]):.3f} max {max(ts[n]):.3f})")
        print(f"    {'metrics.sifid (wall)':20s} {median(wall):9.3f} ms  (min {min(wall):.3f} max {max(wall):.3f})  two frames, "
              "host finaliser included")


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
    time_sifid(rounds)


if __name__ == "__main__":
    main()
