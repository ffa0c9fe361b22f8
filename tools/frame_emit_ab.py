"""A/B of the three routes from the decoder's last layer to a cv2-ready u8 BGR frame on the host, at 1080p B1
and 512^2 B8, fp32 and bf16 compute (Cin = 64, the decoder's last layer):

  (a) the route before mhada_frame_emit: mhada_conv3x3_out3(clamp255) -> fp32 download into pinned memory ->
      numpy permute / astype(uint8) / channel flip on the host;
  (b) mhada_conv3x3_out3(clamp255) + mhada_frame_emit -> u8 download into pinned memory;
  (c) the fused mhada_conv3x3_out3_u8 -> u8 download into pinned memory.

One process, interleaved rounds (every candidate timed once per round, in turn), median of rounds.  Kernel time
(device events around the launches) and frame-to-host time (host clock from before the launch until the numpy
frame exists, the stream drained first) are reported separately.  The fp32 out3 kernel is timed twice per round
("again"); the difference of its two medians is the measurement's own A-against-A resolution, and the fused
kernel passes when it does not exceed the same-run out3 time by more than that spread.

    python tools/frame_emit_ab.py [rounds]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import numpy as np
import torch

from mhada_hip import ops

SHAPES = [("1080p B1", 1, 1080, 1920), ("512^2 B8", 8, 512, 512)]


def dev_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    for name, B, H, W in SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            g = torch.Generator().manual_seed(3)
            x = (torch.rand(B, H, W, 64, generator=g) - 0.5).to("cuda").to(dt)
            w = (torch.randn(9, 64, 3, generator=g) * (250.0 / 48.0 ** 0.5)).to("cuda")
            b = torch.tensor([120.0, 127.5, 135.0], device="cuda")
            pin32 = torch.empty(B, 3, H, W, dtype=torch.float32, pin_memory=True)
            pin8 = torch.empty(B, H, W, 3, dtype=torch.uint8, pin_memory=True)
            u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
            y32 = ops.conv3x3_out3(x, w, b, clamp255=True)

            def route_a():
                pin32.copy_(ops.conv3x3_out3(x, w, b, clamp255=True), non_blocking=True)
                torch.cuda.current_stream().synchronize()
                return np.ascontiguousarray(pin32.permute(0, 2, 3, 1).numpy().astype(np.uint8)[..., ::-1])

            def route_b():
                pin8.copy_(ops.frame_emit(ops.conv3x3_out3(x, w, b, clamp255=True), out=u8), non_blocking=True)
                torch.cuda.current_stream().synchronize()
                return pin8.numpy()

            def route_c():
                pin8.copy_(ops.conv3x3_out3_u8(x, w, b, out=u8), non_blocking=True)
                torch.cuda.current_stream().synchronize()
                return pin8.numpy()

            fa = route_a()
            assert np.array_equal(fa, route_b()) and np.array_equal(fa, route_c()), "the routes disagree"
            kern = {
                "out3 (fp32 frame)": lambda: ops.conv3x3_out3(x, w, b, clamp255=True),
                "out3 (again)": lambda: ops.conv3x3_out3(x, w, b, clamp255=True),
                "frame_emit": lambda: ops.frame_emit(y32, out=u8),
                "out3 + frame_emit": lambda: ops.frame_emit(ops.conv3x3_out3(x, w, b, clamp255=True), out=u8),
                "out3_u8 (fused)": lambda: ops.conv3x3_out3_u8(x, w, b, out=u8),
            }
            host = {"(a) out3 -> fp32 D2H -> numpy": route_a, "(a) again": route_a,
                    "(b) out3 + emit -> u8 D2H": route_b, "(c) out3_u8 -> u8 D2H": route_c}
            for fn in list(kern.values()) + list(host.values()):  # warm-up
                fn()
            torch.cuda.synchronize()
            tk, th = {n: [] for n in kern}, {n: [] for n in host}
            for _ in range(rounds):
                for n, fn in kern.items():
                    tk[n].append(dev_ms(fn))
                for n, fn in host.items():
                    th[n].append(host_ms(fn))
            mk, mh = {n: median(t) for n, t in tk.items()}, {n: median(t) for n, t in th.items()}
            print(f"{name} {str(dt).split('.')[-1]}: {B} x {H} x {W}, Cin 64, {rounds} interleaved rounds", flush=True)
            print("  kernel time (device events)")
            for n, t in mk.items():
                print(f"    {n:32s} {t * 1e3:9.1f} us  (min {min(tk[n]) * 1e3:.1f} max {max(tk[n]) * 1e3:.1f})")
            a, a2, c = mk["out3 (fp32 frame)"], mk["out3 (again)"], mk["out3_u8 (fused)"]
            spread = abs(a - a2)
            ok = c <= min(a, a2) + spread
            print(f"    A-against-A spread {spread * 1e3:.1f} us ({spread / min(a, a2) * 100:.2f} %); fused - out3 = "
                  f"{(c - min(a, a2)) * 1e3:+.1f} us: {'PASS' if ok else 'FAIL'} (fused <= out3 + spread)")
            print("  frame-to-host time (host clock, launch to numpy frame)")
            for n, t in mh.items():
                print(f"    {n:32s} {t:9.3f} ms  (min {min(th[n]):.3f} max {max(th[n]):.3f})")
            ha, ha2 = mh["(a) out3 -> fp32 D2H -> numpy"], mh["(a) again"]
            print(f"    A-against-A spread {abs(ha - ha2):.3f} ms; (a) / (b) = x{min(ha, ha2) / mh['(b) out3 + emit -> u8 D2H']:.2f}, "
                  f"(a) / (c) = x{min(ha, ha2) / mh['(c) out3_u8 -> u8 D2H']:.2f}", flush=True)


if __name__ == "__main__":
    main()
