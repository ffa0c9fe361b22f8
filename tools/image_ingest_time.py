"""What preparing one image costs on the two routes, for a 3000 x 4000 photograph and a 1080 x 1920 frame resized
to 512 x 512 (PIL's BILINEAR, then toTensor255):

  (a) the device route: the full-size u8 image from pinned host memory to the device, then image.prepare
      (mhada_image_resize: the resized u8 image and the fp32 model input);
  (b) the host route it replaces: PIL.Image.resize + toTensor255 on the CPU, then the fp32 result from pinned
      host memory to the device.  Without PIL on the machine, tests/pil_resize_ref.py stands in for it and the
      output says so (that restatement is written for clarity, not speed).

One process, warm-up first, interleaved rounds, medians.  Route times are host-clock times that end in a device
synchronise; the kernels alone (ops.image_resize on an image already on the device) and a same-run torch copy, the
HBM yardstick of tools/bw_probe.py, are timed with device events.  Bytes are counted from the shapes.

    python tools/image_ingest_time.py [rounds]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd"), os.path.join(REPO, "tests")]

import numpy as np
import torch

from mhada_hip import image, ops

try:
    import PIL
    from PIL import Image
except ImportError:
    Image = None
    import pil_resize_ref

SHAPES = [("3000x4000 -> 512^2", 3000, 4000, 512, 512), ("1080x1920 -> 512^2", 1080, 1920, 512, 512)]


def dev_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def host_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    dev = torch.device("cuda", torch.cuda.current_device())
    big = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    big2 = torch.empty_like(big)
    for _ in range(3):
        big2.copy_(big)
    copy_us = median([dev_us(lambda: big2.copy_(big)) for _ in range(rounds)])
    hbm = 2 * big.numel() / copy_us / 1e6
    print(f"torch copy 2 x 512 MiB: {copy_us:.1f} us = {hbm:.2f} TB/s (the same-run HBM yardstick)", flush=True)
    del big, big2
    print("host resize: " + (f"Pillow {PIL.__version__}" if Image is not None
                             else "tests/pil_resize_ref.py (PIL is not installed: a stand-in)"))
    for name, H, W, Ho, Wo in SHAPES:
        x = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        pin_src = torch.from_numpy(x).pin_memory()
        pin_f32 = torch.empty(3, Ho, Wo, dtype=torch.float32).pin_memory()
        on_dev = pin_src.to(dev)
        pil = Image.fromarray(x) if Image is not None else None

        def host_resize():
            if pil is not None:
                return np.array(pil.resize((Wo, Ho), Image.BILINEAR))
            return pil_resize_ref.resize(x, Ho, Wo)

        def route_a():
            return image.prepare(pin_src.to(dev, non_blocking=True), (Wo, Ho))

        def route_b():
            r = torch.from_numpy(np.ascontiguousarray(host_resize()))
            pin_f32.copy_((r.permute(2, 0, 1).float() / 255.0) * 255.0)  # toTensor255
            return pin_f32.to(dev, non_blocking=True)

        def upload():
            return pin_src.to(dev, non_blocking=True)

        def kernels():
            return ops.image_resize(on_dev, (Ho, Wo))

        u8, f32 = route_a()
        assert np.array_equal(u8.cpu().numpy(), host_resize()), "the routes disagree"
        assert torch.equal(f32.cpu(), route_b().cpu()), "the routes disagree"
        host = {"(a) H2D u8 + image.prepare": route_a, "(a) again": route_a, "    of which H2D of the u8 image": upload,
                "(b) host resize + toTensor255 + H2D": route_b}
        for fn in list(host.values()) + [kernels]:  # warm-up
            fn()
        th, tk = {n: [] for n in host}, []
        for _ in range(rounds):
            for n, fn in host.items():
                th[n].append(host_us(fn))
            tk.append(dev_us(kernels))
        src, work = 3 * H * W, (3 * H * Wo if (Wo != W and Ho != H) else 0)
        out = 3 * Ho * Wo + 12 * Ho * Wo
        cx, cy = ops.pil_bilinear_tables(W, Wo)[0], ops.pil_bilinear_tables(H, Ho)[0]
        tables = (cx.size + cy.size) * 4 + 8 * (Wo + Ho)
        moved = src + 2 * work + out + tables
        k = median(tk)
        print(f"{name}: {rounds} interleaved rounds, taps {cx.shape[1]} x {cy.shape[1]}")
        for n in host:
            print(f"  {n:38s} {median(th[n]) / 1e3:9.3f} ms  (min {min(th[n]) / 1e3:.3f} max {max(th[n]) / 1e3:.3f})")
        print(f"  {'kernels alone (device events)':38s} {k:9.1f} us  (min {min(tk):.1f} max {max(tk):.1f})")
        print(f"  bytes: source {src / 1e6:.2f} MB read once, workspace {work / 1e6:.2f} MB written and read, outputs "
              f"{out / 1e6:.2f} MB, tables {tables / 1e3:.1f} kB: {moved / 1e6:.2f} MB in all = {moved / k / 1e6:.3f} TB/s "
              f"= {100 * moved / k / 1e6 / hbm:.1f} % of the torch copy rate", flush=True)


if __name__ == "__main__":
    main()
