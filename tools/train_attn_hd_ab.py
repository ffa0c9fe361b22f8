"""A/B of training a 4- / 16-head MHAda block (head_dim 128 / 32) on the HIP attention kernels
(autograd_path.TRAIN_ATTN = "hip": csrc/attn_train.hip at D = 32 | 128, the grouped head projection) against the
per-head aten loop ("torch": what these widths ran before the kernels existed — the baseline).

One process, interleaved rounds: every configuration runs once per round, block forward + backward,
timed with device events around the whole call; the median and the spread over the rounds are
printed, and the peak bytes allocated above what was live before the call (one extra run each).
Shapes: 256^2 images (Nc = Ns = 1024 tokens, B = 2) and 512^2 (4096 tokens, B = 1).  Beside them the
8-head block on the 64-wide fp32-MFMA forms the new kernels are modelled on (TRAIN_FWD_S3 and
TRAIN_DQ_S3 off, no dS spill; "r1" also turns TRAIN_FWD_VT off: the round-1 forward), so the cost
per FLOP of the D-wide kernels can be read against their 64-wide model.

    python tools/train_attn_hd_ab.py [--rounds 7] [--errsweep]

--errsweep: instead, the error of MHAdaAttnFn (forward + backward) against fp64 autograd over four
seeds at scale 1.5 (logit std 12.7 at D = 32, 25 at D = 128 — above what the tests assert), with
the reference's fp32 autograd on the device as the yardstick: kernel error, aten error, ratio.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

import network
from mhada_hip import autograd_path, ops
from mhada_hip.recipe import load_recipe


def ref(q, k, v, x):
    a = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    m = a @ v
    e2 = a @ (v * v)
    return torch.sqrt((e2 - m * m).clamp(min=1e-6)) * x + m


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def errsweep():
    BH, Nc, Ns, scale = 2, 256, 129, 1.5
    for D in (32, 128):
        worst = {"kernel": 0.0, "aten": 0.0, "ratio": 0.0}
        for seed in range(4):
            g = torch.Generator().manual_seed(Nc * 7 + Ns + D + 1000 * seed)
            q = torch.randn(BH, Nc, D, generator=g) * scale
            k = torch.randn(BH, Ns, D, generator=g) * scale
            v = torch.randn(BH, Ns, D, generator=g) * 3
            v = v - v.mean(dim=1, keepdim=True)
            x = torch.randn(BH, Nc, D, generator=g)
            dout = torch.randn(BH, Nc, D, generator=g)
            ts = [t.double().requires_grad_() for t in (q, k, v, x)]
            r = ref(*ts)
            r.backward(dout.double())
            fs = [t.cuda().requires_grad_() for t in (q, k, v, x)]
            o32 = ref(*fs)
            o32.backward(dout.cuda())
            gs = [t.cuda().requires_grad_() for t in (q, k, v, x)]
            out = autograd_path.MHAdaAttnFn.apply(*gs)
            out.backward(dout.cuda())
            rows = [("out", rel(out.detach().double().cpu(), r.detach()), rel(o32.detach().double().cpu(), r.detach()))]
            rows += [("d" + n, rel(a.grad.double().cpu(), b.grad), rel(c.grad.double().cpu(), b.grad))
                     for n, a, b, c in zip("qkvx", gs, ts, fs)]
            line = f"D {D:3d} BH {BH} Nc {Nc} Ns {Ns} scale {scale} seed {seed} |"
            for n, e, e32 in rows:
                line += f" {n} kernel {e:.1e} aten {e32:.1e} ratio {e / e32:.2f} |"
                worst["kernel"], worst["aten"] = max(worst["kernel"], e), max(worst["aten"], e32)
                worst["ratio"] = max(worst["ratio"], e / e32)
            print(line, flush=True)
        print(f"D {D:3d} worst over seeds and tensors: kernel {worst['kernel']:.1e} aten {worst['aten']:.1e} "
              f"kernel / aten {worst['ratio']:.2f}", flush=True)


class Config:
    def __init__(self, name, heads, attn, knobs=None):
        self.name, self.heads, self.attn, self.knobs = name, heads, attn, knobs or {}

    def run(self, blk, fc, fs, fcs, dout):
        saved = {k: getattr(ops, k) for k in self.knobs}
        autograd_path.TRAIN_ATTN = self.attn
        for k, val in self.knobs.items():
            setattr(ops, k, val)
        try:
            for t in (fc, fs, fcs, *blk.parameters()):
                t.grad = None
            autograd_path.block_forward(blk, fc, fs, fcs).backward(dout)
        finally:
            autograd_path.TRAIN_ATTN = "hip"
            for k, val in saved.items():
                setattr(ops, k, val)


F32_FORMS = dict(TRAIN_FWD_S3=False, TRAIN_DQ_S3=False, DS_SPILL_BYTES=0)
CONFIGS = [Config("h4  hip", 4, "hip"), Config("h4  torch", 4, "torch"),
           Config("h16 hip", 16, "hip"), Config("h16 torch", 16, "torch"),
           Config("h8  f32-mfma (vt fwd)", 8, "hip", F32_FORMS),
           Config("h8  f32-mfma (r1 fwd)", 8, "hip", dict(F32_FORMS, TRAIN_FWD_VT=False))]


def ab(rounds):
    blocks = {h: load_recipe(network.AdaAttnTransformerMultiHead(num_heads=h), "ada").cuda().adaAttnHead[0]
              for h in (4, 8, 16)}
    for label, B, side in (("256^2 B2", 2, 32), ("512^2 B1", 1, 64)):
        g = torch.Generator(device="cuda").manual_seed(side)
        fc, fs, fcs = ((torch.randn(B, 512, side, side, device="cuda", generator=g) * 2).requires_grad_()
                       for _ in range(3))
        dout = torch.randn(B, 512, side, side, device="cuda", generator=g)
        times = {c.name: [] for c in CONFIGS}
        peaks = {}
        for c in CONFIGS:  # warm-up, and the peak of one run
            c.run(blocks[c.heads], fc, fs, fcs, dout)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            live = torch.cuda.memory_allocated()
            c.run(blocks[c.heads], fc, fs, fcs, dout)
            torch.cuda.synchronize()
            peaks[c.name] = torch.cuda.max_memory_allocated() - live
        for _ in range(rounds):
            for c in CONFIGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c.run(blocks[c.heads], fc, fs, fcs, dout)
                e1.record()
                torch.cuda.synchronize()
                times[c.name].append(e0.elapsed_time(e1))
        n = side * side
        print(f"{label}: Nc = Ns = {n}, block forward + backward, {rounds} interleaved rounds", flush=True)
        for c in CONFIGS:
            t = times[c.name]
            print(f"  {c.name:24s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                  f"peak {peaks[c.name] / 2 ** 20:9.1f} MiB", flush=True)
        for h in (4, 16):
            a, b = statistics.median(times[f"h{h:<2d} hip"]), statistics.median(times[f"h{h:<2d} torch"])
            print(f"  h{h}: hip / torch time {a / b:.3f}, peak {peaks[f'h{h:<2d} hip'] / peaks[f'h{h:<2d} torch']:.3f}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--errsweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_attn_hd_ab.py needs the GPU: there is nothing to measure on the CPU")
    if a.errsweep:
        errsweep()
    else:
        ab(a.rounds)


if __name__ == "__main__":
    main()
