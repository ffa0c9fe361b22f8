"""A/B of the bf16 training attention (autograd_path.TRAIN_ATTN = "bf16") against the default fp32 path:
one 8-head AdaAttnMultiHead block forward + backward at 256^2 B2 (Nc = Ns = 1024) and 512^2 B1 (4096),
both modes in one process in interleaved rounds, device events, median and range, peak bytes; with
--step, one Trainer.step at 512^2 B8 in each mode.

    python tools/train_attn_bf16_ab.py [--rounds 7] [--step]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mhada-style-transfer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import network  # noqa: E402
from mhada_hip import autograd_path, ops  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402
from mhada_hip.train import Trainer  # noqa: E402

MODES = ("hip", "bf16")


def block_once(blk, fc, fs, fcs, dout, mode):
    for t in (fc, fs, fcs, *blk.parameters()):
        t.grad = None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    e0.record()
    with autograd_path.train_attn(mode):
        y = autograd_path.block_forward(blk, fc, fs, fcs)
    y.backward(dout)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - live


def block_ab(B, side, rounds):
    blk = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").cuda().adaAttnHead[0]
    g = torch.Generator(device="cuda").manual_seed(side)
    fc, fs, fcs = ((torch.randn(B, 512, side, side, device="cuda", generator=g) * 2).requires_grad_() for _ in range(3))
    dout = torch.randn(B, 512, side, side, device="cuda", generator=g)
    ms, peak = {m: [] for m in MODES}, {}
    for r in range(rounds + 2):  # two warm-up rounds
        for m in MODES if r % 2 == 0 else MODES[::-1]:
            before = dict(ops.BF16_TRAIN_COUNTS)
            t, pk = block_once(blk, fc, fs, fcs, dout, m)
            assert (ops.BF16_TRAIN_COUNTS != before) == (m == "bf16")
            if r >= 2:
                ms[m].append(t)
                peak[m] = pk
    for m in MODES:
        print(f"block B{B} Nc=Ns={side * side} {m:5s}: median {statistics.median(ms[m]):8.3f} ms "
              f"(min {min(ms[m]):.3f} max {max(ms[m]):.3f}, n={len(ms[m])}) peak {peak[m] / 2 ** 20:.1f} MiB")
    print(f"block B{B} Nc=Ns={side * side} fp32 / bf16 = {statistics.median(ms['hip']) / statistics.median(ms['bf16']):.2f}x")


def step_ab(rounds):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_train_cpu import build
    c, s = seeded_image(8, 512, 512, 1).cuda(), seeded_image(8, 512, 512, 2).cuda()
    trs = {"fp32": Trainer(*build("cuda")), "bf16": Trainer(*build("cuda"), attn_precision="bf16")}
    ms = {m: [] for m in trs}
    for r in range(rounds + 1):
        for m, tr in trs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.step(c, s)
            e1.record()
            torch.cuda.synchronize()
            if r >= 1:
                ms[m].append(e0.elapsed_time(e1))
    for m in trs:
        print(f"Trainer.step 512^2 B8 {m}: median {statistics.median(ms[m]):.1f} ms (min {min(ms[m]):.1f} max {max(ms[m]):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    block_ab(2, 32, a.rounds)
    block_ab(1, 64, a.rounds)
    if a.step:
        step_ab(3)
