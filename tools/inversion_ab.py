"""A/B of one feature-inversion iteration (forward, backward, Adam step on the image) at the reference
scripts' own size: 512 x 512, B = 1, 3 layers, 8 heads, recipe weights, frozen models.

  (a) visual_vit.py:97-112    — the content ViT alone;
  (b) visual_mhada.py:112-127 — the content ViT and the six MHAda blocks, style features from a
      no-grad call.

Routes of the grad-carrying image: autograd_path.VIT_INPUT_GRAD = "hip" (the HIP training kernels,
image gradient from mhada_patch_embed_dgrad) against "torch" (the aten modules — what such a run took
before the kernel existed).  For (b) also the dQ-only attention backward (autograd_path.ATTN_DQ_ONLY)
against the full backward.  Beside them the kernel alone against
F.conv_transpose2d(dy_nchw, weight, stride=8).

One process, interleaved rounds after a warm-up: every configuration runs once per round, timed with
device events around the whole iteration (synchronised); the median and the spread over the rounds are
printed.

    python tools/inversion_ab.py [--rounds 9] [--size 512]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch
import torch.nn.functional as F

import network
from mhada_hip import autograd_path, ops
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"


def frozen(m):
    return m.to(DEV).eval().requires_grad_(False)


def blocks(ada, fc, fs):
    fcs = fc[0]
    for i in range(ada.num_layers):
        fcs = ada.adaAttnHead[2 * i](fc[i], fs[i], fcs)
        fcs = ada.adaAttnHead[2 * i + 1](fcs, fs[i], fcs)
    return fcs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def report(name, ts):
    print(f"{name:44s} median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  (n = {len(ts)})",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("inversion_ab.py measures on the GPU; no device found")
    S = args.size
    vit_c = frozen(load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c"))
    vit_s = frozen(load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s"))
    ada = frozen(load_recipe(network.AdaAttnTransformerMultiHead(), "ada"))
    content, style = seeded_image(1, S, S, 101).to(DEV), seeded_image(1, S, S, 102).to(DEV)
    with torch.no_grad():
        target = vit_c(content)
        fs = vit_s(style)
        target_ada = blocks(ada, target, fs)

    def make(loss_fn, route, dq_only=True):
        recon = torch.randn(1, 3, S, S, generator=torch.Generator().manual_seed(7)).to(DEV).requires_grad_(True)
        opt = torch.optim.Adam([recon], lr=0.5)

        def step():
            saved = autograd_path.ATTN_DQ_ONLY
            autograd_path.ATTN_DQ_ONLY = dq_only
            try:
                with autograd_path.vit_input_grad(route):
                    opt.zero_grad()
                    loss_fn(recon).backward()
                    opt.step()
            finally:
                autograd_path.ATTN_DQ_ONLY = saved
        return step

    vit_loss = lambda x: sum(F.mse_loss(f, t) for f, t in zip(vit_c(x), target))  # noqa: E731
    ada_loss = lambda x: F.mse_loss(blocks(ada, vit_c(x), fs), target_ada)  # noqa: E731
    configs = [
        ("(a) ViT, image grad on HIP", make(vit_loss, "hip")),
        ("(a) ViT, image grad on aten", make(vit_loss, "torch")),
        ("(b) ViT + MHAda, HIP, dQ-only backward", make(ada_loss, "hip", True)),
        ("(b) ViT + MHAda, HIP, full backward", make(ada_loss, "hip", False)),
        ("(b) ViT + MHAda, ViT on aten, dQ-only", make(ada_loss, "torch", True)),
        ("(b) ViT + MHAda, ViT on aten, full backward", make(ada_loss, "torch", False)),
    ]
    # the kernel alone against aten's transposed conv
    N = (S // 8) ** 2
    dy = torch.randn(1, N, 512, generator=torch.Generator().manual_seed(1)).to(DEV)
    w = vit_c.patch_embedding.conv_proj.weight.detach().contiguous()
    dy_nchw = dy.view(1, S // 8, S // 8, 512).permute(0, 3, 1, 2).contiguous()
    out = torch.empty(1, 3, S, S, device=DEV)
    reps = 20
    configs += [
        (f"kernel: mhada_patch_embed_dgrad x{reps}", lambda: [ops.patch_embed_dgrad(dy, w, S, S, out=out) for _ in range(reps)]),
        (f"kernel: F.conv_transpose2d x{reps}", lambda: [F.conv_transpose2d(dy_nchw, w, stride=8) for _ in range(reps)]),
    ]
    print(f"inversion iteration at {S} x {S}, B = 1, 3 layers, 8 heads; device {torch.cuda.get_device_name(0)}; "
          f"{args.rounds} interleaved rounds after 3 warm-up rounds", flush=True)
    for _ in range(3):
        for _, fn in configs:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, fn in configs:
            times[name].append(timed(fn))
    for name, _ in configs:
        ts = times[name]
        if name.startswith("kernel"):
            ts = [t / reps for t in ts]
        report(name + (" (per call)" if name.startswith("kernel") else ""), ts)
    a = ops.patch_embed_dgrad(dy, w, S, S)
    b = F.conv_transpose2d(dy_nchw, w, stride=8)
    print(f"kernel vs aten conv_transpose2d: max |diff| / max |ref| = {((a - b).abs().max() / b.abs().max()).item():.2e}")
    print(f"counters: BWD_PATH_COUNTS {ops.BWD_PATH_COUNTS} DQ_ONLY_COUNTS {ops.DQ_ONLY_COUNTS}")


if __name__ == "__main__":
    main()
