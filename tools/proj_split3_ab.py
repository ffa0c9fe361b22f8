"""The 512 x 512 out-projection and its producers, fp32 form against plane form, in one process: interleaved
rounds, median per call, at the 512^2 batch-8 shapes (M = 32768 tokens).

  gemm      ops.linear on the fp32 MFMA against ops.linear_split3 (gemm_s3_kernel), N = K0 = 512, with the
            residual (the ViT out-projection) and without (the MHAda out_conv)
  vit_attn  the batch-axis attention (L = 8, ntok = 4096) with fp32 output against plane output
  attn_s3   the SPLIT3 MHAda attention (B = 8, H = 8, Nc = Ns = 4096) with fp32 output against plane output
Each pair is also timed A against A (the fp32 form against its own second copy): that difference is the
resolution of the comparison.

    python tools/proj_split3_ab.py [rounds] [iters]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import ops


def ab(name, calls, rounds, iters):
    """calls: {label: fn}; interleaved rounds of iters launches each, median us per launch."""
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / iters * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    base = next(iter(calls))
    print(f"{name:14s} " + "   ".join(f"{k} {med[k]:7.1f} us (min {min(times[k]):.1f} max {max(times[k]):.1f}) "
                                      f"x{med[k] / med[base]:.3f}" for k in calls), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    torch.manual_seed(0)
    dev = "cuda"
    M, C, heads = 32768, 512, 8
    x = torch.randn(M, C, device=dev)
    w = torch.randn(C, C, device=dev) / C ** 0.5
    b = torch.randn(C, device=dev)
    r = torch.randn(M, C, device=dev)
    pl, w6 = ops.split3_rows(x), ops.split3_weight(w)
    for res in (r, None):
        ab("gemm res" if res is not None else "gemm plain",
           {"f32": lambda: ops.linear(x, w, b, torch.float32, residual=res),
            "f32'": lambda: ops.linear(x, w, b, torch.float32, residual=res),
            "split3": lambda: ops.linear_split3(pl, w6, b, torch.float32, residual=res)}, rounds, iters)
    L, ntok = 8, 4096
    qkv = torch.randn(L, ntok, 3 * C, device=dev)
    ab("vit_attn", {"f32": lambda: ops.vit_batch_attn(qkv, L, ntok, heads),
                    "f32'": lambda: ops.vit_batch_attn(qkv, L, ntok, heads),
                    "planes": lambda: ops.vit_batch_attn_split3(qkv, L, ntok, heads)}, rounds, iters)
    B, N = 8, 4096
    q = torch.randn(B, heads, N, 64, device=dev) * 0.5
    kv = torch.randn(B, heads, N, 128, device=dev) * 0.5
    fcs = torch.randn(B, N, C, device=dev)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = torch.randn(B, C, device=dev)
    img = ops.split3_kv(kv, ops.transpose_v(kv))
    ab("attn_s3", {"f32": lambda: ops.attn_split3(q, img, N, fcs, mu, rs, vmu),
                   "f32'": lambda: ops.attn_split3(q, img, N, fcs, mu, rs, vmu),
                   "planes": lambda: ops.attn_split3_planes(q, img, N, fcs, mu, rs, vmu)}, rounds, max(iters // 4, 3))


if __name__ == "__main__":
    main()
