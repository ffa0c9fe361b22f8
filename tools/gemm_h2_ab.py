"""HALF2 against SPLIT3 on the LayerNorm-fed ViT GEMMs in one process: the 512^2 batch-8 shapes
(M = 32768 tokens) QKV and MLP1 (ReLU, plane output), each with its LayerNorm (the plane writer differs too),
interleaved rounds, median per call, and the relative difference of the two results.

    python tools/gemm_h2_ab.py [rounds] [iters]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import ops


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    M, K0 = 32768, 512
    torch.manual_seed(0)
    for name, N, planes, relu in (("qkv", 1536, False, False), ("mlp1", 2048, True, True)):
        x = torch.randn(M, K0, device="cuda") * 2 + 0.3
        g = torch.randn(K0, device="cuda").abs() + 0.5
        be = torch.randn(K0, device="cuda") * 0.3
        w = torch.randn(N, K0, device="cuda") / K0 ** 0.5
        b = torch.randn(N, device="cuda")
        w6 = ops.split3_weight(w)
        h = ops.half2_prepare(g, be, w)
        p3 = ops.layernorm_split3(x, g, be, 1e-6)
        p2 = ops.layernorm_half2(x, g, be, 1e-6, h["s_a"])
        forms = {
            "s3": (lambda: ops.layernorm_split3(x, g, be, 1e-6),
                   lambda: ops.linear_split3(p3, w6, b, torch.float32, relu=relu, out_planes=planes)),
            "h2": (lambda: ops.layernorm_half2(x, g, be, 1e-6, h["s_a"]),
                   lambda: ops.linear_half2(p2, h["w2"], h["cs"], b, torch.float32, relu=relu, out_planes=planes)),
        }
        out = {k: f[1]() for k, f in forms.items()}
        if planes:
            out = {k: v.double().sum(0) for k, v in out.items()}
        torch.cuda.synchronize()
        t = {(k, i): [] for k in forms for i in (0, 1)}
        for _ in range(rounds):
            for k, f in forms.items():
                for i in (0, 1):
                    t[k, i].append(timed(f[i], iters))
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in t.items()}
        lo = {k: min(v) * 1e3 for k, v in t.items()}
        d = (out["h2"].double() - out["s3"].double()).norm() / out["s3"].double().norm()
        fl = 2 * M * N * K0
        print(f"{name:5s} M={M} N={N} K0={K0}: gemm s3 {med['s3', 1]:6.1f} us ({6 * fl / med['s3', 1] / 1e6:6.1f} TF issued)  "
              f"h2 {med['h2', 1]:6.1f} us ({3 * fl / med['h2', 1] / 1e6:6.1f} TF issued)  h2/s3 {med['h2', 1] / med['s3', 1]:.3f}  "
              f"min s3 {lo['s3', 1]:.1f} h2 {lo['h2', 1]:.1f} | layernorm s3 {med['s3', 0]:5.1f} us h2 {med['h2', 0]:5.1f} us | "
              f"rel diff {d:.2e}")


if __name__ == "__main__":
    main()
