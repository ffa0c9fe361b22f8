"""SPLIT3 GEMM term order A/B in one process: tuning gemm_s3_order = 0 (six K-tiles per chunk, both
operands staged for each) against 1 (each plane staged once per chunk, gemm_s3_kernel), interleaved
rounds, median per call, on the 512^2 batch-8 ViT shapes (M = 32768 tokens): QKV, MLP1 with plane
output, MLP2 with a residual.

    python tools/gemm_s3_ab.py [rounds] [iters]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import _lib, ops


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    M = 32768
    torch.manual_seed(0)
    for name, N, K0, planes, res, relu in (("qkv", 1536, 512, False, False, False),
                                           ("mlp1", 2048, 512, True, False, True),
                                           ("mlp2", 512, 2048, False, True, False)):
        x = torch.randn(M, K0, device="cuda")
        w = torch.randn(N, K0, device="cuda") / K0 ** 0.5
        b = torch.randn(N, device="cuda")
        r = torch.randn(M, N, device="cuda") if res else None
        pl, w6 = ops.split3_rows(x), ops.split3_weight(w)
        call = lambda: ops.linear_split3(pl, w6, b, torch.float32, residual=r, relu=relu, out_planes=planes)  # noqa: E731
        out, times = {}, {0: [], 1: []}
        for knob in (0, 1):
            with _lib.tuning(gemm_s3_order=knob):
                out[knob] = call().double().sum(0) if planes else call()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for knob in (0, 1):
                with _lib.tuning(gemm_s3_order=knob):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(iters):
                        call()
                    e.record()
                    torch.cuda.synchronize()
                    times[knob].append(s.elapsed_time(e) / iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        fl = 6 * 2 * M * N * K0  # bf16 MFMA FLOP issued
        d = (out[1].double() - out[0].double()).norm() / out[0].double().norm()
        print(f"split3 {name:5s} M={M} N={N:5d} K0={K0:5d}: old {med[0] * 1e3:7.1f} us {fl / med[0] / 1e9:7.1f} TF   "
              f"new {med[1] * 1e3:7.1f} us {fl / med[1] / 1e9:7.1f} TF   new/old {med[1] / med[0]:.3f}   "
              f"min old {min(times[0]) * 1e3:.1f} new {min(times[1]) * 1e3:.1f}   rel diff {d:.2e}")


if __name__ == "__main__":
    main()
