"""A/B of the single-head AdaAttN attention at head width 512: the bf16 kernel mhada_attn_wide
(csrc/attn_wide.hip) against the only other route at this width, the fp32 mhada_loss_attn at d_qk = d_v = 512,
with the 8-head bf16 mhada_attn on the same token counts as a yardstick (the same algorithmic
6 Nc Ns C B FLOP at head width 64).  One process, interleaved rounds (every candidate timed once per round, in
turn), median of rounds; mhada_attn_wide is timed twice per round and the difference of its two medians is
reported as the measurement's own A-against-A resolution.  Rates: TF/s of the algorithmic FLOP and their
fraction of 2.5 PF (the dense bf16 peak).

    python tools/attn_wide_ab.py [rounds]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import _lib, ops

SHAPES = [("512^2 B8", 8, 4096, 4096), ("1024^2 B4", 4, 16384, 16384)]


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    torch.manual_seed(0)
    C = 512
    sc = 0.5 * (64.0 / C) ** 0.25
    for name, B, nc, ns in SHAPES:
        q = torch.randn(B, nc, C, device="cuda") * sc
        k = torch.randn(B, ns, C, device="cuda") * sc
        v = torch.randn(B, ns, C, device="cuda") * sc
        fcs = torch.randn(B, nc, C, device="cuda")
        mu, rs = ops.instnorm_stats(fcs)
        vmu = torch.zeros(B, C, device="cuda")
        q16, k16, v16 = ((t * (ops.LOG2E if t is q else 1.0)).to(torch.bfloat16) for t in (q, k, v))
        # the 8-head yardstick: q [B][8][nc][64], kv [B][8][ns][128] (K | V'), vt its transposed image
        qh = (torch.randn(B, 8, nc, 64, device="cuda") * 0.5).to(torch.bfloat16)
        kvh = (torch.randn(B, 8, ns, 128, device="cuda") * 0.5).to(torch.bfloat16)
        vth = ops.transpose_v(kvh)
        cands = {
            "attn_wide bf16": lambda: ops.attn_wide(q16, k16, v16, fcs, mu, rs, vmu),
            "attn_wide bf16 (again)": lambda: ops.attn_wide(q16, k16, v16, fcs, mu, rs, vmu),
            "loss_attn fp32 512/512": lambda: ops.loss_attn(q, k, v, fcs, mu, rs, _lib.ACT_SOFTMAX),
            "mhada_attn bf16 8 heads": lambda: ops.mhada_attn(qh, kvh, vth, fcs, mu, rs, vmu, _lib.ACT_SOFTMAX),
        }
        for fn in cands.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        ts = {n: [] for n in cands}
        for _ in range(rounds):
            for n, fn in cands.items():
                ts[n].append(once(fn))
        med = {n: median(t) for n, t in ts.items()}
        fl = 6.0 * nc * ns * C * B
        a, a2, lo = med["attn_wide bf16"], med["attn_wide bf16 (again)"], med["loss_attn fp32 512/512"]
        res = abs(a - a2) / min(a, a2)
        print(f"{name}: Nc = Ns = {nc}, B = {B}, {fl / 1e12:.2f} TFLOP, {rounds} interleaved rounds", flush=True)
        for n, t in med.items():
            print(f"  {n:26s} {t:9.3f} ms  {fl / t / 1e9:8.1f} TF/s  {fl / t / 1e9 / 2500:.4f} of 2.5 PF  "
                  f"(min {min(ts[n]):.3f} max {max(ts[n]):.3f})", flush=True)
        print(f"  A-against-A resolution {res * 100:.2f} %; loss_attn / attn_wide = x{lo / max(a, a2):.2f} "
              f"({'beyond' if lo / max(a, a2) - 1 > res else 'WITHIN'} the resolution)", flush=True)


if __name__ == "__main__":
    main()
