"""A/B of the kernels whose instruction stream changed when they took the shared device helpers
(profiles/r30_helpers_isa.txt): three builds of libmhada_hip.so in ONE process, as tools/lib_ab.py.

    python tools/helpers_ab.py PARENT.so PARENT_COPY.so NEW.so

1. Bits: every entry point that launches such a kernel, run from PARENT and from NEW on the same operands;
   all outputs must be torch.equal as bit patterns.  The Winograd convs run every case of
   tests/test_gpu_wino_forms.py's FORMS table (its operands, epilogues and knobs; the SPLIT3 route with
   wino_s3_rows 0 and 1), the other entry points the odd / partial-tile shapes listed below.
2. Time: the same entry points at the shapes of the benchmark's 512 x 512, batch 8 step, interleaved
   rounds PARENT, COPY, NEW.  COPY is a byte copy of PARENT: the per-round ratios COPY / PARENT are the
   resolution of the measurement, spread = max |ratio - 1| over the rounds.  NEW passes for an entry
   point if its median ratio NEW / PARENT is at most 1 + spread (no number is fixed in advance).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd"), os.path.join(REPO, "tests")]

import torch

from mhada_hip import _lib, ops

LIBS = {k: _lib.load(p) for k, p in zip(("parent", "copy", "new"), sys.argv[1:4])}
ROUNDS, ITERS = 9, 10


def use(name):
    _lib._lib = LIBS[name]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(label, fn):
    """fn() -> list of tensors; PARENT against NEW."""
    out = {}
    for k in ("parent", "new"):
        use(k)
        out[k] = [bits(t).clone() for t in fn()]
    torch.cuda.synchronize()
    ok = all(torch.equal(a, b) for a, b in zip(out["parent"], out["new"]))
    print(f"bits  {label:58s} {'equal' if ok else 'DIFFER'}", flush=True)
    return ok


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS


def time_ab(label, fn):
    t = {k: [] for k in LIBS}
    for k in LIBS:
        use(k)
        fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k in LIBS:
            use(k)
            t[k].append(timed(fn))
    spread = max(abs(c / p - 1) for c, p in zip(t["copy"], t["parent"]))
    r = sorted(n / p for n, p in zip(t["new"], t["parent"]))
    med = r[len(r) // 2]
    ok = med <= 1 + spread
    print(f"time  {label:58s} parent {sorted(t['parent'])[ROUNDS // 2] * 1e3:9.1f} us  copy/parent spread "
          f"{spread:.4f}  new/parent median {med:.4f} (min {r[0]:.4f} max {r[-1]:.4f})  {'pass' if ok else 'FAIL'}",
          flush=True)
    return ok


def rnd(*shape):
    return torch.randn(*shape, device="cuda")


def wino_bits():
    import test_gpu_wino_forms as T
    ok = True
    for prm in T.FORMS:
        fm = prm.values[0]
        variants = [fm] if fm["route"] != "s3" else [dict(fm, knobs=dict(wino_s3_rows=r), name=f"{fm['name']}_rows{r}")
                                                     for r in (0, 1)]
        pb = T.problem(fm["grid"], fm["pad"], fm["Ci"], fm["Co"], False)
        for v in variants:
            def run():
                U, P = T.prepack(pb, v["planes"])
                ys = [T.run_conv(v, pb, U, ep, pb.Co + 4 * (i & 1)) for i, ep in enumerate(T.EPILOGUES)]
                return ys + ([P.t] if P is not None else [])
            ok &= same_bits("conv3x3_wino " + v["name"], run)
    return ok


def main():
    torch.manual_seed(0)
    ok = wino_bits()
    # ---- bits: the plane writers, partial tiles and odd sizes
    for BH, Nc, Ns in ((3, 1, 32), (2, 255, 96), (8, 257, 160), (1, 300, 64)):
        ldt = (Ns + 63) // 64 * 64
        k, ds = rnd(BH, Ns, 64), rnd(BH, Nc, Ns)

        def run():
            kt = ops.transpose64_split3(k)
            dq = torch.zeros(BH, Nc, 64, device="cuda")
            ops.gemm_n64_split3(ds, kt, dq, BH, Nc, Ns, ldt)
            return [kt, dq]
        ok &= same_bits(f"transpose64_split3 + gemm_n64_split3 BH{BH} Nc{Nc} Ns{Ns}", run)
    for N in (1, 63, 130):
        k = rnd(2, N, 64)
        ok &= same_bits(f"transpose64_split3 N{N}", lambda: [ops.transpose64_split3(k)])
    for rows, cols in ((1, 256), (7, 512), (300, 1024), (65, 2048)):
        x, g, b = rnd(rows, cols), rnd(cols), rnd(cols)
        ok &= same_bits(f"layernorm_split3 {rows}x{cols}", lambda: [ops.layernorm_split3(x, g, b, 1e-5)])
    for L, ntok in ((2, 5), (3, 100), (8, 37)):
        qkv, dout = rnd(L, ntok, 1536), rnd(L, ntok, 512)
        ok &= same_bits(f"vit_batch_attn_split3 L{L} ntok{ntok}", lambda: [ops.vit_batch_attn_split3(qkv, L, ntok, 8)])
        ok &= same_bits(f"vit_batch_attn_bwd planes L{L} ntok{ntok}",
                        lambda: list(ops.vit_batch_attn_bwd(qkv, dout, L, ntok, 8, planes=True)))

    # ---- time: the 512 x 512, batch 8 step's shapes
    for (B, H, Ci, Co) in ((8, 128, 256, 256), (8, 256, 128, 128)):
        x, w, bias = rnd(B, H, H, Ci), rnd(Co, 9 * Ci) / (9 * Ci) ** 0.5, rnd(Co)
        use("parent")
        u_s3 = ops.wino_weights(w)  # carries the plane image
        us = (u_s3.clone(), u_s3)   # the clone does not: the fp32 kernels
        y = torch.empty(B, H, H, Co, device="cuda")
        for label, idx, knobs in (("wino_kernel", 0, dict(wino4=0)), ("wino4_kernel", 0, {}),
                                  ("wino_s3_kernel", 1, dict(wino_s3_rows=0)), ("wino_s3_rows_kernel", 1, {})):
            def run():
                with _lib.tuning(**knobs):
                    ops.conv3x3_wino(x, us[idx], bias, True, out=y)
            ok &= time_ab(f"conv3x3_wino {label} {B}x{H}x{H} {Ci}->{Co}", run)
        ok &= time_ab(f"wino_weights_split3 {Co}x{Ci}", lambda: ops.wino_weights_split3(w))
    BH, N = 64, 4096
    k, ds, dq = rnd(BH, N, 64), rnd(BH, N, N), torch.empty(BH, N, 64, device="cuda")
    kt = ops.transpose64_split3(k)
    ok &= time_ab(f"gemm_n64_split3 BH{BH} {N}x{N}", lambda: ops.gemm_n64_split3(ds, kt, dq, BH, N, N, N))
    ok &= time_ab(f"transpose64_split3 BH{BH} N{N}", lambda: ops.transpose64_split3(k))
    del ds
    x, g, b = rnd(8 * 4096, 512), rnd(512), rnd(512)
    ok &= time_ab("layernorm_split3 32768x512", lambda: ops.layernorm_split3(x, g, b, 1e-5))
    qkv, dout = rnd(8, 4096, 1536), rnd(8, 4096, 512)
    ok &= time_ab("vit_batch_attn_split3 L8 ntok4096", lambda: ops.vit_batch_attn_split3(qkv, 8, 4096, 8))
    ok &= time_ab("vit_batch_attn_bwd planes L8 ntok4096", lambda: ops.vit_batch_attn_bwd(qkv, dout, 8, 4096, 8, planes=True))
    print("ALL PASS" if ok else "SOME FAILED")


if __name__ == "__main__":
    main()
