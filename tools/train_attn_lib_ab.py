"""A/B of the fp32 training attention (csrc/attn_train.hip, the bwd_prep entries of csrc/train_ops.hip)
between two builds of libmhada_hip.so in ONE process, as tools/lib_ab.py: bits first, then time.

    python tools/train_attn_lib_ab.py <parent.so> <copy of parent.so> <new.so> [--rounds 9]

Bits: every output of the seven attention entries and the two prep entries at head widths 32, 64, 128
(64: the plain forward, both TRAIN_FWD_* knobs off, and the recompute backward), and the dS-spill
entry mhada_attn_train_dkv in both forms (tuning train_dkv_dma 1 / 0), new against parent, compared
as bit patterns.  Any mismatch ends the run with exit status 1.

Time: interleaved rounds of parent, its copy and new, device events around `iters` calls (sized to
about 30 ms per sample), the median per build.  The largest |copy / parent - 1| over the paths is the
resolution of the measurement; new / parent is marked "ok" within twice that, "OUTSIDE" otherwise.
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import _lib, ops

LIBS = {}


def use(name):
    _lib._lib = LIBS[name]


def inputs(BH, Nc, Ns, D, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, x, dout = (torch.randn(BH, n, D, generator=g) * s
                        for n, s in ((Nc, 0.5), (Ns, 0.5), (Ns, 3.0), (Nc, 1.0), (Nc, 1.0)))
    v = v - v.mean(dim=1, keepdim=True)
    return [t.cuda().contiguous() for t in (q, k, v, x, dout)]


def entries(D):
    """(fwd, prep, bwd, dq) of width D: the plain fp32-MFMA kernels."""
    if D == 64:
        return ops.attn_train_fwd, ops.attn_train_bwd_prep, \
            lambda *a: ops.attn_train_bwd(*a, spill=False), ops.attn_train_dq
    return ops.attn_train_fwd_hd, ops.attn_train_bwd_prep_hd, ops.attn_train_bwd_hd, ops.attn_train_dq_hd


def chain(D, q, k, v, x, dout):
    fwd, prep, bwd, dq = entries(D)
    out, mo, lse = fwd(q, k, v, x)
    dx, dmo, dd = prep(dout, x, mo)
    return dict(zip(("out", "mo", "lse", "dx", "dmo", "dd", "dq", "dk", "dv", "dq_only"),
                    (out, mo, lse, dx, dmo, dd, *bwd(q, k, v, lse, dmo, dd), dq(q, k, v, lse, dmo, dd))))


def spill(dma, q, k, v, x, dout):
    """mhada_attn_train_dkv with the dS spill (dma: the LDS-DMA kernel or the register-staged one)."""
    out, mo, lse = ops.attn_train_fwd(q, k, v, x)
    dx, dmo, dd = ops.attn_train_bwd_prep(dout, x, mo)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    ds = torch.full((q.shape[0], q.shape[1], k.shape[1]), float("nan"), device="cuda")
    with _lib.tuning(train_dkv_dma=dma):
        ops._call("mhada_attn_train_dkv", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
                  dd.data_ptr(), dk.data_ptr(), dv.data_ptr(), ds.data_ptr(), q.shape[0], q.shape[1], k.shape[1])
    return {"dk": dk, "dv": dv, "ds": ds}


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def bits():
    bad = 0
    cases = [(f"D {D:3d} chain", D, shape, lambda *a, D=D: chain(D, *a))
             for D in (32, 64, 128) for shape in ((2, 200, 160), (3, 37, 5), (1, 128, 64))]
    cases += [(f"D  64 spill dma={dma}", 64, shape, lambda *a, dma=dma: spill(dma, *a))
              for dma in (1, 0) for shape in ((2, 161, 96), (2, 33, 4))]
    for label, D, (BH, Nc, Ns), fn in cases:
        t = inputs(BH, Nc, Ns, D, seed=BH * 1000 + Nc + Ns + D)
        res = {}
        for name in ("P", "N"):
            use(name)
            res[name] = fn(*t)
        torch.cuda.synchronize()
        diff = [key for key in res["P"] if not same_bits(res["P"][key], res["N"][key])]
        finite = all(bool(torch.isfinite(v).all()) for v in res["N"].values())
        bad += bool(diff) or not finite
        print(f"bits {label:20s} ({BH}, {Nc:3d}, {Ns:3d}): {len(res['P'])} outputs "
              f"{'EQUAL' if not diff else 'DIFFER: ' + ' '.join(diff)}{'' if finite else ' NON-FINITE'}", flush=True)
    return bad


def sample(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def times(rounds):
    ops.TRAIN_FWD_S3 = ops.TRAIN_FWD_VT = False
    rows = []
    for D, BH in ((32, 16), (64, 8), (128, 4)):
        for n in (1024, 4096):
            q, k, v, x, dout = inputs(BH, n, n, D, seed=n + D)
            fwd, prep, bwd, dq = entries(D)
            use("P")
            out, mo, lse = fwd(q, k, v, x)
            dx, dmo, dd = prep(dout, x, mo)
            paths = [("fwd", lambda: fwd(q, k, v, x)), ("prep", lambda: prep(dout, x, mo)),
                     ("dq", lambda: dq(q, k, v, lse, dmo, dd)), ("bwd dq+dkv", lambda: bwd(q, k, v, lse, dmo, dd))]
            if D == 64:
                paths.append(("dkv spill (dma)", lambda: spill_only(q, k, v, lse, dmo, dd)))
            for label, fn in paths:
                for name in LIBS:  # warm-up of every build at this shape
                    use(name)
                    fn()
                    fn()
                use("P")
                iters = max(5, min(400, math.ceil(30.0 / max(sample(fn, 5), 1e-3))))
                t = {name: [] for name in LIBS}
                for _ in range(rounds):
                    for name in LIBS:
                        use(name)
                        t[name].append(sample(fn, iters))
                med = {name: statistics.median(v) for name, v in t.items()}
                rows.append((f"D {D:3d} BH {BH:2d} N {n:4d} {label}", med, iters))
                print(f"time {rows[-1][0]:36s} x{iters:3d}  parent {med['P'] * 1e3:9.1f} us  copy/parent "
                      f"{med['P2'] / med['P']:.4f}  new/parent {med['N'] / med['P']:.4f}", flush=True)
    res = max(abs(med["P2"] / med["P"] - 1) for _, med, _ in rows)
    print(f"resolution: largest |copy / parent - 1| = {res:.4f}; accepted |new / parent - 1| <= {2 * res:.4f}")
    for label, med, _ in rows:
        r = med["N"] / med["P"]
        print(f"verdict {label:36s} new/parent {r:.4f}  {'ok' if abs(r - 1) <= 2 * res else 'OUTSIDE'}")


def spill_only(q, k, v, lse, dmo, dd):
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    ds = torch.empty(q.shape[0], q.shape[1], k.shape[1], device="cuda")
    ops._call("mhada_attn_train_dkv", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
              dd.data_ptr(), dk.data_ptr(), dv.data_ptr(), ds.data_ptr(), q.shape[0], q.shape[1], k.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("parent_copy")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_attn_lib_ab.py needs the GPU: there is nothing to measure on the CPU")
    LIBS.update(P=_lib.load(a.parent), P2=_lib.load(a.parent_copy), N=_lib.load(a.new))
    ops.TRAIN_FWD_S3 = ops.TRAIN_FWD_VT = False
    if bits():
        sys.exit(1)
    times(a.rounds)


if __name__ == "__main__":
    main()
