"""Probe operands for the inference attention kernels, with their fp64 reference and element-wise bound.

A plain helper module (tests/test_attn_probe_cpu.py checks it on the CPU, tests/test_gpu_attn_forms.py
runs the kernels on it).  The idea: every attention weight is an exact power of two (softmax) or exactly
0, 1 or 2 (cosine) and every V' is a small integer, so a correct kernel rounds only in the final mean,
the square root and the output store, while a mis-addressed, dropped or twice-counted key changes an
integer sum or an integer count.

Softmax probe (head width D, logits in log2 units as mhada_attn's K contract has them):
  q_i = e_{gq(i)} (one-hot), k_j = -40 everywhere except k_j[gk(j)] = L(j // 64), so q_i . k_j is exactly
  L(j // 64) for the keys of query i's group (gk(j) == gq(i)) and -40 for every other key: the other keys
  weigh at most 2^-40 of an in-group key.  Queries whose group holds no key see uniform weights.
  natural units (mhada_loss_attn): the same integers times fp32(ln 2), and fp32(-41 ln 2) outside the
  group (one more level, so that the rounding of ln 2 cannot lift the ratio above 2^-40).  The reference
  exponentiates the fp32 values the kernel is handed, so the weights are powers of two to 2^-24 |L| only.
  Levels L(t): 0 ("flat"), 8 t ("l8"), 40 t ("l40": an online-max kernel rescales at every 64-key block,
  a fixed-shift kernel passes 2^64 above its first tile and must take its exact recompute).
  Every entry is an integer; operands() rounds them to the kernel's operand type and the reference uses
  the rounded values (bf16 holds 8 t exactly, and 40 t up to 2048; above that a level moves to the next
  multiple of 16, stays an integer, and the weights stay powers of two).
  V'[b][h][j][d] = (131 j + 71 d + 13 (j // 7) + 5 (b H + h)) mod 17 - 8: integers in [-8, 8], V'^2 <= 64
  exact in bf16 (the (b, h) term makes a read from another head's keys visible).
Cosine probe: q^_i = e_{gq(i)}, k^_j = s_j e_{gk(j)}, s_j = -1 where (7 j + j // 64) % 3 == 0, else +1:
  the weights q^ . k^ + 1 are exactly 2, 0 (in-group) or 1.
Key maps gk: "mod" j % D, "tile" (j // 64) % D (whole-tile mistakes; blind to a permutation inside a
  tile), "mix" (37 j + 11 (j // 64)) % D.  Query maps gq: "mod" i % D, "blk" (i // 32) % D, "mix" (29 i + 5) % D.
Content side: f = (fcs - mu) rstd is exactly 0 on the elements with (i + c) % 3 == 0 (they expose M
  alone), exactly +-64 where (i + c) % 3 == 1 (they expose S) and Gaussian elsewhere; mu are small
  integers, rstd in {1/2, 1, 2}, so the kernel's fp32 (fcs - mu) rstd is exact on the first two kinds.
  v_mu is Gaussian.

Reference (include/mhada_hip.h, fp64): A = softmax(Q K^T) or (q^ . k^ + 1) / rowsum, M = A V',
E2 = A V'^2, S = sqrt(max(E2 - M^2, 1e-6)), out = S f + M + v_mu, with A1 = A |V'| and A2 = A V'^2 for the
bound.  A group of one key has E2 - M^2 = 0 exactly: the 1e-6 clamp is exercised.

Bound, per output element (u = 2^-24):
  |out - ref| <= C_BOUND u (A1 + |M| + |v_mu| + |f| (A2 + 2 |M| A1) / (2 S) + |S f|) + leak (+ 2^-8 |ref|, bf16 out)
  leak = Ns 2^-40 8 (1 + 8 |f| / S) (softmax: room for a kernel that drops the out-of-group weights; 0 for
  the cosine probes, whose weights are exact).  The first-order error of M is u-relative to A1 + |M|, that
  of S = sqrt(E2 - M^2) is the errors of E2 and M^2 divided by 2 S, and S f and the final sum round once
  each.  C_BOUND is not taken from any kernel: it is 4 times the largest ratio that an fp32 evaluation
  of the reference with plain torch ops reaches over every shape, map, level and width of the table
  (measured 1.95 to 2.14 -> REF32_WORST = 2.5, C_BOUND = 10; test_attn_probe_cpu.py re-measures it and holds
  the fp32 evaluation to bound / 4).  That evaluation, like the fp64 one, sums the weights' numerators
  and divides once per element, the order of every kernel here; normalising the weights first puts
  a rounding into each of the Ns terms, an error of the evaluation that grows like sqrt(Ns) u (10 x the
  bound at C = 1 for the cosine probes at Ns = 4096) and says nothing about the expression.  The factor 4 covers another summation order, a reciprocal multiply
  instead of a division, a one-ulp exp2 and truncating adders inside the MFMA.
"""
import math

import torch

U = 2.0 ** -24
# fp32-torch error / (bound at C = 1), the largest over the table (test_attn_probe_cpu.py): 1.954 on one CPU,
# 2.14 on another (the element-wise fp32 ops contract into fmas differently); 2.5 leaves room for a third
REF32_WORST = 2.5
C_BOUND = 10.0     # 4 * REF32_WORST; the condition is C_BOUND <= 16

# (B, Nc, Ns): fewer keys than a tile (empty groups) | ragged both | one whole 128 tile | three tiles |
# ragged over many tiles | eight whole 128 tiles | sixty-four 64-key tiles
SHAPES = [(1, 97, 33), (2, 300, 100), (1, 256, 128), (1, 97, 384), (2, 300, 700), (1, 64, 1024), (1, 130, 4096)]

KEY_MAPS = {
    "mod": lambda j, D: j % D,
    "tile": lambda j, D: (j // 64) % D,
    "mix": lambda j, D: (37 * j + 11 * (j // 64)) % D,
}
QUERY_MAPS = {
    "mod": lambda i, D: i % D,
    "blk": lambda i, D: (i // 32) % D,
    "mix": lambda i, D: (29 * i + 5) % D,
}
LEVELS = {"flat": 0, "l8": 8, "l40": 40}
OUT_LEVEL = -40

# every key map with every level schedule, the query map rotating so that each meets each key map
SOFTMAX_PROBES = [(km, list(QUERY_MAPS)[(a + b) % 3], lv) for a, km in enumerate(KEY_MAPS) for b, lv in enumerate(LEVELS)]
COSINE_PROBES = [(km, qm, None) for km in KEY_MAPS for qm in QUERY_MAPS]


def swap23(n):
    """The key position of the bf16 vt image and the SPLIT3 plane image: bits 2 and 3 of n swapped."""
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


class Probe:
    """Operands of one probe as fp64 tensors holding the exact intended values:
    q [B][H][Nc][Dqk], k [B][H][Ns][Dqk], v [B][H][Ns][Dv], fcs [B][Nc][H Dv], mu / rstd / v_mu [B][H Dv]."""

    def __init__(self, B, H, Nc, Ns, Dqk, Dv, act, kmap, qmap, level=None, natural=False, device="cpu", seed=0):
        self.B, self.H, self.Nc, self.Ns, self.Dqk, self.Dv = B, H, Nc, Ns, Dqk, Dv
        self.act, self.natural = act, natural
        self.name = f"{act}-{kmap}-{qmap}" + (f"-{level}" if level else "")
        dev = device
        i = torch.arange(Nc, device=dev)
        j = torch.arange(Ns, device=dev)
        self.gq = QUERY_MAPS[qmap](i, Dqk)
        self.gk = KEY_MAPS[kmap](j, Dqk)
        q = torch.zeros(Nc, Dqk, dtype=torch.float64, device=dev)
        q[i, self.gq] = 1.0
        if act == "softmax":
            lv = (LEVELS[level] * (j // 64)).double()
            k = torch.full((Ns, Dqk), float(OUT_LEVEL - (1 if natural else 0)), dtype=torch.float64, device=dev)
            k[j, self.gk] = lv
            if natural:  # fp32(level) * fp32(ln 2), rounded to fp32: what mhada_loss_attn is handed
                k = (k.float() * torch.tensor(math.log(2.0), dtype=torch.float32, device=dev)).double()
        else:
            sgn = torch.where((7 * j + j // 64) % 3 == 0, -1.0, 1.0).double()
            k = torch.zeros(Ns, Dqk, dtype=torch.float64, device=dev)
            k[j, self.gk] = sgn
        self.q = q.expand(B, H, Nc, Dqk).contiguous()
        self.k = k.expand(B, H, Ns, Dqk).contiguous()
        d = torch.arange(Dv, device=dev)
        bh = torch.arange(B * H, device=dev).view(B, H, 1, 1)
        self.v = ((131 * j.view(1, 1, Ns, 1) + 71 * d.view(1, 1, 1, Dv) + 13 * (j.view(1, 1, Ns, 1) // 7) + 5 * bh) % 17
                  - 8).double()
        C = H * Dv
        g = torch.Generator(device="cpu").manual_seed(1234 + seed)
        c = torch.arange(C, device=dev)
        ii = i.view(1, Nc, 1)
        kind = (ii + c.view(1, 1, C)) % 3
        mu = ((c % 5) - 2).double().expand(B, C).contiguous()
        rstd = torch.pow(2.0, ((c % 3) - 1).double()).expand(B, C).contiguous()
        gauss = torch.randn(B, Nc, C, generator=g, dtype=torch.float64).to(dev)
        sign = torch.where(((ii + c.view(1, 1, C)) // 3) % 2 == 0, 1.0, -1.0).double()
        f = torch.where(kind == 0, torch.zeros_like(gauss), torch.where(kind == 1, 64.0 * sign, gauss))
        # fcs in fp32, as the kernel reads it; f is then DEFINED as the fp64 value of (fcs - mu) rstd
        self.fcs = (f / rstd[:, None] + mu[:, None]).float().double()
        self.mu, self.rstd = mu, rstd
        self.v_mu = torch.randn(B, C, generator=g, dtype=torch.float64).float().double().to(dev)

    def in_group(self):
        """[Nc][Ns] bool: key j belongs to query i's group."""
        return self.gq[:, None] == self.gk[None, :]

    def rounded(self, dtype):
        """A copy whose q, k and v are rounded to the kernel's operand type (the values it computes with)."""
        p = object.__new__(Probe)
        p.__dict__.update(self.__dict__)
        p.q, p.k, p.v = (t.to(dtype).double() for t in (self.q, self.k, self.v))
        assert torch.equal(p.q, self.q) and torch.equal(p.v, self.v)
        if not self.natural:
            assert torch.equal(p.k, p.k.round()), "a rounded level is no longer an integer"
        return p


def weights(p, in_group_only=False, f32=False, normalise=True):
    """The attention weights A [B][H][Nc][Ns] (fp64, or fp32 with plain torch ops); normalise = False: their
    numerators exp2(s - rowmax) / q^ . k^ + 1, which are exact in either precision."""
    dt = torch.float32 if f32 else torch.float64
    s = p.q.to(dt) @ p.k.to(dt).transpose(-1, -2)
    if p.act == "softmax":
        if in_group_only:
            s = torch.where(p.in_group(), s, torch.full_like(s, -math.inf))
        s = s - s.amax(-1, keepdim=True)
        w = torch.exp(s) if p.natural else torch.exp2(s)
    else:
        w = s + 1.0
        if in_group_only:
            w = torch.where(p.in_group(), w, torch.zeros_like(w))
    return w / w.sum(-1, keepdim=True) if normalise else w


def evaluate(p, a=None, v=None, f32=False):
    """The reference expression: dict of out, M, E2, A1, A2, S, f, v_mu as [B][Nc][H Dv] tensors.
    a / v: other weights / values (the injected defects of the CPU test)."""
    dt = torch.float32 if f32 else torch.float64
    B, H, Nc, Dv = p.B, p.H, p.Nc, p.Dv
    a = weights(p, f32=f32, normalise=False) if a is None else a
    v = (p.v if v is None else v).to(dt)
    l = a.sum(-1, keepdim=True)

    def rows(x):  # [B][H][Nc][Dv] -> [B][Nc][H Dv]
        return x.permute(0, 2, 1, 3).reshape(B, Nc, H * Dv)
    # numerators first, one division per element (the flash order of every kernel here): with integer V'
    # the sums are sums of integers times powers of two
    m = rows(a @ v / l)
    e2 = rows(a @ (v * v) / l)
    a1 = rows(a @ v.abs() / l)
    s = torch.sqrt(torch.clamp(e2 - m * m, min=1e-6))
    f = (p.fcs.to(dt) - p.mu.to(dt)[:, None]) * p.rstd.to(dt)[:, None]
    vmu = p.v_mu.to(dt)[:, None].expand_as(m)
    return dict(out=s * f + m + vmu, M=m, E2=e2, A1=a1, A2=e2, S=s, f=f, v_mu=vmu)


def leak(p, r):
    if p.act != "softmax":
        return torch.zeros_like(r["S"])
    return p.Ns * 2.0 ** -40 * 8.0 * (1.0 + r["f"].abs() * 8.0 / r["S"])


def bound(p, r, c=C_BOUND, bf16_out=False):
    """The element-wise bound of the module docstring for the fp64 evaluation r of probe p."""
    m, s, f = r["M"].abs(), r["S"], r["f"].abs()
    b = c * U * (r["A1"] + m + r["v_mu"].abs() + f * (r["A2"] + 2 * m * r["A1"]) / (2 * s) + s * f) + leak(p, r)
    if bf16_out:
        b = b + 2.0 ** -8 * r["out"].abs()
    return b
