"""The attention probes of tests/attn_probe.py, checked on the CPU (no kernel runs here).

This file is what ties tests/test_gpu_attn_forms.py to something other than the kernels:
  * the fp32 evaluation of the reference with plain torch ops stays within bound / 4 at every shape, map,
    level and width of the table (this is how attn_probe.C_BOUND is chosen: 4 x the largest ratio);
  * the weight a softmax probe leaves outside a query's group moves the result by less than `leak`;
  * three injected defects are each flagged by the element-wise bound of a bf16 kernel (the fp32 bound plus
    the 2^-8 |ref| output rounding) at every shape: V' taken in the bits-2-3-swapped key order while K is
    not, the last key dropped, one zero-padded key counted in the row sum.
Measured here (H = 1): the fp32 evaluation reaches 1.95 to 2.14 of the bound at C = 1, depending on the CPU
(cosine, d_qk = 136 / 452, Ns = 4096);
the permutation is flagged on 12-100 % of the rows under the "mod" and "mix" key maps and, for the softmax
probes, on none under "tile"; the dropped key on the rows of its group (0.7-100 %); the counted pad key on
every row of the "flat" probes, always on f = 0 elements, whose bound is M's alone: that is why a third
of the elements have f = 0.
"""
import pytest
import torch

import attn_probe as P

BF16 = torch.bfloat16
# (name, Dqk, Dv, natural units): the three head widths of mhada_attn / mhada_attn_hd and two wide
# d_qk of mhada_loss_attn (nch = 2 at W = 1; the register form at d_v 256)
WIDTHS = [("d32", 32, 32, False), ("d64", 64, 64, False), ("d128", 128, 128, False),
          ("wide136", 136, 64, True), ("wide452", 452, 64, True)]
H = 1


def probes(shape, width):
    B, Nc, Ns = shape
    _, Dqk, Dv, natural = width
    for km, qm, lv in P.SOFTMAX_PROBES:
        yield P.Probe(B, H, Nc, Ns, Dqk, Dv, "softmax", km, qm, lv, natural=natural)
    for km, qm, _ in P.COSINE_PROBES:
        yield P.Probe(B, H, Nc, Ns, Dqk, Dv, "cosine", km, qm)


@pytest.mark.parametrize("width", WIDTHS, ids=[w[0] for w in WIDTHS])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_evaluation_stays_within_a_quarter_of_the_bound(shape, width):
    assert P.C_BOUND <= 16 and P.C_BOUND >= 4 * P.REF32_WORST
    worst = 0.0
    for p in probes(shape, width):
        r = P.evaluate(p)
        if p.act == "softmax" and not p.natural:  # the premise: every weight numerator is a power of two
            s = p.q @ p.k.transpose(-1, -2)
            w = torch.exp2(s - s.amax(-1, keepdim=True))
            mant, _ = torch.frexp(w[w > 0])
            assert bool((mant == 0.5).all())
        err = (P.evaluate(p, f32=True)["out"].double() - r["out"]).abs()
        ratio = (err / P.bound(p, r, c=1.0)).max().item()
        worst = max(worst, ratio)
        assert bool((err <= P.bound(p, r) / 4).all()), f"{p.name}: fp32 evaluation at {ratio:.2f} of the C = 1 bound"
    print(f"REF32 {width[0]} {shape}: worst fp32 error / bound(C = 1) = {worst:.3f}")
    assert worst <= P.REF32_WORST


@pytest.mark.parametrize("width", WIDTHS, ids=[w[0] for w in WIDTHS])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_of_group_weight_stays_below_leak(shape, width):
    for p in probes(shape, width):
        if p.act != "softmax":
            continue
        has = p.in_group().any(-1)  # queries whose group holds a key
        if not bool(has.any()):
            continue
        a = P.weights(p)
        out_w = torch.where(p.in_group(), torch.zeros_like(a), a).sum(-1)[..., has]
        assert bool((out_w <= p.Ns * 2.0 ** -40).all()), p.name
        r = P.evaluate(p)
        a_in = torch.nan_to_num(P.weights(p, in_group_only=True), nan=0.0)
        r_in = P.evaluate(p, a=a_in)
        diff = (r_in["out"] - r["out"]).abs()[:, has]
        # (to first order M moves by eps (|mean out-of-group v'| + |M|) <= 16 eps, eps = Ns 2^-40: twice the
        # 8 eps of the leak term where |M| = 8, measured 1.10 x.  The reference keeps these weights, so the
        # GPU bound does not lean on the term; it is room for a kernel that flushes them.)
        assert bool((diff <= 2 * P.leak(p, r)[:, has]).all()), p.name


def _permuted_v(p):
    """V' read at the vt image's key position while K is read in the natural order."""
    n16 = -(-p.Ns // 16) * 16
    vpad = torch.zeros(*p.v.shape[:2], n16, p.Dv, dtype=torch.float64)
    vpad[:, :, :p.Ns] = p.v
    return vpad[:, :, P.swap23(torch.arange(p.Ns))]


def _drop_last(p):
    a = P.weights(p).clone()
    a[..., -1] = 0
    return a / a.sum(-1, keepdim=True)


def _with_pad_key(p):
    """One zero-padded key (K = 0, V' = 0) counted like a real one."""
    x = object.__new__(P.Probe)
    x.__dict__.update(p.__dict__)
    x.k = torch.cat([p.k, torch.zeros_like(p.k[:, :, :1])], 2)
    x.v = torch.cat([p.v, torch.zeros_like(p.v[:, :, :1])], 2)
    x.Ns = p.Ns + 1
    return x


def _flagged(p, r, out, bf16):
    """Fraction of query rows with an element beyond the bound."""
    bad = (out - r["out"]).abs() > P.bound(p, r, bf16_out=bf16)
    return bad.any(-1).double().mean().item(), bad


@pytest.mark.parametrize("width", WIDTHS[:3], ids=[w[0] for w in WIDTHS[:3]])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_injected_defects_are_flagged(shape, width):
    """Softmax probes against the bf16 kernels' bound, cosine probes against the fp32 bound (a key counted
    once too often moves a cosine row by 1 / Ns, below bf16 output rounding at Ns = 4096).  The permutation
    must be flagged under the "mod" and the "mix" key map, the counted pad key under all three, the dropped
    key under at least one (at D = 128, Nc = 64, Ns = 1024 no query of the "mod" maps is in the last key's
    group).  Not under every single probe: the "blk" query map reaches only the groups 0 .. Nc / 32, which at
    Nc <= 130 are fixed points of the bit swap and need not hold the last key; and above level 0 a pad
    key's weight 2^0 is itself below 2^-40, so the pad defect is judged on the "flat" probes."""
    seen = {}
    for p0 in probes(shape, width):
        soft = p0.act == "softmax"
        p = p0.rounded(BF16) if soft else p0
        r = P.evaluate(p)
        km = p.name.split("-")[1]

        def note(defect, frac):
            key = (p.act, defect, km)
            seen[key] = max(seen.get(key, 0.0), frac)
        note("perm", _flagged(p, r, P.evaluate(p, v=_permuted_v(p))["out"], soft)[0])
        note("drop", _flagged(p, r, P.evaluate(p, a=_drop_last(p))["out"], soft)[0])
        if not soft or p.name.endswith("flat"):
            pad, bad = _flagged(p, r, P.evaluate(_with_pad_key(p))["out"], soft)
            note("pad", pad)
            if soft:  # the f = 0 elements, whose bound is M's alone, are there to show this defect
                assert bool(bad[r["f"] == 0].any()), p.name
    for act in ("softmax", "cosine"):
        print(f"DEFECTS {width[0]} {shape} {act}: flagged row fraction " +
              " ".join(f"{d}/{km} {seen[(act, d, km)]:.3f}" for d in ("perm", "drop", "pad") for km in P.KEY_MAPS))
        assert seen[(act, "perm", "mod")] > 0 and seen[(act, "perm", "mix")] > 0, f"{act}: permuted V' not flagged"
        assert max(seen[(act, "drop", km)] for km in P.KEY_MAPS) > 0, f"{act}: dropped last key not flagged"
        assert min(seen[(act, "pad", km)] for km in P.KEY_MAPS) > 0, f"{act}: counted pad key not flagged"
