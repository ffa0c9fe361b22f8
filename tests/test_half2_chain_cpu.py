"""The HALF2 chain (MLP2 and the attention out-projection as HALF2 products) without a GPU: the bound
Z_k = sqrt(C) ||gamma * w_k|| + |beta . w_k + b_k| against the adversarial LayerNorm output, the per-column
scale u, the exact weight division, the plane reconstruction of u v, an fp64 emulation of the three-product
sum, every refusal, and the bound under the batch-axis attention's convex combination."""
import math

import pytest
import torch

from mhada_hip import engine, ops

FP16_MIN = 2.0 ** -14


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def params(C, N, gs, bs, ws, seed):
    return (rnd(C, scale=gs, seed=seed), rnd(C, scale=bs, seed=seed + 1), rnd(N, C, scale=ws, seed=seed + 2),
            rnd(N, scale=ws, seed=seed + 3))


def adversarial(g, be, w, b):
    """Per output k the xhat with sum xhat^2 = C aligned with +-gamma * w[k] (the sign of the offset): the
    LayerNorm output gamma xhat + beta that maximises |y . w[k] + b[k]|.  -> values [N] in fp64."""
    g, be, w, b = g.double(), be.double(), w.double(), b.double()
    d = w * g[None, :]
    off = w @ be + b
    sgn = torch.where(off >= 0, 1.0, -1.0)
    xhat = sgn[:, None] * d / d.norm(dim=1, keepdim=True) * math.sqrt(g.numel())
    assert torch.allclose((xhat ** 2).sum(1), torch.full((w.shape[0],), float(g.numel()), dtype=torch.float64))
    y = g[None, :] * xhat + be[None, :]
    return (y * w).sum(1) + b


CASES = [(512, 96, 1.0, 1.0, 0.04, 1), (512, 96, 1e-3, 0.0, 0.04, 2), (256, 64, 40.0, 7.0, 3.0, 3), (128, 64, 1e3, 1e4, 1e-3, 4)]


@pytest.mark.parametrize("C,N,gs,bs,ws,seed", CASES)
def test_bound_and_scale_hold_for_the_adversarial_input(C, N, gs, bs, ws, seed):
    g, be, w, b = params(C, N, gs, bs, ws, seed)
    Z = ops.half2_chain_bound(g, be, w, b)
    assert Z.dtype == torch.float64
    worst = adversarial(g, be, w, b).abs()
    assert (worst <= Z * (1 + 1e-12)).all() and (worst >= Z * (1 - 1e-9)).all()  # the bound is attained
    # and holds for actual LayerNorm outputs, a one-hot row included
    x = rnd(64, C, seed=seed + 9)
    x[0] = 0
    x[0, int(g.abs().argmax())] = 1e4
    v = torch.nn.functional.layer_norm(x.double(), (C,), g.double(), be.double(), 1e-6) @ w.double().T + b.double()
    assert (v.abs() <= Z[None, :] * (1 + 1e-12)).all()
    u = ops.half2_out_scale(Z)
    assert u is not None and u.dtype == torch.float32 and (torch.frexp(u)[0] == 0.5).all()  # powers of two
    uz = u.double() * Z
    assert (uz <= 32768).all() and (2 * uz > 32768).all()
    # the bound evaluated in fp32 instead: the scaled adversarial value still fits fp16
    Z32 = math.sqrt(C) * (w * g[None, :]).norm(dim=1) + (w @ be + b).abs()
    assert Z32.dtype == torch.float32
    u32 = ops.half2_out_scale(Z32)
    assert (u32.double() * worst < 65504).all()


def test_weight_division_is_exact_and_planes_reconstruct_the_scaled_value():
    C, K0, N = 512, 128, 80
    g, be, w, b = params(C, K0, 1.0, 0.5, 0.04, 11)
    w[3] *= 2.0 ** -9  # a column with a small bound gets a large u
    u = ops.half2_out_scale(ops.half2_chain_bound(g, be, w, b))
    assert u[3] >= 256 * u.min()
    wc = rnd(N, K0, scale=0.03, seed=15)
    wu = wc / u[None, :]
    assert torch.equal(wu.double(), wc.double() / u.double()[None, :]) and torch.equal(wu * u[None, :], wc)
    h = ops.half2_chain_prepare(g, be, w, b, wc)
    w2, t = ops.half2_weight(wu)
    assert torch.equal(h["u"], u) and torch.equal(h["w2"].view(torch.int16), w2.view(torch.int16))
    assert torch.equal(h["cs"], (1.0 / t.double()).float()) and (torch.frexp(h["cs"])[0] == 0.5).all()
    # hi + lo = u v to max(2^-22 |u v|, 2^-14), for v anywhere inside the bound (tiny values included)
    Z = ops.half2_chain_bound(g, be, w, b)
    frac = torch.cat([torch.rand(4000, K0, generator=torch.Generator().manual_seed(3)) * 2 - 1,
                      torch.exp2(-torch.rand(4000, K0, generator=torch.Generator().manual_seed(4)) * 30)])
    v = (frac.double() * Z[None, :]).float()
    uv = u[None, :] * v
    assert torch.equal(uv.double(), u.double()[None, :] * v.double())  # the producer's multiply is exact
    assert (uv.abs() <= 32768).all()
    hi, lo = ops._half2_planes(uv)
    for p in (hi, lo):
        assert ((p == 0) | (p.abs().float() >= FP16_MIN)).all()
    err = (hi.double() + lo.double() - uv.double()).abs()
    assert (err <= torch.maximum(2.0 ** -22 * uv.double().abs(), torch.full_like(err, 2.0 ** -14))).all()
    assert (hi == 0).any() and (lo == 0).any()


@pytest.mark.parametrize("M,K0,N,relu", [(256, 2048, 512, True), (256, 512, 512, False)])
def test_three_product_sum_in_fp64_against_the_exact_product(M, K0, N, relu):
    """A planes of u a, W planes of t (w / u), every product and sum in fp64 (so only the plane rounding, the
    flush and the dropped lo lo term remain), times cs, against a w^T in fp64.  Per element the error is at
    most 4 * 2^-22 sum |a||w| (2^-22 per operand's planes, 2^-22 for lo lo, rounding of the bounds) plus the
    flush: 2^-14 / u_k per A element and 2^-14 / t_n per W element."""
    C = 512
    g, be, w1, b1 = params(C, K0, 1.0, 0.3, C ** -0.5, 21)
    x = rnd(M, C, seed=25) * 3 + 0.5
    a = torch.nn.functional.layer_norm(x, (C,), g, be, 1e-6) @ w1.T + b1
    if relu:
        a = torch.relu(a)
    wc = rnd(N, K0, scale=K0 ** -0.5, seed=26)
    h = ops.half2_chain_prepare(g, be, w1, b1, wc)
    assert h is not None
    u = h["u"]
    assert (u[None, :] * a.abs() <= 32768).all()
    ah, al = (p.double() for p in ops._half2_planes(u[None, :] * a))
    wu = wc / u[None, :]
    _, t = ops.half2_weight(wu)
    wh, wl = (p.double() for p in ops._half2_planes(wu * t[:, None]))
    out = (al @ wh.T + ah @ wh.T + ah @ wl.T) * h["cs"].double()[None, :]
    ref = a.double() @ wc.double().T
    aa, ww = a.double().abs(), wc.double().abs()
    bound = 4 * 2.0 ** -22 * (aa @ ww.T) + (2.0 ** -14 / u.double())[None, :] @ ww.T \
        + aa.sum(1, keepdim=True) * (2.0 ** -14 / t.double())[None, :]
    assert ((out - ref).abs() <= bound).all()
    e = ((out - ref).norm() / ref.norm()).item()
    print(f"chain emulation {M}x{N}x{K0}: norm-relative error {e:.3e}")
    assert e < 2e-6


def test_every_refusal_returns_none():
    C, K0, N = 128, 64, 32
    g, be, w, b = params(C, K0, 1.0, 0.5, 0.05, 31)
    wc = rnd(N, K0, scale=0.05, seed=35)
    assert ops.half2_chain_prepare(g, be, w, b, wc) is not None
    assert ops.half2_chain_prepare(g, be, w, None, wc) is not None
    wz, bz = w.clone(), b.clone()
    wz[5], bz[5] = 0, 0
    assert ops.half2_chain_prepare(g, be, wz, bz, wc) is None                       # a Z is zero
    assert ops.half2_out_scale(torch.tensor([1.0, float("inf")])) is None           # a Z not finite
    assert ops.half2_out_scale(torch.tensor([1.0, float("nan")])) is None
    for bad in (float("inf"), float("nan")):                                         # a parameter not finite
        for i in range(5):
            ts = [g.clone(), be.clone(), w.clone(), b.clone(), wc.clone()]
            ts[i].view(-1)[3] = bad
            assert ops.half2_chain_prepare(*ts) is None
    assert ops.half2_chain_prepare(g * 2.0 ** 60, be, w, b, wc) is None             # u < 2^-40
    assert ops.half2_chain_prepare(g, be, w * 2.0 ** 60, b, wc) is None
    assert ops.half2_chain_prepare(g * 2.0 ** -60, be * 2.0 ** -60, w, b * 2.0 ** -60, wc) is None  # u > 2^40
    ws = w.clone()
    ws[2] *= 2.0 ** -20  # one u 2^20 above the others, still inside the window: the scale is per column
    bs = b.clone()
    bs[2] *= 2.0 ** -20
    assert ops.half2_chain_prepare(g, be, ws, bs, wc) is not None
    ws[2] *= 2.0 ** -20
    bs[2] *= 2.0 ** -20
    assert ops.half2_chain_prepare(g, be, ws, bs, wc) is None                       # that one u > 2^40
    wc2 = wc.clone()
    wc2[7] *= 2.0 ** 60
    assert ops.half2_chain_prepare(g, be, w, b, wc2) is None                        # |w / u| > 2^40, t < 2^-40
    wc2[7] = wc[7] * 2.0 ** -60
    assert ops.half2_chain_prepare(g, be, w, b, wc2) is None                        # |w / u| < 2^-40, t > 2^40
    wc2[7] = 0
    assert ops.half2_chain_prepare(g, be, w, b, wc2) is None                        # a zero row: no |w / u| in the window
    assert ops.half2_chain_prepare(g, be, w[:48], b[:48], wc[:, :48]) is None       # K0 % 64
    assert ops.half2_chain_prepare(g, be, w[:32], b[:32], wc) is None               # producer / consumer mismatch


def layer(C=128, H=256, seed=41):
    return dict(ln1_g=rnd(C, seed=seed), ln1_b=rnd(C, seed=seed + 1), ln2_g=rnd(C, seed=seed + 2),
                ln2_b=rnd(C, seed=seed + 3), w_qkv=rnd(3 * C, C, scale=0.05, seed=seed + 4),
                b_qkv=rnd(3 * C, scale=0.05, seed=seed + 5), w_o=rnd(C, C, scale=0.05, seed=seed + 6),
                w1=rnd(H, C, scale=0.05, seed=seed + 7), b1=rnd(H, scale=0.05, seed=seed + 8),
                w2=rnd(C, H, scale=0.05, seed=seed + 9))


def test_engine_decides_once_per_layer_and_follows_the_switches(monkeypatch):
    monkeypatch.setattr(ops, "F32_HALF2", True)
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN", True)
    assert ops.F32_HALF2_CHAIN_OUTPROJ is False  # the out-projection half is opt-in
    assert engine._h2_chain(layer(), "w_o") is None and engine._h2_chain(layer(), "w2") is not None
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN_OUTPROJ", True)
    L = layer()
    C = 128
    m, o = engine._h2_chain(L, "w2"), engine._h2_chain(L, "w_o")
    assert m is not None and o is not None and L["w2_half2"] is m and L["w_o_half2"] is o
    assert engine._h2_chain(L, "w2") is m  # cached
    # the out-projection's bound is V's: the last third of the QKV weight
    want = ops.half2_out_scale(ops.half2_chain_bound(L["ln1_g"], L["ln1_b"], L["w_qkv"][2 * C:], L["b_qkv"][2 * C:]))
    assert torch.equal(o["u"], want)
    for sw in ("F32_HALF2", "F32_HALF2_CHAIN"):
        monkeypatch.setattr(ops, sw, False)
        assert engine._h2_chain(L, "w2") is None and engine._h2_chain(L, "w_o") is None
        monkeypatch.setattr(ops, sw, True)
    # MLP1 not HALF2 (its LayerNorm's scale leaves the window): MLP2 keeps SPLIT3, whatever its own bound says
    L2 = layer()
    L2["ln2_g"] = L2["ln2_g"] * 2.0 ** 56
    L2["w1"] = L2["w1"] * 2.0 ** -56
    assert ops.half2_chain_prepare(L2["ln2_g"], L2["ln2_b"] * 0, L2["w1"], L2["b1"], L2["w2"]) is not None
    assert engine._h2_chain(L2, "w2") is None and L2["w1_half2"] is None and L2["w2_half2"] is None
    # a LayerNorm weight times 2^56 puts the bounds outside the window: both routes refused
    L3 = layer()
    L3["ln1_g"] = L3["ln1_g"] * 2.0 ** 56
    L3["ln2_g"] = L3["ln2_g"] * 2.0 ** 56
    assert engine._h2_chain(L3, "w2") is None and engine._h2_chain(L3, "w_o") is None


@pytest.mark.parametrize("Lb", [1, 2, 8])
def test_the_convex_combination_keeps_the_bound(Lb):
    """The batch-axis attention output is softmax-weighted over the Lb images' V rows: each weight set is
    non-negative and sums to one (to rounding), so |att| <= max |V| <= Z."""
    C, ntok, heads = 128, 33, 2
    g, be, w, b = params(C, C, 2.0, 1.0, 0.2, 51)
    Z = ops.half2_chain_bound(g, be, w, b)
    u = ops.half2_out_scale(Z)
    x = rnd(Lb, ntok, C, seed=55) * 4
    x[0, 0] = 0
    x[0, 0, 5] = 1e5  # a one-hot token: xhat at its extreme
    v = torch.nn.functional.layer_norm(x, (C,), g, be, 1e-6) @ w.T + b
    assert (v.double().abs() <= Z * (1 + 1e-6)).all()
    logits = rnd(ntok, heads, Lb, Lb, scale=6.0, seed=56)
    p = torch.softmax(logits, dim=-1)  # fp32, as the kernel's
    vh = v.view(Lb, ntok, heads, C // heads).permute(1, 2, 0, 3)
    att = (p @ vh).permute(2, 0, 1, 3).reshape(Lb, ntok, C)
    assert (att.double().abs() <= Z * (1 + 1e-6)).all()
    assert (u * att.abs() <= 32768 * (1 + 1e-6)).all() and (u * att.abs() < 65504).all()
    if Lb == 1:
        assert torch.equal(att, v)
