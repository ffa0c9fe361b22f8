"""HALF2 (an fp32 product as three fp16 products) without a GPU: the scale rules and their fallback, the
two-plane reconstruction with subnormals flushed, a torch emulation of the three-product sum against
fp64, and ops.half2_weight against a plain transcription of its definition."""
import math

import pytest
import torch

from mhada_hip import ops

FP16_MIN = 2.0 ** -14


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def planes(v):
    hi, lo = ops._half2_planes(v)
    for p in (hi, lo):  # no subnormal plane value survives
        assert ((p == 0) | (p.abs().float() >= FP16_MIN)).all()
    return hi, lo


@pytest.mark.parametrize("C,gs,bs,seed", [(512, 1.0, 1.0, 1), (512, 1e-3, 0.0, 2), (2048, 40.0, 7.0, 3), (256, 1e4, 1e5, 4)])
def test_a_scale_bounds_the_layernorm_output(C, gs, bs, seed):
    g, b = rnd(C, scale=gs, seed=seed), rnd(C, scale=bs, seed=seed + 10)
    s_a = ops.half2_a_scale(g, b)
    Y = math.sqrt(C) * g.abs().max().item() + b.abs().max().item()
    assert s_a is not None and math.frexp(s_a)[0] == 0.5  # a power of two
    assert Y * s_a <= 32768 < 2 * Y * s_a
    # the bound holds for an actual LayerNorm output, a one-hot row (|x^| = sqrt(C - 1)) included
    x = rnd(64, C, seed=seed + 20)
    x[0] = 0
    x[0, int(g.abs().argmax())] = 1e4
    y = torch.nn.functional.layer_norm(x, (C,), g, b, 1e-6)
    assert (y.abs() * s_a <= 32768).all()


def test_weight_row_maxima_land_in_the_top_binade():
    w = rnd(96, 128, scale=0.04, seed=5)
    w[3] *= 2.0 ** 20
    w[4] *= 2.0 ** -20
    w[5] = 0
    w[6, 1:] = 0
    w[6, 0] = 0.5  # an exact power of two: floor(log2) = -1, t = 2^15, t w = 2^14
    _, t = ops.half2_weight(w)
    m = (w * t[:, None]).abs().amax(1)
    nz = torch.arange(96) != 5
    assert (m[nz] >= 2.0 ** 14).all() and (m[nz] < 2.0 ** 15).all()
    assert t[5] == 1 and t[6] == 2.0 ** 15
    assert (torch.frexp(t)[0] == 0.5).all()


def test_fallback_cases():
    C = 512
    g, b, w = rnd(C, seed=1), rnd(C, seed=2), rnd(64, C, scale=0.04, seed=3)
    assert ops.half2_prepare(g, b, w) is not None
    assert ops.half2_prepare(torch.zeros(C), torch.zeros(C), w) is None            # Y = 0
    assert ops.half2_prepare(g * float("inf"), b, w) is None                        # Y not finite
    gn = g.clone()
    gn[7] = float("nan")
    assert ops.half2_prepare(gn, b, w) is None
    wn = w.clone()
    wn[5, 9] = float("inf")
    assert ops.half2_prepare(g, b, wn) is None                                      # a weight row not finite
    wn[5, 9] = float("nan")
    assert ops.half2_prepare(g, b, wn) is None
    assert ops.half2_prepare(g * 2.0 ** 60, b, w) is None                           # s_a < 2^-40
    assert ops.half2_prepare(g * 2.0 ** -60, b * 2.0 ** -60, w) is None             # s_a > 2^40
    ws = w.clone()
    ws[2] *= 2.0 ** -60
    assert ops.half2_prepare(g, b, ws) is None                                      # t_n > 2^40
    ws[2] = w[2] * 2.0 ** 60
    assert ops.half2_prepare(g, b, ws) is None                                      # t_n < 2^-40
    h = ops.half2_prepare(g, b, w)
    _, t = ops.half2_weight(w)
    assert torch.equal(h["cs"], (1.0 / (h["s_a"] * t.double())).float())
    assert (torch.frexp(h["cs"])[0] == 0.5).all()


def test_planes_reconstruct_with_subnormals_flushed():
    """hi + lo = v to 2^-22 relative for |v| >= 2^-3 and to 2^-14 absolute below — with fp16 subnormals kept
    (lo's spacing is then 2^-24 at worst).  With every subnormal plane value flushed, as the plane writers
    do, a flushed lo costs less than 2^-14 absolute, which is within 2^-22 relative only from |v| >= 2^8:
    the flushed planes meet max(2^-22 |v|, 2^-14) everywhere, 2^-14 absolute below 2^-3 included."""
    g = torch.Generator().manual_seed(7)
    mag = torch.exp2(torch.rand(200000, generator=g) * 36 - 21)     # 2^-21 .. 2^15
    v = (mag * torch.sign(torch.randn(200000, generator=g))).clamp(-32768, 32768)
    v = torch.cat([v, torch.tensor([0.0, -0.0, 32768.0, -32768.0, 2.0 ** -14, 2.0 ** -15, 1 + 2.0 ** -11, 2.0 ** -3,
                                    2.0 ** -24, 3 * 2.0 ** -16])])
    big = v.abs() >= 2.0 ** -3
    av = v.double().abs()
    h0 = v.half()
    err0 = (h0.double() + (v - h0.float()).half().double() - v.double()).abs()  # subnormals kept
    assert (err0[big] <= 2.0 ** -22 * av[big]).all()
    assert (err0[~big] <= 2.0 ** -14).all()
    hi, lo = planes(v)
    err = (hi.double() + lo.double() - v.double()).abs()
    assert (err <= torch.maximum(2.0 ** -22 * av, torch.full_like(av, 2.0 ** -14))).all()
    assert (err[~big] <= 2.0 ** -14).all()
    assert (err[av >= 2.0 ** 8] <= 2.0 ** -22 * av[av >= 2.0 ** 8]).all()


@pytest.mark.parametrize("M,N,K0", [(512, 1536, 512), (512, 2048, 512)])
def test_three_product_emulation_against_fp64(M, N, K0):
    """lo hi + hi hi + hi lo (fp32 matmul per term, every plane value normal or zero) against fp64: the
    bound of test_linear_split3_fp32_accuracy, < 2e-6 and <= 2.5 x the fp32 matmul's error + 1e-7."""
    gam, bet = rnd(K0, seed=11).abs() + 0.5, rnd(K0, scale=0.3, seed=12)
    y = torch.nn.functional.layer_norm(rnd(M, K0, seed=13) * 3 + 0.5, (K0,), gam, bet, 1e-6)
    w = rnd(N, K0, scale=K0 ** -0.5, seed=14)
    s_a = ops.half2_a_scale(gam, bet)
    ah, al = (p.float() for p in planes(y * s_a))
    _, t = ops.half2_weight(w)
    wh, wl = (p.float() for p in planes(w * t[:, None]))
    cs = 1.0 / (s_a * t)
    out = (al @ wh.T + ah @ wh.T + ah @ wl.T) * cs[None, :]
    ref = y.double() @ w.double().T
    e_h2, e_f32 = rel(out, ref), rel(y @ w.T, ref)
    print(f"half2 emulation {M}x{N}x{K0}: e_h2 {e_h2:.3e} e_f32 {e_f32:.3e} ratio {e_h2 / e_f32:.2f}")
    assert e_h2 < 2e-6, (e_h2, e_f32)
    assert e_h2 <= 2.5 * e_f32 + 1e-7, (e_h2, e_f32)


def test_half2_weight_equals_a_plain_transcription():
    N, K0 = 40, 192
    w = rnd(N, K0, scale=0.05, seed=21)
    w[1] = 0
    w[2] *= 1e-6
    w[3, 5] = 3.0
    w2, t = ops.half2_weight(w)
    assert w2.dtype == torch.float16 and w2.shape == (N, 2 * K0) and t.dtype == torch.float32
    exp = torch.zeros(N, 2 * K0, dtype=torch.float16)
    for n in range(N):
        m = max(abs(float(x)) for x in w[n])
        tn = 1.0 if m == 0 else 2.0 ** (14 - math.floor(math.log2(m)))
        assert float(t[n]) == tn
        for k in range(K0):
            v = torch.tensor(float(w[n, k]) * tn, dtype=torch.float32)
            hi = v.half()
            if abs(float(hi)) < FP16_MIN:
                hi = torch.zeros((), dtype=torch.float16)
            lo = (v - hi.float()).half()
            if abs(float(lo)) < FP16_MIN:
                lo = torch.zeros((), dtype=torch.float16)
            exp[n, 128 * (k // 64) + k % 64] = hi
            exp[n, 128 * (k // 64) + 64 + k % 64] = lo
    assert torch.equal(w2.view(torch.int16), exp.view(torch.int16))
