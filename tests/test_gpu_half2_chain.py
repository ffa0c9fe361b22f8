"""The HALF2 chain on the GPU: the fp16-plane epilogue of mhada_gemm_half2_planes and the fp16-plane batch
attention against ops._half2_planes bit for bit (NaN guards around every buffer), the consuming GEMM at
K0 = 2048 / 512 with a residual on exact operands, its accuracy behind the real producers against fp64,
SPLIT3 and the fp32 MFMA GEMM, and the routing in vit_forward with its switch and its refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from conftest import load_golden
from mhada_hip.recipe import load_recipe, seeded_image

if torch.cuda.is_available():
    from mhada_hip import ops
    DEV = "cuda"
CASE = "full_64_b2"

GUARD = 64


def guarded(shape, dtype):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=dtype)
    return flat, flat[GUARD:GUARD + n].view(*shape)


def guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def ints(shape, lim, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bits16(t):
    return t.contiguous().view(torch.int16)


def col_scales(N, seed):
    """Powers of two 2^-18 .. 2^4 by column: the small ones push hi (and everywhere some lo) below 2^-14."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.exp2((torch.randint(0, 12, (N,), generator=g) * 2 - 18).float()).to(DEV)


# ---- the plane epilogue ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epi_operands():
    cache = {}

    def get(N):
        if N not in cache:
            M, K0 = 300, 128
            s_a = 2.0 ** 10  # |x| < 16: the planes of s_a x stay below 32768
            pl = torch.stack(ops._half2_planes(rnd(M, K0, seed=1).clamp(-7, 7) * 2 * s_a)).contiguous()
            w2, t = ops.half2_weight_dev(rnd(N, K0, scale=K0 ** -0.5, seed=2))
            h = dict(w2=w2, cs=(1.0 / (s_a * t.double())).float().contiguous())
            cache[N] = (pl, h, rnd(N, seed=3), col_scales(N, 4))
        return cache[N]
    return get


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("N", [256, 512])
def test_plane_epilogue_is_half2_planes_of_the_scaled_result(epi_operands, N, with_bias, relu, pad):
    pl, h, bias, osc = epi_operands(N)
    _, M, K0 = pl.shape
    b = bias if with_bias else None
    y = ops.linear_half2(pl, h["w2"], h["cs"], b, torch.float32, relu=relu)  # the existing HALF2 form
    hi, lo = ops._half2_planes(osc[None, :] * y)
    assert (hi == 0).any() and (lo == 0).any() and (hi != 0).any() and (lo != 0).any()
    assert ((hi != 0) & (hi.abs().float() < 2.0 ** -14)).sum() == 0
    ldc2 = N + pad
    with_c = with_bias and not relu  # C is optional: written once, left out otherwise
    flats = []

    def buf(shape, dtype, src=None):
        flat, v = guarded(shape, dtype)
        flats.append(flat)
        if src is not None:
            v.copy_(src)
        return v
    c2 = buf((2, M, ldc2), torch.float16)
    c = buf((M, N), torch.float32)
    ops.gemm(a=buf(pl.shape, torch.float16, pl), w=buf(h["w2"].shape, torch.float16, h["w2"]), c=c if with_c else None,
             M=M, N=N, K=K0, compute=torch.float16, lda=K0, ldw=2 * K0,
             bias=buf((N,), torch.float32, b) if with_bias else None, relu=relu, ldc=N,
             col_scale=buf((N,), torch.float32, h["cs"]), c2=c2, ldc2=ldc2, out_scale=buf((N,), torch.float32, osc))
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in flats)
    assert torch.equal(bits16(c2[0, :, :N]), bits16(hi)) and torch.equal(bits16(c2[1, :, :N]), bits16(lo))
    assert torch.isnan(c2[:, :, N:]).all()
    assert torch.equal(c, y) if with_c else bool(torch.isnan(c).all())
    if pad == 0 and with_bias and relu:  # the op-level route writes the same planes
        m1 = ops.linear_half2(pl, h["w2"], h["cs"], b, torch.float32, relu=True, out_planes=True, out_scale=osc)
        assert torch.equal(bits16(m1), bits16(torch.stack([hi, lo])))


def test_plane_epilogue_refusals():
    a = torch.zeros(2, 64, 64, device=DEV, dtype=torch.float16)
    w = torch.zeros(64, 128, device=DEV, dtype=torch.float16)
    cs = torch.ones(64, device=DEV)
    c2 = torch.zeros(2, 64, 64, device=DEV, dtype=torch.float16)
    kw = dict(a=a, w=w, c=None, M=64, K=64, compute=torch.float16, lda=64, ldw=128, ldc=64, col_scale=cs, c2=c2,
              out_scale=cs)
    with pytest.raises(ValueError, match="half2_planes"):
        ops.gemm(N=62, ldc2=64, **kw)  # N % 4
    with pytest.raises(ValueError, match="half2_planes"):
        ops.gemm(N=64, ldc2=32, **kw)  # ldc2 < N
    with pytest.raises(ValueError, match="out_scale"):
        ops.gemm(N=64, ldc2=64, **{**kw, "c2": c2.bfloat16()})
    ops.gemm(N=64, ldc2=64, **kw)
    torch.cuda.synchronize()
    assert (c2 == 0).all()


# ---- the batch-axis attention ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 8])
def test_batch_attention_planes_are_half2_planes_of_the_scaled_fp32_output(L):
    ntok, heads, C = 70, 8, 512
    qkv = rnd(L, ntok, 3 * C, seed=10 + L)
    osc = col_scales(C, 20 + L)
    hi, lo = ops._half2_planes(osc[None, :] * ops.vit_batch_attn(qkv, L, ntok, heads).view(L * ntok, C))
    assert (hi == 0).any() and (lo == 0).any() and (hi != 0).any() and (lo != 0).any()
    n = L * ntok * C
    flat, pl = guarded((2, L * ntok, C), torch.float16)
    fo, ob = guarded((C,), torch.float32)
    ob.copy_(osc)
    ops._call("mhada_vit_batch_attn_half2", qkv, qkv.data_ptr(), pl.data_ptr(), n, ob.data_ptr(), L, ntok, heads, 64)
    torch.cuda.synchronize()
    assert guards_intact(flat) and guards_intact(fo)
    assert torch.equal(bits16(pl[0]), bits16(hi)) and torch.equal(bits16(pl[1]), bits16(lo))
    got = ops.vit_batch_attn_half2(qkv, L, ntok, heads, osc)
    assert torch.equal(bits16(got), bits16(pl))


def test_batch_attention_refuses_what_the_split3_form_refuses():
    ntok = 8
    osc = torch.ones(128, device=DEV)
    with pytest.raises(ValueError):
        ops.vit_batch_attn_half2(rnd(9, ntok, 3 * 128, seed=1), 9, ntok, 2, osc)      # L > 8
    with pytest.raises(ValueError):
        ops.vit_batch_attn_half2(rnd(2, ntok, 3 * 128, seed=1), 2, ntok, 1, osc)      # head_dim 128
    with pytest.raises(ValueError):
        ops.vit_batch_attn_half2(rnd(2, ntok, 3 * 128, seed=1), 2, ntok, 4, osc)      # head_dim 32
    with pytest.raises(ValueError):
        ops.vit_batch_attn_half2(rnd(2, ntok, 3 * 128, seed=1).bfloat16(), 2, ntok, 2, osc)
    qkv = rnd(2, ntok, 3 * 128, seed=1)
    pl = torch.zeros(2, 2 * ntok, 128, device=DEV, dtype=torch.float16)
    with pytest.raises(ValueError, match="plane stride"):
        ops._call("mhada_vit_batch_attn_half2", qkv, qkv.data_ptr(), pl.data_ptr(), 2 * ntok * 128 - 1, osc.data_ptr(),
                  2, ntok, 2, 64)
    for L in (9, 0):
        with pytest.raises(ValueError):
            ops._call("mhada_vit_batch_attn_split3", qkv, qkv.data_ptr(), pl.data_ptr(), 2 * ntok * 128, L, ntok, 2, 64)
        with pytest.raises(ValueError):
            ops._call("mhada_vit_batch_attn_half2", qkv, qkv.data_ptr(), pl.data_ptr(), 2 * ntok * 128, osc.data_ptr(),
                      L, ntok, 2, 64)


# ---- the consumers --------------------------------------------------------------------------------------
def consume(a_hi, a_lo, w_hi, w_lo, cs, bias, res):
    """ops.linear_half2_planes on explicit planes (fp64 tensors holding fp16-exact values), guarded."""
    M, K0 = a_hi.shape
    N = w_hi.shape[0]
    fa, a = guarded((2, M, K0), torch.float16)
    a[0], a[1] = a_hi.to(DEV, torch.float16), a_lo.to(DEV, torch.float16)
    fw, w = guarded((N, K0 // 64, 2, 64), torch.float16)
    w[:, :, 0] = w_hi.view(N, K0 // 64, 64).to(DEV, torch.float16)
    w[:, :, 1] = w_lo.view(N, K0 // 64, 64).to(DEV, torch.float16)
    out = ops.linear_half2_planes(a, w.view(N, 2 * K0), cs.float().to(DEV), None if bias is None else bias.float().to(DEV),
                                  residual=None if res is None else res.float().to(DEV))
    torch.cuda.synchronize()
    assert guards_intact(fa) and guards_intact(fw)
    return out


@pytest.mark.parametrize("K0,with_res", [(2048, True), (128, True), (128, False)])
def test_consumer_on_integer_operands_gives_the_fp64_bits(K0, with_res):
    """32 K chunks (MLP2's depth) once: the counted waits and the ring slots of the staging hold over a long
    K loop; |x| <= 1024, |w| <= 2: every sum below 2^23."""
    M, N = 300, 512
    x, w = ints((M, K0), 1024, 31), ints((N, K0), 2, 32)
    x[0, 0], x[M - 1, K0 - 1] = 1024, -1024
    cs = torch.exp2(-(torch.arange(N) % 4).double())
    bias = ((torch.arange(N) % 13) - 6).double() / 8
    res = ints((M, N), 100, 33) if with_res else None
    ref = (x.to(DEV) @ w.to(DEV).T).cpu() * cs[None, :] + bias[None, :]
    if with_res:
        ref = ref + res
    assert torch.equal(ref.float().double(), ref)
    out = consume(x, torch.zeros_like(x), w, torch.zeros_like(w), cs, bias, res)
    assert torch.equal(out.cpu(), ref.float())


@pytest.mark.parametrize("which", ["a_lo", "w_lo"])
def test_consumer_dyadic_lo_planes_decide_bits(which):
    M, N, K0 = 300, 512, 128
    hi_a, hi_w = ints((M, K0), 32, 41), ints((N, K0), 4, 42)
    lo_a, lo_w = torch.zeros(M, K0).double(), torch.zeros(N, K0).double()
    if which == "a_lo":
        lo_a = ints((M, K0), 8, 43) / 64
    else:
        lo_w = ints((N, K0), 8, 44) / 64
    res = ints((M, N), 100, 45)
    ref = (hi_a + lo_a) @ (hi_w + lo_w).T + res
    assert not torch.equal(ref, hi_a @ hi_w.T + res) and torch.equal(ref.float().double(), ref)
    out = consume(hi_a, lo_a, hi_w, lo_w, torch.ones(N), None, res)
    assert torch.equal(out.cpu(), ref.float())


# ---- accuracy behind the real producers -----------------------------------------------------------------
def report(name, out, out_s3, out_f32, ref):
    e, e3, e32 = rel(out, ref), rel(out_s3, ref), rel(out_f32, ref)
    print(f"half2 chain {name}: e_chain {e:.3e} e_split3 {e3:.3e} e_f32 {e32:.3e} "
          f"ratio to SPLIT3 {e / e3:.2f}, to the fp32 MFMA GEMM {e / e32:.2f}")
    assert e < 2e-6, (e, e3, e32)              # the bound of test_linear_split3_fp32_accuracy
    assert e <= 2.5 * e32 + 1e-7, (e, e3, e32)


def test_mlp2_accuracy_behind_the_real_mlp1():
    M, C, H = 512, 512, 2048
    x = rnd(M, C, seed=51) * 2
    g, be = rnd(C, seed=52).abs() + 0.5, rnd(C, scale=0.3, seed=53)
    w1, b1 = rnd(H, C, scale=C ** -0.5, seed=54), rnd(H, seed=55)
    w2, b2, r = rnd(C, H, scale=H ** -0.5, seed=56), rnd(C, seed=57), rnd(M, C, seed=58)
    h1, hc = ops.half2_prepare(g, be, w1), ops.half2_chain_prepare(g, be, w1, b1, w2)
    assert h1 is not None and hc is not None
    pl = ops.layernorm_half2(x, g, be, 1e-6, h1["s_a"])
    a = ops.linear_half2(pl, h1["w2"], h1["cs"], b1, torch.float32, relu=True)  # what MLP2 multiplies, in fp32
    m1 = ops.linear_half2(pl, h1["w2"], h1["cs"], b1, torch.float32, relu=True, out_planes=True, out_scale=hc["u"])
    assert (m1.float().abs() <= 32768).all()
    hi, lo = ops._half2_planes(hc["u"][None, :] * a)
    assert torch.equal(bits16(m1), bits16(torch.stack([hi, lo])))
    out = ops.linear_half2_planes(m1, hc["w2"], hc["cs"], b2, residual=r)
    assert torch.equal(out, ops.linear_half2_planes(m1, hc["w2"], hc["cs"], b2, residual=r))
    m3 = ops.linear_half2(pl, h1["w2"], h1["cs"], b1, torch.float32, relu=True, out_planes=True)
    out_s3 = ops.linear_split3(m3, ops.split3_weight(w2), b2, torch.float32, residual=r)
    ref = a.double() @ w2.double().T + b2.double() + r.double()
    report("MLP2 512x512x2048", out, out_s3, ops.linear(a, w2, b2, torch.float32, residual=r), ref)


def test_out_projection_accuracy_behind_the_real_attention():
    L, ntok, heads, C = 8, 64, 8, 512
    x = rnd(L * ntok, C, seed=61) * 2
    g, be = rnd(C, seed=62).abs() + 0.5, rnd(C, scale=0.3, seed=63)
    wq, bq = rnd(3 * C, C, scale=C ** -0.5, seed=64), rnd(3 * C, scale=0.3, seed=65)
    wo, bo, r = rnd(C, C, scale=C ** -0.5, seed=66), rnd(C, seed=67), rnd(L * ntok, C, seed=68)
    hq = ops.half2_prepare(g, be, wq)
    hc = ops.half2_chain_prepare(g, be, wq[2 * C:], bq[2 * C:], wo)
    assert hq is not None and hc is not None
    qkv = ops.linear_half2(ops.layernorm_half2(x, g, be, 1e-6, hq["s_a"]), hq["w2"], hq["cs"], bq, torch.float32)
    qkv = qkv.view(L, ntok, 3 * C)
    att = ops.vit_batch_attn(qkv, L, ntok, heads).view(L * ntok, C)
    pl = ops.vit_batch_attn_half2(qkv, L, ntok, heads, hc["u"])
    assert (pl.float().abs() <= 32768).all()
    out = ops.linear_half2_planes(pl, hc["w2"], hc["cs"], bo, residual=r)
    out_s3 = ops.linear_split3(ops.vit_batch_attn_split3(qkv, L, ntok, heads), ops.split3_weight(wo), bo, torch.float32,
                               residual=r)
    ref = att.double() @ wo.double().T + bo.double() + r.double()
    report("out-projection 512x512x512", out, out_s3, ops.linear(att, wo, bo, torch.float32, residual=r), ref)


# ---- routing --------------------------------------------------------------------------------------------
def models():
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(activation="softmax"), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = torch.float32
    return vc, vs, ada


def stylize(ms, c, s):
    vc, vs, ada = ms
    with torch.no_grad():
        fc, fs = vc(c), vs(s)
        fcs, cs = ada(fc, fs)
    return fc, fs, fcs, cs


def bits(ts):
    return [t.contiguous().view(torch.int32).clone() for t in ts]


def inputs():
    g = load_golden(CASE)
    c = seeded_image(*map(int, g["content_shape"]), int(g["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, g["style_shape"]), int(g["seeds"][1])).to(DEV)
    return g, c, s


NEW_ENTRIES = ("mhada_gemm_half2_planes", "mhada_vit_batch_attn_half2")


@pytest.fixture()
def routed(monkeypatch):
    """The SPLIT3 routing rule forced on (as test_gpu_vit_half2 does), both halves of the chain on; calls of ops.linear_half2_planes and
    launches of the new entries counted."""
    from mhada_hip import engine
    monkeypatch.setattr(engine, "_split3_fills", lambda M, N, dev: True)
    monkeypatch.setattr(ops, "F32_SPLIT_ATTN", True)
    monkeypatch.setattr(ops, "F32_HALF2", True)
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN_OUTPROJ", True)  # both halves of the chain (the default: MLP2 only)
    calls = {"planes": 0, "entries": 0}
    lin, call = ops.linear_half2_planes, ops._call

    def lin_(*a, **k):
        calls["planes"] += 1
        return lin(*a, **k)

    def call_(name, *a, **k):
        calls["entries"] += name in NEW_ENTRIES
        return call(name, *a, **k)
    monkeypatch.setattr(ops, "linear_half2_planes", lin_)
    monkeypatch.setattr(ops, "_call", call_)
    return calls


def test_chain_route_meets_the_goldens_and_off_is_the_previous_route(routed, monkeypatch):
    g, c, s = inputs()
    ms = models()
    nlayers = len(ms[0].encoder) + len(ms[1].encoder)
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN", True)
    fc, fs, fcs, cs = stylize(ms, c, s)
    assert routed["planes"] == 2 * nlayers and routed["entries"] == 2 * nlayers  # MLP2 and the out-projection
    csn = cs.cpu().numpy()
    a, b = np.clip(csn, 0, 255) / 255.0, np.clip(g["cs"], 0, 255) / 255.0
    assert float(((a.astype(np.float64) - b) ** 2).mean()) < 1e-4
    assert float(((csn.astype(np.float64) - g["cs"]) ** 2).mean()) < 1e-4
    np.testing.assert_allclose(fcs.cpu().numpy(), g["fcs"], rtol=1e-3, atol=2e-3)
    for i in (0, 2):
        np.testing.assert_allclose(fc[i].cpu().numpy(), g[f"fc{i}"], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(fs[i].cpu().numpy(), g[f"fs{i}"], rtol=1e-3, atol=1e-3)
    on = bits(list(fc) + list(fs) + [fcs, cs])

    # the out-projection's own switch off (the default): MLP2 alone takes the chain, once per layer
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN_OUTPROJ", False)
    routed["planes"] = routed["entries"] = 0
    stylize(ms, c, s)
    assert routed["planes"] == nlayers and routed["entries"] == nlayers
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN_OUTPROJ", True)

    monkeypatch.setattr(ops, "F32_HALF2_CHAIN", False)
    routed["planes"] = routed["entries"] = 0
    off_out = stylize(ms, c, s)
    assert routed["planes"] == 0 and routed["entries"] == 0
    off = bits(list(off_out[0]) + list(off_out[1]) + list(off_out[2:]))
    fresh_out = stylize(models(), c, s)
    assert routed["planes"] == 0 and routed["entries"] == 0
    fresh = bits(list(fresh_out[0]) + list(fresh_out[1]) + list(fresh_out[2:]))
    assert all(torch.equal(x, y) for x, y in zip(off, fresh))
    assert any(not torch.equal(x, y) for x, y in zip(on, off))


def test_a_layer_whose_bound_leaves_the_window_keeps_split3_for_mlp2(routed, monkeypatch):
    from mhada_hip import engine
    _, c, _ = inputs()
    vc = models()[0]
    with torch.no_grad():
        vc.encoder[1].mlp[0].weight.mul_(2.0 ** 60)  # Z ~ 2^60: u would be below 2^-40
    monkeypatch.setattr(ops, "F32_HALF2_CHAIN", True)
    with torch.no_grad():
        vc(c)
    layers = engine.vit_prep(vc, torch.float32)["layers"]
    assert layers[1]["w2_half2"] is None and layers[1]["w_o_half2"] is not None
    assert all(L["w2_half2"] is not None and L["w_o_half2"] is not None for i, L in enumerate(layers) if i != 1)
    assert routed["planes"] == 2 * len(layers) - 1
