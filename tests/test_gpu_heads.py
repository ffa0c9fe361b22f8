"""4- and 16-head MHAda models (head_dim 128 / 32) on the GPU: the D-wide kernels of csrc/attn_hd.hip
against fp64, the head-count goldens of the reference, the style cache, the video stylizer and the
graphed call.  Tolerances are the project's own (test_gpu_kernels.py / test_gpu_parity.py)."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import network
    from mhada_hip import _lib, ops, video
    from mhada_hip.recipe import load_recipe, seeded_image
    DEV = "cuda"


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


# fp32 compute: exact-fp32 MFMA, only summation order differs -> 1e-5; bf16 operands -> 1e-2
TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}
DTS = [torch.float32, torch.bfloat16]
WIDTHS = [32, 128]


def _attn_ref(q, kv, fcs, mu, rstd, v_mu, dtype=torch.float64):
    """mhada_attn_hd's header formula (K carries log2(e): the natural-unit logit is (q.k) ln 2) in
    ``dtype``: fp64 is the reference, fp32 the plain aten yardstick."""
    B, H, Nc, D = q.shape
    qd, kd, vd = q.to(dtype), kv[..., :D].to(dtype), kv[..., D:].to(dtype)
    a = torch.softmax(qd @ kd.transpose(-1, -2) * math.log(2.0), dim=-1)
    m = a @ vd
    e2 = a @ (vd * vd)
    s = torch.sqrt(torch.clamp(e2 - m * m, min=1e-6))
    out = s.permute(0, 2, 1, 3).reshape(B, Nc, H * D)
    mm = m.permute(0, 2, 1, 3).reshape(B, Nc, H * D)
    f = (fcs.to(dtype) - mu.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    return out * f + mm + v_mu.to(dtype)[:, None]


def _log(line):
    """Measured figures go to the file named by MHADA_HD_ERR_LOG (unset: printed only)."""
    print(line)
    path = os.environ.get("MHADA_HD_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,H,Nc,Ns", [(1, 2, 256, 64), (2, 3, 300, 100), (1, 2, 97, 33), (1, 4, 513, 128),
                                       (2, 2, 1000, 777), (1, 2, 64, 4096), (1, 1, 3000, 192)])
def test_attn_hd_vs_fp64(dt, D, B, H, Nc, Ns):
    """mhada_attn_hd against fp64 on the same operands: one whole tile, ragged tiles, Ns below one
    tile with a partial query block, many tiles, more query blocks than one (b, h)'s share of CUs.
    Operands scaled by 0.5 (64/D)^(1/4): the logit standard deviation of the 64-wide scale-0.5 cases."""
    sc = 0.5 * (64.0 / D) ** 0.25
    C = H * D
    q = (rnd(B, H, Nc, D, seed=21) * sc).to(dt)
    kv = (rnd(B, H, Ns, 2 * D, seed=22) * sc).to(dt)
    fcs = rnd(B, Nc, C, seed=23)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, C, seed=24)
    y = ops.attn_hd(q, kv, fcs, mu, rs, vmu, _lib.ACT_SOFTMAX)
    y2 = ops.attn_hd(q, kv, fcs, mu, rs, vmu, _lib.ACT_SOFTMAX)
    ref = _attn_ref(q.float(), kv.float(), fcs, mu, rs, vmu)
    err = rel(y.float(), ref)
    if dt == torch.float32:
        aten = rel(_attn_ref(q, kv, fcs, mu, rs, vmu, torch.float32), ref)
        _log(f"attn_hd fp32 D={D} B={B} H={H} Nc={Nc} Ns={Ns}: kernel {err:.3e} aten-fp32 {aten:.3e} "
             f"ratio {err / aten:.2f}")
    else:
        _log(f"attn_hd bf16 D={D} B={B} H={H} Nc={Nc} Ns={Ns}: kernel {err:.3e}")
    assert y.shape == (B, Nc, C) and y.dtype == dt
    assert torch.isfinite(y.float()).all()
    assert err < TOL[dt]
    assert torch.equal(y, y2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("Nc,Ns", [(300, 700), (97, 33), (256, 1024)])
def test_attn_hd_late_max_jump(dt, D, Nc, Ns):
    """A key in the last key tile far above every earlier score (test_mhada_attn_late_max_jump's
    construction with 64 -> D): the deferred rescale must fire late and leave finite, exact sums."""
    B, H = 1, 8
    q = rnd(B, H, Nc, D, seed=11)
    q = q / q.norm(dim=-1, keepdim=True) * 4.0
    kv = rnd(B, H, Ns, 2 * D, scale=0.1, seed=12)
    late = Ns - 5  # in the last key tile
    kv[:, :, late, :D] = 30.0 * q[:, :, : min(Nc, 1), :].mean(dim=2)
    kv[:, :, late - 1, :D] = -kv[:, :, late, :D]
    q, kv = q.to(dt), kv.to(dt)
    fcs = rnd(B, Nc, H * D, seed=13)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, H * D, seed=14)
    y = ops.attn_hd(q, kv, fcs, mu, rs, vmu, _lib.ACT_SOFTMAX)
    ref = _attn_ref(q.float(), kv.float(), fcs, mu, rs, vmu)
    err = rel(y.float(), ref)
    _log(f"attn_hd late jump {dt} D={D} Nc={Nc} Ns={Ns}: {err:.3e}")
    assert torch.isfinite(y.float()).all()
    assert err < (1e-5 if dt == torch.float32 else 1.5e-2)


def _rownorm64(x):
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,H,Nc,Ns", [(2, 2, 300, 100), (1, 2, 97, 384)])
def test_cosine_hd_vs_fp64(dt, D, B, H, Nc, Ns):
    """cosine_prep_hd + attn_hd(ACT_COSINE) against fp64 of adaDecoder.py:20-34 on the operands before
    the normalisation: A = (q^ . k^ + 1) / rowsum."""
    C = H * D
    q = rnd(B, H, Nc, D, seed=1, dtype=dt)
    kv = rnd(B, H, Ns, 2 * D, seed=2, dtype=dt)
    fcs = rnd(B, Nc, C, seed=3)
    mu = rnd(B, C, seed=4, scale=0.1)
    rs = rnd(B, C, seed=5).abs() + 0.5
    vmu = rnd(B, C, seed=6)
    qd, kd, vd = _rownorm64(q), _rownorm64(kv[..., :D]), kv[..., D:].double()
    ops.cosine_prep_hd(q, kv)
    out = ops.attn_hd(q, kv, fcs, mu, rs, vmu, _lib.ACT_COSINE)
    a = qd @ kd.transpose(-1, -2) + 1
    a = a / a.sum(-1, keepdim=True)
    m = a @ vd
    e2 = a @ (vd * vd)
    s = torch.sqrt((e2 - m * m).clamp(min=1e-6))
    x = (fcs.double().view(B, Nc, H, D).permute(0, 2, 1, 3) - mu.double().view(B, H, 1, D)) * \
        rs.double().view(B, H, 1, D)
    ref = (s * x + m + vmu.double().view(B, H, 1, D)).permute(0, 2, 1, 3).reshape(B, Nc, C)
    err = rel(out.float(), ref)
    _log(f"cosine hd {dt} D={D} B={B} H={H} Nc={Nc} Ns={Ns}: {err:.3e}")
    assert torch.isfinite(out.float()).all()
    assert err < TOL[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", WIDTHS)
def test_cosine_prep_hd_rows(dt, D):
    """Row normalisation alone, one side at a time (Nc = 0 / Ns = 0): the other tensor and the V'
    half of kv stay untouched."""
    B, H, Nc, Ns = 2, 3, 37, 53
    q0 = rnd(B, H, Nc, D, seed=7, dtype=dt)
    kv0 = rnd(B, H, Ns, 2 * D, seed=8, dtype=dt)
    q, kv = q0.clone(), kv0.clone()
    ops.cosine_prep_hd(q, None)  # Ns = 0
    assert rel(q.float(), _rownorm64(q0)) < (1e-6 if dt == torch.float32 else 4e-3)
    ops.cosine_prep_hd(None, kv)  # Nc = 0
    assert rel(kv[..., :D].float(), _rownorm64(kv0[..., :D])) < (1e-6 if dt == torch.float32 else 4e-3)
    assert torch.equal(kv[..., D:], kv0[..., D:])
    with pytest.raises(ValueError):
        ops.cosine_prep_hd(rnd(1, 1, 4, 64, dtype=dt), None)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", WIDTHS)
def test_fold_block_hd(dt, D, H):
    """The four header formulas in fp64; bf16 outputs against the bf16 rounding of the fp64 value
    (the kernel rounds an fp32 product: at most one bf16 ulp apart, and an ulp is at most 2^-7 of the value)."""
    B, C, ks = 2, H * D, 1.4426950408889634
    wf, wg, wh = (rnd(H, D, D, seed=30 + i, scale=D ** -0.5) for i in range(3))
    bg, bh = rnd(H, D, seed=33), rnd(H, D, seed=34)
    rc, rs = rnd(B, C, seed=35).abs() + 0.5, rnd(B, C, seed=36).abs() + 0.5
    ms = rnd(B, C, seed=37)
    wq, wkv, bkv, v_mu = ops.fold_block_hd(wf, wg, wh, bg, bh, rc, ms, rs, dt, ks)
    assert wq.shape == (B, H, D, D) and wkv.shape == (B, H, 2 * D, D) and bkv.shape == (H, 2 * D)
    r_wq = wf.double()[None] * rc.double().view(B, H, 1, D)
    r_wk = wg.double()[None] * rs.double().view(B, H, 1, D) * ks
    r_wkv = torch.cat([r_wk, wh.double()[None].expand(B, H, D, D)], dim=2)
    r_bkv = torch.cat([bg.double() * ks, torch.zeros(H, D, device=DEV, dtype=torch.float64)], dim=1)
    r_vmu = (torch.einsum("hoc,bhc->bho", wh.double(), ms.double().view(B, H, D)) + bh.double()).reshape(B, C)
    if dt == torch.float32:
        assert rel(wq, r_wq) < TOL[dt] and rel(wkv, r_wkv) < TOL[dt]
    else:
        for got, want in ((wq, r_wq), (wkv, r_wkv)):
            w16 = want.float().bfloat16().double()
            assert ((got.double() - w16).abs() <= 2.0 ** -7 * w16.abs()).all()
    assert rel(bkv, r_bkv) < TOL[torch.float32] and rel(v_mu, r_vmu) < TOL[torch.float32]
    with pytest.raises(ValueError):
        ops.fold_block_hd(*(rnd(H, 64, 64, seed=1),) * 3, rnd(H, 64), rnd(H, 64), rnd(B, H * 64), rnd(B, H * 64),
                          rnd(B, H * 64), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("heads", [2, 5])
@pytest.mark.parametrize("ntok", [1, 63, 1000])
@pytest.mark.parametrize("L", [1, 2, 5, 8, 11])
@pytest.mark.parametrize("D", WIDTHS)
def test_vit_batch_attn_hd(dt, D, L, ntok, heads):
    """mhada_vit_batch_attn at head_dim 32 / 128 against multi_head_attention_forward's semantics in
    fp64: softmax over the batch axis, scale 1/sqrt(D)."""
    C = heads * D
    qkv = rnd(L, ntok, 3 * C, seed=L + ntok, dtype=dt)
    att = ops.vit_batch_attn(qkv, L, ntok, heads)
    q, k, v = (t.double().view(L, ntok, heads, D).permute(1, 2, 0, 3) for t in qkv.split(C, dim=-1))
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1)
    ref = (a @ v).permute(2, 0, 1, 3).reshape(L, ntok, C)
    assert att.shape == (L, ntok, C) and att.dtype == dt
    assert rel(att.float(), ref) < TOL[dt]


def test_vit_batch_attn_rejects_other_widths():
    with pytest.raises(ValueError, match="32, 64 or 128"):
        ops.vit_batch_attn(rnd(2, 8, 3 * 96), 2, 8, 2)  # head_dim 48


# ---- reference goldens ----------------------------------------------------------------------
def models(heads, act="softmax", dtype=torch.float32):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads, activation=act), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = dtype
    return vc, vs, ada


def stylize(ms, c, s):
    vc, vs, ada = ms
    with torch.no_grad():
        return ada(vc(c), vs(s))


def mse01(a, b):
    a = np.clip(np.asarray(a, dtype=np.float64), 0, 255) / 255.0
    b = np.clip(np.asarray(b, dtype=np.float64), 0, 255) / 255.0
    return float(((a - b) ** 2).mean())


@pytest.mark.parametrize("case", ["block_h4_b2_4x4_s3x5", "block_h16_b2_4x4_s3x5", "block_cos_h16_b1_4x4"])
def test_block_matches_reference_goldens_heads(case):
    g = load_golden(case)
    blk = load_recipe(network.AdaAttnMultiHead(512, int(g["heads"]), str(g["activation"])), "blk").to(DEV).eval()
    blk.compute_dtype = torch.float32
    with torch.no_grad():
        out = blk(*(torch.from_numpy(g[k]).to(DEV) for k in ("fc", "fs", "fcs")))
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("case", ["full_64_b2_h4", "full_64_b2_h16", "full_64x128_s64_b1_h16"])
def test_forward_matches_reference_goldens_heads(case, dtype):
    g = load_golden(case)
    cshape, sshape, seeds = g["content_shape"], g["style_shape"], g["seeds"]
    c = seeded_image(*map(int, cshape), int(seeds[0])).to(DEV)
    s = seeded_image(*map(int, sshape), int(seeds[1])).to(DEV)
    fcs, cs = stylize(models(int(g["heads"]), str(g["activation"]), dtype), c, s)
    cs = cs.cpu().numpy()
    assert cs.shape == g["cs"].shape
    assert mse01(cs, g["cs"]) < 1e-4
    if dtype == torch.float32:
        assert float(((cs.astype(np.float64) - g["cs"].astype(np.float64)) ** 2).mean()) < 1e-4
        np.testing.assert_allclose(fcs.cpu().numpy(), g["fcs"], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("dtype", DTS)
def test_style_cache_with_16_heads(dtype):
    """Same fs objects: a hit (the cached sides are kept) with bit-identical cs; fs changed in place:
    a miss; VideoStylizer over two frames equals the uncached calls bit for bit."""
    vc, vs, ada = models(16, dtype=dtype)
    style = seeded_image(1, 64, 64, 1).to(DEV)
    frames = [seeded_image(1, 72, 128, 2 + i).to(DEV) for i in range(2)]
    with torch.no_grad():
        fs = vs(style)
        fc = vc(frames[0])
        _, cs1 = ada(fc, fs)
        sides = ada.__dict__["_mhada_style"]["sides"]
        assert all("kv" in sd and sd["kv"].shape[-1] == 64 for sd in sides)
        _, cs2 = ada(fc, fs)
        assert ada.__dict__["_mhada_style"]["sides"] is sides  # hit
        assert torch.equal(cs1, cs2)
        fs[0].mul_(1.0)  # in-place write: the version counter moves
        _, cs3 = ada(fc, fs)
        assert ada.__dict__["_mhada_style"]["sides"] is not sides  # miss
        assert torch.equal(cs1, cs3)
    st = video.VideoStylizer(vc, vs, ada)
    st.set_style(style)
    outs = [st(f) for f in frames]
    ada.cache_style = False
    for f, o in zip(frames, outs):
        _, cs = stylize((vc, vs, ada), f, style)
        assert torch.equal(o, cs.clamp(0, 255))


@pytest.mark.parametrize("dtype", DTS)
def test_graphed_stylizer_with_4_heads(dtype):
    from mhada_hip.graphs import GraphedStylizer
    ms = models(4, dtype=dtype)
    g = GraphedStylizer(*ms, (2, 3, 64, 96))
    for seed in (3, 5):
        c = seeded_image(2, 64, 96, seed).to(DEV)
        s = seeded_image(2, 64, 96, seed + 1).to(DEV)
        ref = stylize(ms, c, s)[1].clamp(0, 255)
        out = g(c, s)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_unsupported_head_width_raises():
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=2), "ada").to(DEV).eval()  # head_dim 256
    vc, vs, _ = models(8)
    c = seeded_image(1, 64, 64, 1).to(DEV)
    with torch.no_grad():
        fc, fs = vc(c), vs(c)
        with pytest.raises(ValueError, match=r"\{32, 64, 128\}"):
            ada(fc, fs)
