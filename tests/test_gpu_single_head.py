"""The single-head AdaAttN stack (head width 512) on the GPU: ``mhada_attn_wide`` (csrc/attn_wide.hip) and
the fp32 route (``mhada_loss_attn`` at d_qk = d_v = 512) against fp64 on the same rounded operands, the
reference's single-head goldens (tests/golden/make_goldens_single.py) through ``network.AdaAttN`` /
``network.AdaAttnTransformer`` in both dtypes, and the routing.  Tolerances are those of test_gpu_heads.py."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import network
    from mhada_hip import _lib, engine, ops
    from mhada_hip.recipe import load_recipe, seeded_image
    DEV = "cuda"

D = 512
TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}  # test_gpu_heads.py's
DTS = [torch.float32, torch.bfloat16]
# one whole tile; ragged queries with keys below a tile; several of both; one key past a key-tile boundary;
# many key tiles; 17 query blocks of 64 and one query (more than one XCD's share, the last block one query)
SHAPES = [(1, 64, 64), (2, 97, 33), (2, 300, 100), (1, 130, 257), (1, 64, 2048), (1, 1089, 192)]
SC = 0.5 * (64.0 / D) ** 0.25  # the logit spread of the other width tests


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


def _attn_ref(q, k, v, fcs, mu, rstd, v_mu, log2_units):
    """The header formula in fp64 (``_attn_ref`` of test_gpu_heads.py with H = 1, D = 512).  log2_units: q
    carries log2(e), the natural-unit logit is (q.k) ln 2 (mhada_attn_wide); otherwise q.k (mhada_loss_attn)."""
    qd, kd, vd = q.double(), k.double(), v.double()
    a = torch.softmax(qd @ kd.transpose(-1, -2) * (math.log(2.0) if log2_units else 1.0), dim=-1)
    m = a @ vd
    s = torch.sqrt(torch.clamp(a @ (vd * vd) - m * m, min=1e-6))
    f = (fcs.double() - mu.double()[:, None]) * rstd.double()[:, None]
    return s * f + m + v_mu.double()[:, None]


def _log(line):
    """Measured figures go to the file named by MHADA_WIDE_ERR_LOG (unset: printed only)."""
    print(line)
    path = os.environ.get("MHADA_WIDE_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("B,Nc,Ns", SHAPES)
def test_attn_wide_vs_fp64(B, Nc, Ns):
    q = (rnd(B, Nc, D, seed=21) * SC).to(torch.bfloat16)
    k = (rnd(B, Ns, D, seed=22) * SC).to(torch.bfloat16)
    v = (rnd(B, Ns, D, seed=25) * SC).to(torch.bfloat16)
    fcs = rnd(B, Nc, D, seed=23)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, D, seed=24)
    y, y16 = ops.attn_wide(q, k, v, fcs, mu, rs, vmu, want_bf16=True)
    y2 = ops.attn_wide(q, k, v, fcs, mu, rs, vmu)
    ref = _attn_ref(q, k, v, fcs, mu, rs, vmu, True)
    err = rel(y, ref)
    _log(f"attn_wide bf16 B={B} Nc={Nc} Ns={Ns}: kernel {err:.3e}")
    assert y.shape == (B, Nc, D) and y.dtype == torch.float32 and y16.dtype == torch.bfloat16
    assert torch.isfinite(y).all()
    assert err < TOL[torch.bfloat16]
    assert torch.equal(y, y2)
    assert torch.equal(y16, y.to(torch.bfloat16))


@pytest.mark.parametrize("Nc,Ns", [(97, 33), (300, 700)])
def test_attn_wide_late_max_jump(Nc, Ns):
    """test_attn_hd_late_max_jump's construction at D = 512: a key in the last key tile far above every earlier
    score; the deferred rescale must fire late and leave finite, exact sums."""
    B = 1
    q = rnd(B, Nc, D, seed=11)
    q = q / q.norm(dim=-1, keepdim=True) * 4.0
    k = rnd(B, Ns, D, scale=0.1, seed=12)
    v = rnd(B, Ns, D, scale=0.1, seed=15)
    late = Ns - 5  # in the last key tile
    k[:, late] = 30.0 * q[:, : min(Nc, 1)].mean(dim=1)
    k[:, late - 1] = -k[:, late]
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    fcs = rnd(B, Nc, D, seed=13)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, D, seed=14)
    y = ops.attn_wide(q, k, v, fcs, mu, rs, vmu)
    err = rel(y, _attn_ref(q, k, v, fcs, mu, rs, vmu, True))
    _log(f"attn_wide late jump Nc={Nc} Ns={Ns}: {err:.3e}")
    assert torch.isfinite(y).all()
    assert err < 1.5e-2


@pytest.mark.parametrize("B,Nc,Ns", SHAPES)
def test_loss_attn_at_512_vs_fp64(B, Nc, Ns):
    """The fp32 route of the single-head block: mhada_loss_attn at d_qk = d_v = 512 (natural-unit logits)."""
    q, k, v = rnd(B, Nc, D, seed=21) * SC, rnd(B, Ns, D, seed=22) * SC, rnd(B, Ns, D, seed=25) * SC
    fcs = rnd(B, Nc, D, seed=23)
    mu, rs = ops.instnorm_stats(fcs)
    y = ops.loss_attn(q, k, v, fcs, mu, rs, _lib.ACT_SOFTMAX)
    err = rel(y, _attn_ref(q, k, v, fcs, mu, rs, torch.zeros(B, D, device=DEV), False))
    _log(f"loss_attn fp32 512/512 B={B} Nc={Nc} Ns={Ns}: kernel {err:.3e}")
    assert torch.isfinite(y).all()
    assert err < TOL[torch.float32]


def test_attn_wide_wrapper_validates():
    q, k, v = (torch.zeros(1, 8, D, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    fcs = torch.zeros(1, 8, D, device=DEV)
    st = torch.zeros(1, D, device=DEV)
    with pytest.raises(ValueError, match="head width must be 512"):
        ops.attn_wide(q[..., :256].contiguous(), k, v, fcs, st, st, st)
    with pytest.raises(ValueError, match="contiguous bfloat16"):
        ops.attn_wide(q.float(), k, v, fcs, st, st, st)
    with pytest.raises(ValueError, match="contiguous bfloat16"):
        ops.attn_wide(q, k.transpose(1, 2).contiguous().transpose(1, 2), v, fcs, st, st, st)  # strided k
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.attn_wide(q, k, v, fcs, st[:, :256], st, st)


# ---- reference goldens ----------------------------------------------------------------------
def mse01(a, b):
    a = np.clip(np.asarray(a, dtype=np.float64), 0, 255) / 255.0
    b = np.clip(np.asarray(b, dtype=np.float64), 0, 255) / 255.0
    return float(((a - b) ** 2).mean())


def _block(case, dtype):
    g = load_golden(case)
    blk = load_recipe(network.AdaAttN(512, str(g["activation"])), "blk").to(DEV).eval()
    blk.compute_dtype = dtype
    with torch.no_grad():
        out = blk(*(torch.from_numpy(g[k]).to(DEV) for k in ("fc", "fs", "fcs")))
    assert out.dtype == torch.float32 and out.shape == g["out"].shape
    return out.cpu().numpy(), g["out"]


@pytest.mark.parametrize("case", ["block1_b2_4x4_s3x5", "block1_cos_b1_4x4"])
def test_block_matches_reference_goldens_fp32(case):
    out, want = _block(case, torch.float32)
    np.testing.assert_allclose(out, want, rtol=1e-3, atol=2e-3)


def _bf16_block_emulation(blk, fc, fs, fcs):
    """The bf16 block's arithmetic in fp64 with every operand rounded where the HIP route rounds it
    (engine.adaattn_forward): bf16 weights (f with log2 e folded in), bf16 normalised / centred GEMM inputs,
    bf16 Q, K, V'; statistics, biases, v_mu and everything after the products unrounded."""
    def r(t):
        return t.float().to(torch.bfloat16).double()

    def tok(x):
        return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()

    def w(m):
        return m.weight.reshape(D, D).double()
    fct, fst, fcst = tok(fc), tok(fs), tok(fcs)
    (mu_c, rs_c), (mu_s, rs_s), (mu_o, rs_o) = (ops.instnorm_stats(t) for t in (fct, fst, fcst))
    qn = r((fct - mu_c[:, None]) * rs_c[:, None])
    kn = r((fst - mu_s[:, None]) * rs_s[:, None])
    q = r(qn @ r(w(blk.f) * ops.LOG2E).T + blk.f.bias.double() * ops.LOG2E)
    k = r(kn @ r(w(blk.g)).T + blk.g.bias.double())
    v = r(r(fst - mu_s[:, None]) @ r(w(blk.h)).T)
    v_mu = mu_s.double() @ w(blk.h).T + blk.h.bias.double()
    out = _attn_ref(q, k, v, fcst, mu_o, rs_o, v_mu, True)
    return out.view(fc.shape[0], fc.shape[2], fc.shape[3], D).permute(0, 3, 1, 2)


def test_block_matches_reference_goldens_bf16():
    """The bf16 softmax block (mhada_attn_wide) on the golden's inputs.  test_gpu_heads.py has no bf16 block
    test, so the bounds are worked out here.  (1) Against the fp64 emulation of the same rounded operands
    (_bf16_block_emulation): the project's bf16 bound, norm-relative 1e-2 (TOL[bfloat16]).  (2) Against the
    reference's fp32 golden: the logits of this case span -20 .. 23 (std 7.6), so rounding the weights, the
    GEMM inputs and Q, K to bf16 moves a logit by about 0.03 and the output by that fraction — what the
    number format costs is the emulation's own distance from the golden, and by the triangle inequality the
    block may be at most that plus bound (1) away.  Measured: 9.9e-3 from the emulation (the kernel alone is
    1.5e-4 from fp64 on its own operands, test_attn_wide_vs_fp64: the rest is where the projection GEMMs round
    differently from the emulation, which has not been taken apart further), 1.47e-2 from the golden, the
    emulation itself 1.09e-2 from the golden."""
    g = load_golden("block1_b2_4x4_s3x5")
    blk = load_recipe(network.AdaAttN(512, "softmax"), "blk").to(DEV).eval()
    blk.compute_dtype = torch.bfloat16
    fc, fs, fcs = (torch.from_numpy(g[k]).to(DEV) for k in ("fc", "fs", "fcs"))
    with torch.no_grad():
        out = blk(fc, fs, fcs)
        emu = _bf16_block_emulation(blk, fc, fs, fcs)
    want = torch.from_numpy(g["out"]).to(DEV)
    assert out.dtype == torch.float32 and out.shape == want.shape
    e_emu, e_gold, fmt = rel(out, emu), rel(out, want), rel(emu, want)
    _log(f"AdaAttN bf16 block: vs same-operand fp64 emulation {e_emu:.3e}, vs reference golden {e_gold:.3e} "
         f"(the emulation itself is {fmt:.3e} from the golden)")
    assert e_emu < TOL[torch.bfloat16]
    assert e_gold < fmt + TOL[torch.bfloat16]


def test_cosine_block_under_bf16_autocast_takes_the_fp32_route():
    g = load_golden("block1_cos_b1_4x4")
    blk = load_recipe(network.AdaAttN(512, "cosine"), "blk").to(DEV).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(*(torch.from_numpy(g[k]).to(DEV) for k in ("fc", "fs", "fcs")))
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-3, atol=2e-3)


def _models(dtype, act="softmax"):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformer(activation=act), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = dtype
    return vc, vs, ada


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("case", ["full1_64_b2", "full1_64x128_s64_b1"])
def test_forward_matches_reference_goldens(case, dtype):
    g = load_golden(case)
    c = seeded_image(*map(int, g["content_shape"]), int(g["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, g["style_shape"]), int(g["seeds"][1])).to(DEV)
    vc, vs, ada = _models(dtype, str(g["activation"]))
    with torch.no_grad():
        cs = ada(vc(c), vs(s))
    assert isinstance(cs, torch.Tensor)  # cs alone, not a tuple
    cs = cs.cpu().numpy()
    assert cs.shape == g["cs"].shape
    mse = mse01(cs, g["cs"])
    _log(f"AdaAttnTransformer {case} {dtype}: mse01 {mse:.3e}")
    assert mse < 1e-4
    if dtype == torch.float32:
        assert float(((cs.astype(np.float64) - g["cs"].astype(np.float64)) ** 2).mean()) < 1e-4


def test_compute_dtype_and_autocast_both_select_bf16(monkeypatch):
    calls = []
    real = ops.attn_wide
    monkeypatch.setattr(ops, "attn_wide", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    vc, vs, ada = _models(None)
    c = seeded_image(1, 64, 64, 1).to(DEV)
    with torch.no_grad():
        fc, fs = vc(c), vs(c)
        ada(fc, fs)
        assert not calls  # fp32 by default
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a = ada(fc, fs)
        assert len(calls) == ada.num_layers
        ada.compute_dtype = torch.bfloat16
        b = ada(fc, fs)
        assert len(calls) == 2 * ada.num_layers
    assert torch.equal(a, b)


def test_strict_state_dict_load_equals_the_recipe():
    vc, vs, ada = _models(torch.float32)
    other = network.AdaAttnTransformer().to(DEV).eval()
    other.load_state_dict({k: v.clone() for k, v in ada.state_dict().items()}, strict=True)
    other.compute_dtype = torch.float32
    c = seeded_image(1, 64, 64, 1).to(DEV)
    with torch.no_grad():
        fc, fs = vc(c), vs(c)
        assert torch.equal(ada(fc, fs), other(fc, fs))
