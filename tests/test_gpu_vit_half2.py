"""HALF2 routing in vit_forward: with the tile-fill rule forced on (as test_fp32_goldens_with_split3_forced
does) the LayerNorm-fed GEMMs take HALF2 and the outputs meet the reference goldens; with ops.F32_HALF2
off no HALF2 entry runs; a layer whose preparation refuses keeps SPLIT3 silently."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from conftest import load_golden
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"
CASE = "full_64_b2"


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


@pytest.fixture()
def forced(monkeypatch):
    """The SPLIT3 routing rule forced on, HALF2 launches counted."""
    from mhada_hip import engine, ops
    monkeypatch.setattr(engine, "_split3_fills", lambda M, N, dev: True)
    monkeypatch.setattr(ops, "F32_SPLIT_ATTN", True)
    calls = {"gemm": 0, "ln": 0}
    lin, ln = ops.linear_half2, ops.layernorm_half2

    def lin_(*a, **k):
        calls["gemm"] += 1
        return lin(*a, **k)

    def ln_(*a, **k):
        calls["ln"] += 1
        return ln(*a, **k)
    monkeypatch.setattr(ops, "linear_half2", lin_)
    monkeypatch.setattr(ops, "layernorm_half2", ln_)
    return calls


def inputs():
    g = load_golden(CASE)
    c = seeded_image(*map(int, g["content_shape"]), int(g["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, g["style_shape"]), int(g["seeds"][1])).to(DEV)
    return g, c, s


def test_half2_route_meets_the_goldens_and_off_is_the_split3_route(forced, monkeypatch):
    from mhada_hip import ops
    g, c, s = inputs()
    ms = models()
    nlayers = len(ms[0].encoder) + len(ms[1].encoder)
    monkeypatch.setattr(ops, "F32_HALF2", True)
    fc, fs, fcs, cs = stylize(ms, c, s)
    assert forced["gemm"] == 2 * nlayers and forced["ln"] == 2 * nlayers  # QKV and MLP1 of every layer
    csn = cs.cpu().numpy()
    a, b = np.clip(csn, 0, 255) / 255.0, np.clip(g["cs"], 0, 255) / 255.0
    assert float(((a.astype(np.float64) - b) ** 2).mean()) < 1e-4
    assert float(((csn.astype(np.float64) - g["cs"]) ** 2).mean()) < 1e-4
    np.testing.assert_allclose(fcs.cpu().numpy(), g["fcs"], rtol=1e-3, atol=2e-3)
    for i in (0, 2):
        np.testing.assert_allclose(fc[i].cpu().numpy(), g[f"fc{i}"], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(fs[i].cpu().numpy(), g[f"fs{i}"], rtol=1e-3, atol=1e-3)
    on = bits(list(fc) + list(fs) + [fcs, cs])

    # off: no HALF2 launch, and the bits of the SPLIT3 route on models that never prepared HALF2
    monkeypatch.setattr(ops, "F32_HALF2", False)
    forced["gemm"] = forced["ln"] = 0
    off_out = stylize(ms, c, s)
    assert forced["gemm"] == 0 and forced["ln"] == 0
    off = bits(list(off_out[0]) + list(off_out[1]) + list(off_out[2:]))
    fresh_out = stylize(models(), c, s)
    fresh = bits(list(fresh_out[0]) + list(fresh_out[1]) + list(fresh_out[2:]))
    assert all(torch.equal(x, y) for x, y in zip(off, fresh))
    assert any(not torch.equal(x, y) for x, y in zip(on, off))  # the two routes are different arithmetic


def test_a_layer_whose_scale_leaves_the_window_keeps_split3(forced, monkeypatch):
    from mhada_hip import engine, ops
    _, c, _ = inputs()
    vc = models()[0]
    with torch.no_grad():
        vc.encoder[1].ln1.weight.mul_(2.0 ** 56)  # Y ~ 2^60: s_a would be below 2^-40
    monkeypatch.setattr(ops, "F32_HALF2", True)
    with torch.no_grad():
        vc(c)
    layers = engine.vit_prep(vc, torch.float32)["layers"]
    assert layers[1]["w_qkv_half2"] is None and layers[1]["w1_half2"] is not None
    assert layers[0]["w_qkv_half2"] is not None
    assert forced["gemm"] == 2 * len(layers) - 1 and forced["ln"] == 2 * len(layers) - 1

    # every LayerNorm refused: the switch on is the switch off, bit for bit, without a HALF2 launch
    vc2 = models()[0]
    with torch.no_grad():
        for blk in vc2.encoder:
            blk.ln1.weight.mul_(2.0 ** 56)
            blk.ln2.weight.mul_(2.0 ** 56)
    forced["gemm"] = forced["ln"] = 0
    with torch.no_grad():
        on2 = bits(vc2(c))
    assert forced["gemm"] == 0 and forced["ln"] == 0
    assert all(L["w_qkv_half2"] is None and L["w1_half2"] is None
               for L in engine.vit_prep(vc2, torch.float32)["layers"])
    monkeypatch.setattr(ops, "F32_HALF2", False)
    with torch.no_grad():
        off2 = bits(vc2(c))
    assert all(torch.equal(x, y) for x, y in zip(on2, off2))
