"""The single-head drop-ins ``network.AdaAttN`` / ``network.AdaAttnTransformer`` (adaDecoder.py:85-131,
209-232) without a GPU: API and state_dict parity with the reference (tests/golden/state_dict_keys_single.json,
recorded by make_goldens_single.py), the CPU route against the reference's own outputs with the tolerances of
test_network_cpu.py, the backward of the CPU route against a direct fp64 transcription, and the host-side
argument checks of ``mhada_attn_wide``."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import network
from conftest import load_golden
from mhada_hip import _lib
from mhada_hip.recipe import load_recipe, seeded_image

HERE = os.path.dirname(os.path.abspath(__file__))


def _recorded():
    with open(os.path.join(HERE, "golden", "state_dict_keys_single.json")) as f:
        return json.load(f)


def test_exports_and_constructor_signatures():
    assert "AdaAttnTransformer" in network.__all__ and "AdaAttN" in network.__all__
    sig = _recorded()["signatures"]
    assert str(inspect.signature(network.AdaAttnTransformer.__init__)) == sig["AdaAttnTransformer"]
    assert str(inspect.signature(network.AdaAttN.__init__)) == sig["AdaAttN"]
    assert network.AdaAttN(512).compute_dtype is None and network.AdaAttnTransformer().compute_dtype is None


def test_state_dict_keys_and_shapes_match_the_reference():
    rec = _recorded()
    for tag, m in (("ada1", network.AdaAttnTransformer()), ("block1_512", network.AdaAttN(512))):
        got = {n: list(t.shape) for n, t in m.state_dict().items()}
        assert got == rec[tag]
        # a dict with the reference's keys loads strictly
        m.load_state_dict({k: torch.zeros(s) for k, s in rec[tag].items()}, strict=True)
    assert not hasattr(network.AdaAttN(512), "out_conv")


def test_bad_activation_raises_the_reference_text():
    for make in (lambda: network.AdaAttN(512, "relu"), lambda: network.AdaAttnTransformer(activation="relu")):
        with pytest.raises(ValueError, match="Unknown activation function: relu"):
            make()


@pytest.mark.parametrize("case", ["block1_b2_4x4_s3x5", "block1_cos_b1_4x4"])
def test_block_cpu_matches_reference_goldens(case):
    g = load_golden(case)
    blk = load_recipe(network.AdaAttN(512, str(g["activation"])), "blk").eval()
    with torch.no_grad():
        y = blk(*(torch.from_numpy(g[k]) for k in ("fc", "fs", "fcs")))
    np.testing.assert_allclose(y.numpy(), g["out"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("case", ["full1_64_b2", "full1_64x128_s64_b1"])
def test_network_cpu_matches_reference_goldens(case):
    g = load_golden(case)
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").eval()
    ada = load_recipe(network.AdaAttnTransformer(activation=str(g["activation"])), "ada").eval()
    c = seeded_image(*map(int, g["content_shape"]), int(g["seeds"][0]))
    s = seeded_image(*map(int, g["style_shape"]), int(g["seeds"][1]))
    np.testing.assert_array_equal(c.numpy(), g["content"])
    with torch.no_grad():
        cs = ada(vc(c), vs(s))
    assert isinstance(cs, torch.Tensor)  # cs alone, not the multi-head (fcs, cs) tuple
    assert not cs.is_cuda and cs.dtype == torch.float32 and cs.shape == g["cs"].shape
    a = np.clip(cs.numpy(), 0, 255) / 255.0
    b = np.clip(g["cs"], 0, 255) / 255.0
    mse = float(((a - b) ** 2).mean())
    print(f"{case}: CPU drop-in vs reference MSE(clamp/255) = {mse:.3e}")
    assert mse < 1e-10, mse


def _transcription(blk, fc, fs, fcs):
    """AdaAttN.forward written out directly (softmax), in the dtype of its inputs."""
    b, c, h, w = fc.shape
    q = F.conv2d(F.instance_norm(fc), blk.f.weight, blk.f.bias).view(b, c, -1).permute(0, 2, 1)
    k = F.conv2d(F.instance_norm(fs), blk.g.weight, blk.g.bias).view(b, c, -1)
    v = F.conv2d(fs, blk.h.weight, blk.h.bias).view(b, c, -1).permute(0, 2, 1)
    a = torch.softmax(torch.bmm(q, k), dim=-1)
    m = torch.bmm(a, v)
    s = torch.sqrt((torch.bmm(a, v ** 2) - m ** 2).clamp(min=1e-6))
    m = m.view(b, h, w, c).permute(0, 3, 1, 2)
    s = s.view(b, h, w, c).permute(0, 3, 1, 2)
    return s * F.instance_norm(fcs) + m


def test_cpu_backward_matches_fp64_transcription():
    """Gradients of the CPU route (fp32 aten, query-chunked) on f, g and h against torch.autograd on the fp64
    transcription.  Bound: fp32 aten against fp64 on a 16 x 15 problem of O(1) values with 512-long sums —
    relative error of the gradient norm < 1e-4 (2^-24 sqrt(512) ~ 1.3e-6 per product chain, two orders of slack
    for the softmax and sqrt chains).  Measured: 4e-5 .. 5e-5 on f and g."""
    torch.manual_seed(5)
    blk = load_recipe(network.AdaAttN(512), "blk")
    g = torch.Generator().manual_seed(11)
    fc = torch.randn(2, 512, 4, 4, generator=g) * 2.0 + 0.5
    fs = torch.randn(2, 512, 3, 5, generator=g) * 1.5 - 0.25
    fcs = torch.randn(2, 512, 4, 4, generator=g)
    wgt = torch.randn(2, 512, 4, 4, generator=g)
    out = blk(fc, fs, fcs)
    assert out.requires_grad
    (out * wgt).sum().backward()
    blk64 = load_recipe(network.AdaAttN(512), "blk").double()
    ref = _transcription(blk64, fc.double(), fs.double(), fcs.double())
    np.testing.assert_allclose(out.detach().numpy(), ref.detach().float().numpy(), rtol=1e-4, atol=1e-4)
    (ref * wgt.double()).sum().backward()
    for name in ("f", "g", "h"):
        for pn in ("weight", "bias"):
            got, want = getattr(getattr(blk, name), pn).grad, getattr(getattr(blk64, name), pn).grad
            assert got is not None and torch.isfinite(got).all()
            # g's bias adds the same q . b_g to every key of a query: softmax ignores it, its gradient is zero
            # in exact arithmetic, so its error is measured against the norm of g's weight gradient
            scale = blk64.g.weight.grad.norm() if (name, pn) == ("g", "bias") else want.norm()
            err = ((got.double() - want).norm() / (scale + 1e-30)).item()
            print(f"grad {name}.{pn}: rel {err:.3e}")
            assert err < 1e-4, (name, pn, err)


def test_two_head_multihead_model_still_constructs():
    ada = network.AdaAttnTransformerMultiHead(num_heads=2)
    assert ada.adaAttnHead[0].head_dim == 256


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_attn_wide_is_an_additive_entry_of_abi_18():
    lib = _lib_or_skip()
    assert "mhada_attn_wide" in _lib.SIGNATURES and hasattr(lib, "mhada_attn_wide")
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18


def test_attn_wide_rejects_bad_arguments_without_a_launch():
    """A null pointer, Nc = -1, width 256 and a bad dtype code return MHADA_ERR_ARG on the host (no GPU here: a
    launch would fail differently).  The pointers are host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15

    def attn(q=p, out=p, dtype=_lib.BF16, B=1, Nc=4, Ns=4, D=512):
        return lib.mhada_attn_wide(q, p, p, p, p, p, p, out, None, dtype, B, Nc, Ns, D, None)

    for kw in (dict(q=None), dict(out=None), dict(Nc=-1), dict(Ns=0), dict(B=0), dict(D=256), dict(D=64),
               dict(dtype=_lib.F32), dict(dtype=7), dict(q=p + 2), dict(Nc=1 << 30, B=1 << 10)):
        assert attn(**kw) == 1, kw
        assert b"mhada_attn_wide" in lib.mhada_last_error(), kw
