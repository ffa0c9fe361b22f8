"""Training 4- and 16-head models (head_dim 128 / 32) without a GPU: the drop-in's CPU autograd path
reproduces the reference's training goldens (tests/golden/make_train_goldens_heads.py) to the
tolerances test_train_cpu.check_against_golden applies to train_64_b2, and the library's D-wide
training entry points exist (in ABI 18, no bump) and validate their arguments on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import network
from conftest import load_golden
from mhada_hip import _lib, autograd_path
from mhada_hip.recipe import load_recipe, seeded_image
from mhada_hip.train import Trainer

HD_ENTRIES = ("mhada_attn_train_fwd_hd", "mhada_attn_train_bwd_hd", "mhada_attn_train_bwd_prep_hd")


def build_heads(heads, device="cpu"):
    """test_train_cpu.build with ``num_heads`` passed to both ViTs and the AdaFormer (as the golden's
    generator builds the reference models)."""
    torch.manual_seed(0)
    vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").to(device).train()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").to(device).train()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads), "ada").to(device).train()
    vgg = load_recipe(network.VGG19(), "vgg").to(device)
    return vc, vs, ada, vgg


def grad_summary(m):
    return np.array([float(p.grad.double().norm()) if p.grad is not None else 0.0
                     for _, p in sorted(m.named_parameters())])


def check_against_golden_heads(tr, device, heads):
    """test_train_cpu.check_against_golden on train_64_b2_h{heads}: the same tolerances for the five
    losses and the per-parameter gradient norms (the head goldens store no single gradient tensor)."""
    g = load_golden(f"train_64_b2_h{heads}")
    assert int(g["heads"]) == heads
    c = seeded_image(2, 64, 64, int(g["content_seed"])).to(device)
    s = seeded_image(2, 64, 64, int(g["style_seed"])).to(device)
    out = tr.backward(c, s)
    got = np.array([float(out[k].detach()) for k in ("loss_gs", "loss_lf", "loss_id1", "loss_id2", "loss")])
    np.testing.assert_allclose(got, g["losses"], rtol=2e-4)
    for name, m in (("vit_c", tr.vit_c), ("vit_s", tr.vit_s), ("ada", tr.ada)):
        ref = g[f"grad_{name}"]  # tiny norms (<1e-4 of the largest) are rounding noise
        np.testing.assert_allclose(grad_summary(m), ref, rtol=2e-3, atol=1e-5 * ref.max())


@pytest.mark.parametrize("heads", [4, 16])
def test_train_step_matches_reference_golden_heads(heads):
    torch.set_num_threads(8)
    tr = Trainer(*build_heads(heads))
    check_against_golden_heads(tr, "cpu", heads)
    # the stylised image of the same (train-mode) forward, to the bound test_heads_cpu holds cs to
    g = load_golden(f"train_64_b2_h{heads}")
    c = seeded_image(2, 64, 64, int(g["content_seed"]))
    s = seeded_image(2, 64, 64, int(g["style_seed"]))
    with torch.no_grad():
        _, cs = tr.ada(tr.vit_c(c), tr.vit_s(s))
    assert float(np.abs(cs.numpy() - g["cs"]).max()) < 5e-3


@pytest.mark.parametrize("heads", [2, 4, 8, 16, 32])
def test_fused_train_attn_is_false_on_cpu_at_every_width(heads):
    blk = network.AdaAttnTransformerMultiHead(num_heads=heads).adaAttnHead[0]
    assert blk.head_dim == 512 // heads
    assert not autograd_path._fused_train_attn(blk, torch.zeros(1, 512, 2, 2))


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_training_entries_were_added_to_abi_18():
    lib = _lib_or_skip()
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18
    for name in HD_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_training_entries_reject_bad_arguments_without_a_launch():
    """D = 48, D = 64, a null pointer and Nc = -1 return MHADA_ERR_ARG on the host (no GPU here: a
    launch would fail differently).  The pointers are host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15

    def fwd(D=32, Nc=4, q=p, Ns=4, BH=2):
        return lib.mhada_attn_train_fwd_hd(q, p, p, p, p, p, p, BH, D, Nc, Ns, None)

    def bwd(D=32, Nc=4, q=p, Ns=4, BH=2):
        return lib.mhada_attn_train_bwd_hd(q, p, p, p, p, p, p, p, p, BH, D, Nc, Ns, None)

    def prep(D=32, rows=4, q=p):
        return lib.mhada_attn_train_bwd_prep_hd(q, p, p, p, p, p, rows, D, None)

    for fn, name in zip((fwd, bwd, prep), HD_ENTRIES):
        for D in (48, 64):  # 64 belongs to the 64-wide entry points
            assert fn(D=D) == 1
            err = lib.mhada_last_error()
            assert name.encode() + b":" in err and b"32 or 128" in err
        assert fn(q=None) == 1
        assert name.encode() + b":" in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    for fn, name in ((lambda: fwd(Nc=-1), HD_ENTRIES[0]), (lambda: bwd(Nc=-1), HD_ENTRIES[1]),
                     (lambda: prep(rows=-1), HD_ENTRIES[2]), (lambda: fwd(Ns=0), HD_ENTRIES[0]),
                     (lambda: bwd(Ns=0), HD_ENTRIES[1]), (lambda: fwd(BH=0), HD_ENTRIES[0]),
                     (lambda: bwd(BH=0), HD_ENTRIES[1])):
        assert fn() == 1
        assert name.encode() + b":" in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    # an empty query side is legal for the forward and the elementwise head: nothing to launch
    assert fwd(Nc=0) == 0 and prep(rows=0) == 0
