"""Feature inversion without a GPU: the header declares the new entry points and the binding lists them,
their host-side argument checks, invert_features against a hand-written copy of its loop, the CPU
routing of a grad-carrying image (unchanged: aten), and autograd_path against the reference's golden
(tests/golden/make_inversion_goldens.py)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import network
from mhada_hip import _lib, autograd_path
from mhada_hip.inversion import invert_features
from mhada_hip.recipe import load_recipe, seeded_image
from conftest import REPO, load_golden

NEW = ("mhada_patch_embed_dgrad", "mhada_attn_train_dq", "mhada_attn_train_dq_hd")


def _frozen(m):
    return m.eval().requires_grad_(False)


def _vit(tag):
    return _frozen(load_recipe(network.VisionTransformer(pos_embedding=tag == "vit_c"), tag))


def _init():
    return torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(7))


def test_header_declares_and_binding_lists_the_new_entries():
    with open(os.path.join(REPO, "include", "mhada_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18  # additive: no version bump
    # the argument counts of the binding follow the header (stream last)
    assert len(_lib.SIGNATURES["mhada_patch_embed_dgrad"][1]) == 9
    assert len(_lib.SIGNATURES["mhada_attn_train_dq"][1]) == 11
    assert len(_lib.SIGNATURES["mhada_attn_train_dq_hd"][1]) == 12


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_new_entries_reject_bad_arguments_without_a_launch():
    """Every case returns MHADA_ERR_ARG on the host, before any launch (no GPU here); the pointers are
    host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    assert lib.mhada_abi_version() == 18
    for name in NEW:
        assert hasattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15

    def dgrad(dy=p, B=1, C=512, Ci=3, H=16, W=16, dimg=p):
        return lib.mhada_patch_embed_dgrad(dy, p, dimg, B, C, Ci, H, W, None)

    for kw, msg in (({"W": 20}, b"multiple of 8"), ({"W": 0}, b"multiple of 8"), ({"H": 7}, b"H >= 8"),
                    ({"Ci": 1}, b"Ci must be 3"), ({"Ci": 4}, b"Ci must be 3"), ({"C": 96}, b"multiple of 64"),
                    ({"C": 0}, b"multiple of 64"), ({"dy": None}, b"bad args"), ({"B": 0}, b"bad args"),
                    ({"dimg": p + 4}, b"16-byte aligned"),
                    ({"B": 4096, "C": 1024, "H": 512, "W": 512}, b"2^31")):
        assert dgrad(**kw) == 1, kw
        err = lib.mhada_last_error()
        assert b"mhada_patch_embed_dgrad" in err and msg in err, (kw, err)

    def dq(q=p, Nc=4, Ns=4):
        return lib.mhada_attn_train_dq(q, p, p, p, p, p, p, 1, Nc, Ns, None)

    def dq_hd(q=p, D=32, Nc=4, Ns=4):
        return lib.mhada_attn_train_dq_hd(q, p, p, p, p, p, p, 1, D, Nc, Ns, None)

    for fn, name in ((lambda: dq(q=None), b"mhada_attn_train_dq"), (lambda: dq(Nc=0), b"mhada_attn_train_dq"),
                     (lambda: dq(Ns=0), b"mhada_attn_train_dq"), (lambda: dq_hd(q=None), b"mhada_attn_train_dq_hd"),
                     (lambda: dq_hd(Nc=-1), b"mhada_attn_train_dq_hd")):
        assert fn() == 1
        assert name in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    for D in (48, 64):
        assert dq_hd(D=D) == 1 and b"32 or 128" in lib.mhada_last_error()
    assert dq_hd(Nc=0) == 0  # no query rows: nothing to launch


def test_invert_features_reproduces_the_hand_written_loop():
    vit = _vit("vit_c")
    with torch.no_grad():
        target = vit(seeded_image(1, 64, 64, 101))
    img, hist = invert_features(vit, target, _init(), steps=3, lr=0.5)

    recon = _init().requires_grad_(True)
    opt = torch.optim.Adam([recon], lr=0.5)
    ref = []
    for _ in range(3):
        opt.zero_grad()
        fc = vit(recon)
        loss = sum(F.mse_loss(fc[l], target[l]) for l in range(3))
        loss.backward()
        opt.step()
        ref.append(loss.item())
    assert hist == ref
    assert torch.equal(img, recon.detach()) and not img.requires_grad
    assert all(p.grad is None for p in vit.parameters())
    # a single tensor counts as a list of one; a count mismatch is an error
    _, h1 = invert_features(lambda x: vit(x)[0], target[0], _init(), steps=1, lr=0.5)
    assert h1[0] == F.mse_loss(vit(_init())[0], target[0]).item()
    with pytest.raises(ValueError):
        invert_features(vit, target[:2], _init(), steps=1, lr=0.5)


def test_cpu_image_with_grad_is_still_the_aten_module():
    vit = _vit("vit_c")
    x = _init().requires_grad_(True)
    with autograd_path.vit_input_grad("hip"):
        outs = autograd_path.vit_forward(vit, x)
    # the module evaluated with aten, as the reference writes it (vit.py:148-169)
    t = vit.patch_embedding.conv_proj(x)
    B, C, h, w = t.shape
    t = t.reshape(B, C, h * w).permute(0, 2, 1)
    pe = F.interpolate(vit.pos_embedding.pos_embed, size=(h, w), mode="bilinear", align_corners=False)
    t = t + pe.reshape(1, C, h * w).permute(0, 2, 1)
    for blk, o in zip(vit.encoder, outs):
        y = blk.ln1(t)
        y, _ = blk.attention(y, y, y, need_weights=False)
        t = y + t
        t = t + blk.mlp(blk.ln2(t))
        assert torch.equal(o, t.permute(0, 2, 1).reshape(B, C, h, w))
    (g,) = torch.autograd.grad(outs[-1].square().mean(), x)
    assert g.shape == x.shape and torch.isfinite(g).all()


def test_switch_validates_and_restores():
    assert autograd_path.VIT_INPUT_GRAD == "hip"
    with autograd_path.vit_input_grad("torch"):
        assert autograd_path.VIT_INPUT_GRAD == "torch"
    assert autograd_path.VIT_INPUT_GRAD == "hip"
    with pytest.raises(ValueError):
        with autograd_path.vit_input_grad("cpu"):
            pass


def test_autograd_path_matches_the_reference_golden():
    """The reference's first inversion iteration (losses and image gradients) from autograd_path on the CPU:
    the same aten expressions in fp32, so agreement is to summation order — 1e-5 relative (L2)."""
    gold = load_golden("inversion_64")
    vit_c, vit_s = _vit("vit_c"), _vit("vit_s")
    ada = _frozen(load_recipe(network.AdaAttnTransformerMultiHead(), "ada"))
    content, style = seeded_image(1, 64, 64, int(gold["seeds"][0])), seeded_image(1, 64, 64, int(gold["seeds"][1]))
    init = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(int(gold["seeds"][2])))

    def blocks(fc, fs):
        fcs = fc[0]
        for i in range(ada.num_layers):
            fcs = ada.adaAttnHead[2 * i](fc[i], fs[i], fcs)
            fcs = ada.adaAttnHead[2 * i + 1](fcs, fs[i], fcs)
        return fcs

    with torch.no_grad():
        target = vit_c(content)
        fs = vit_s(style)
        target_ada = blocks(target, fs)
    # (b) on the image stacked twice, as the golden's generator evaluates it (its docstring: aten's CPU
    # instance_norm backward at B = 1); the leaf collects exactly the B = 1 gradient
    twice = lambda t: torch.cat([t, t])  # noqa: E731
    for loss_fn, key, i in ((lambda x: sum(F.mse_loss(f, t) for f, t in zip(vit_c(x), target)), "grad_vit", 0),
                            (lambda x: F.mse_loss(blocks(vit_c(twice(x)), [twice(f) for f in fs]), twice(target_ada)),
                             "grad_ada", 1)):
        x = init.clone().requires_grad_(True)
        loss = loss_fn(x)
        (g,) = torch.autograd.grad(loss, x)
        ref = torch.from_numpy(gold[key]).double()
        assert abs(loss.item() - gold["losses"][i]) <= 1e-5 * gold["losses"][i]
        assert ((g.double() - ref).norm() / ref.norm()).item() <= 1e-5, key
