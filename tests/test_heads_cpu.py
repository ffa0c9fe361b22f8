"""4- and 16-head models (head_dim 128 / 32) without a GPU: the numpy oracle reproduces the head-count
goldens (tests/golden/make_goldens_heads.py) to the bounds test_oracle_golden.py uses for the 8-head
cases, and the library's D-wide entry points exist and validate their arguments on the host."""
import ctypes
import os

import numpy as np
import pytest

from mhada_hip import _lib
from mhada_hip.recipe import recipe_state_dict, seeded_image
from oracle import mhada_oracle as O
from conftest import load_golden


def _vit_shapes(pos):
    shapes = {"patch_embedding.conv_proj.weight": (512, 3, 8, 8), "patch_embedding.conv_proj.bias": (512,)}
    if pos:
        shapes["pos_embedding.pos_embed"] = (1, 512, 32, 32)
    for i in range(3):
        p = f"encoder.{i}."
        shapes.update({p + "attention.in_proj_weight": (1536, 512), p + "attention.in_proj_bias": (1536,),
                       p + "attention.out_proj.weight": (512, 512), p + "attention.out_proj.bias": (512,),
                       p + "mlp.0.weight": (2048, 512), p + "mlp.0.bias": (2048,),
                       p + "mlp.2.weight": (512, 2048), p + "mlp.2.bias": (512,),
                       p + "ln1.weight": (512,), p + "ln1.bias": (512,),
                       p + "ln2.weight": (512,), p + "ln2.bias": (512,)})
    return shapes


def _block_shapes(heads, pre=""):
    d = 512 // heads
    s = {}
    for i in range(heads):
        for n in ("f", "g", "h"):
            s[f"{pre}{n}_list.{i}.weight"] = (d, d, 1, 1)
            s[f"{pre}{n}_list.{i}.bias"] = (d,)
    s[f"{pre}out_conv.weight"] = (512, 512, 1, 1)
    s[f"{pre}out_conv.bias"] = (512,)
    return s


DEC = [("conv1.0", 512, 256), ("conv1.1", 256, 256), ("conv1.2", 256, 256), ("conv1.3", 256, 256),
       ("conv1.4", 256, 128), ("conv2.0", 128, 128), ("conv2.1", 128, 64), ("conv3.0", 64, 64),
       ("conv3.1", 64, 3)]


def _ada_shapes(heads):
    s = {}
    for k in range(6):
        s.update(_block_shapes(heads, f"adaAttnHead.{k}."))
    for name, ci, co in DEC:
        s[f"decoder.{name}.conv.conv.weight"] = (co, ci, 3, 3)
        s[f"decoder.{name}.conv.conv.bias"] = (co,)
    return s


def params(tag, shapes):
    return O.to_numpy_params(recipe_state_dict(tag, shapes), np.float32)


def rel_err(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.mark.parametrize("case", ["full_64_b2_h4", "full_64_b2_h16", "full_64x128_s64_b1_h16"])
def test_oracle_full_forward_matches_reference_heads(case):
    g = load_golden(case)
    cshape, sshape, seeds, heads = g["content_shape"], g["style_shape"], g["seeds"], int(g["heads"])
    c = seeded_image(int(cshape[0]), int(cshape[1]), int(cshape[2]), int(seeds[0])).numpy()
    s = seeded_image(int(sshape[0]), int(sshape[1]), int(sshape[2]), int(seeds[1])).numpy()
    np.testing.assert_array_equal(c, g["content"])
    # O.stylize does not thread the head count: the same call sequence with it
    fc = O.vit_forward(c, params("vit_c", _vit_shapes(True)), heads=heads)
    fs = O.vit_forward(s, params("vit_s", _vit_shapes(False)), heads=heads)
    fcs, cs = O.adaformer_forward(fc, fs, params("ada", _ada_shapes(heads)), heads=heads,
                                  activation=str(g["activation"]))
    assert rel_err(fcs, g["fcs"]) < 1e-4
    a = np.clip(cs, 0, 255) / 255.0
    b = np.clip(g["cs"], 0, 255) / 255.0
    assert float(((a - b) ** 2).mean()) < 1e-10
    assert float(np.abs(cs - g["cs"]).max()) < 5e-3


@pytest.mark.parametrize("case", ["block_h4_b2_4x4_s3x5", "block_h16_b2_4x4_s3x5", "block_cos_h16_b1_4x4"])
def test_oracle_block_matches_reference_heads(case):
    g = load_golden(case)
    heads = int(g["heads"])
    out = O.ada_attn_multihead(g["fc"], g["fs"], g["fcs"], params("blk", _block_shapes(heads)), "", heads,
                               str(g["activation"]))
    assert rel_err(out, g["out"]) < 1e-5


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_abi_18_exports_the_head_width_entries():
    lib = _lib_or_skip()
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18
    for name in ("mhada_attn_hd", "mhada_fold_block_hd", "mhada_cosine_prep_hd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_head_width_entries_reject_bad_arguments_without_a_launch():
    """D = 48, a null pointer and Nc < 0 return MHADA_ERR_ARG on the host (no GPU here: a launch
    would fail differently).  The pointers are host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15

    def attn(D=32, Nc=4, q=p):
        return lib.mhada_attn_hd(q, p, p, p, p, p, p, 0, 1, 2, D, Nc, 4, 0, None)

    def fold(D=32, wq=p):
        return lib.mhada_fold_block_hd(p, p, p, p, p, p, p, p, wq, p, p, p, 1.0, 0, 1, 2, D, None)

    def prep(D=32, Nc=4, q=p):
        return lib.mhada_cosine_prep_hd(q, p, 0, 1, 2, D, Nc, 4, None)

    for fn, name in ((attn, b"mhada_attn_hd"), (fold, b"mhada_fold_block_hd"), (prep, b"mhada_cosine_prep_hd")):
        assert fn(D=48) == 1
        assert name in lib.mhada_last_error() and b"32 or 128" in lib.mhada_last_error()
        assert fn(D=64) == 1  # 64 belongs to the 64-wide entry points
    for fn, name in ((lambda: attn(q=None), b"mhada_attn_hd"), (lambda: fold(wq=None), b"mhada_fold_block_hd"),
                     (lambda: prep(q=None), b"mhada_cosine_prep_hd"), (lambda: attn(Nc=-1), b"mhada_attn_hd"),
                     (lambda: prep(Nc=-1), b"mhada_cosine_prep_hd")):
        assert fn() == 1
        assert name in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    assert lib.mhada_fold_block_hd(p, p, p, p, p, p, p, p, p, p, p, p, 1.0, 0, -1, 2, 32, None) == 1
    # the ViT's batch-axis attention: any width outside {32, 64, 128} is still an argument error
    assert lib.mhada_vit_batch_attn(p, p, 0, 2, 4, 2, 48, None) == 1
    assert b"32, 64 or 128" in lib.mhada_last_error()
