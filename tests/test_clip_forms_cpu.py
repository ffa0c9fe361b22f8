"""The clip route's cosine and 4- / 16-head forms without a GPU: the bindings and the header list the two
shared-style entries (mhada_cosine_attn_shared, mhada_attn_hd_shared), and on CPU modules stylize_clip for a
cosine model and for a 4-head model is still exactly the loop of single calls."""
import os
import re

import pytest
import torch

import network
from mhada_hip import _lib
from mhada_hip.recipe import load_recipe, seeded_image
from mhada_hip.video import VideoStylizer

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mhada_hip.h")

# entry -> argument count (include/mhada_hip.h):
#   (q, mom, fcs, fcs_mu, fcs_rstd, v_mu, out, dtype, B, H, Nc, stream)
#   (q, kv, fcs, fcs_mu, fcs_rstd, v_mu, out, dtype, B, H, D, Nc, Ns, activation, stream)
ENTRIES = {"mhada_cosine_attn_shared": 12, "mhada_attn_hd_shared": 15}


def test_signature_table_lists_the_shared_entries():
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
        # the per-batch entry it is a form of takes the same arguments
        assert (res, args) == _lib.SIGNATURES[name[:-len("_shared")]]
    assert _lib.ABI_VERSION == 18


def test_header_declares_the_shared_entries():
    src = open(HEADER).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", src, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        base = re.search(r"^int " + name[:-len("_shared")] + r"\(([^;]*)\);", src, re.M)
        assert " ".join(m.group(1).split()) == " ".join(base.group(1).split())
    assert "WITHOUT a version bump" in src[src.index("mhada_attn_split3_planes_shared("):src.index("int mhada_attn_hd_shared(")]


def test_library_exports_the_shared_entries():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name)


FRAMES = seeded_image(3, 32, 48, 5)


@pytest.mark.parametrize("heads,act", [(8, "cosine"), (4, "softmax")], ids=["h8-cosine", "h4-softmax"])
def test_cpu_clip_equals_a_loop_of_calls(heads, act):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads, activation=act), "ada").eval()
    st = VideoStylizer(vc, vs, ada)
    st.set_style(seeded_image(1, 24, 32, 6))
    assert not st._clip_route(FRAMES)  # CPU modules: the per-frame loop
    want = torch.cat([st(FRAMES[i:i + 1]) for i in range(3)])
    got = st.stylize_clip(FRAMES, u8=False)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(st.stylize_clip(FRAMES, u8=False, max_frames=2), want)
    assert torch.equal(st.cur, want[2:3]) and torch.equal(st.prev, want[1:2])
