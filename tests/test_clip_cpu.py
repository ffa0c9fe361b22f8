"""VideoStylizer.stylize_clip and engine.vit_forward(groups=) on CPU modules: the frames are evaluated one
by one through the per-frame route, so the results are exactly a loop's; and the argument checks."""
import numpy as np
import pytest
import torch

import network
from mhada_hip import engine
from mhada_hip.recipe import load_recipe, seeded_image
from mhada_hip.video import VideoStylizer, tensor_to_cv2


@pytest.fixture(scope="module")
def st():
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").eval()
    s = VideoStylizer(vc, vs, ada)
    s.set_style(seeded_image(1, 24, 32, 6))
    return s


FRAMES = seeded_image(3, 32, 48, 5)


def test_clip_equals_a_loop_of_calls(st):
    want = torch.cat([st(FRAMES[i:i + 1]) for i in range(3)])
    got = st.stylize_clip(FRAMES, u8=False)
    assert torch.equal(got, want)
    assert torch.equal(st.cur, want[2:3]) and torch.equal(st.prev, want[1:2])
    for mf in (1, 2):
        assert torch.equal(st.stylize_clip(FRAMES, u8=False, max_frames=mf), want)
    # a batch through the modules is NOT this: the reference ViT attends over the batch axis
    assert not torch.equal(st(FRAMES), want)


@pytest.mark.parametrize("bgr", [True, False])
def test_clip_u8_forms(st, bgr):
    want = tensor_to_cv2(st.stylize_clip(FRAMES, u8=False), bgr=bgr)
    got = st.stylize_clip(FRAMES, bgr=bgr)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert np.array_equal(st.stylize_clip(FRAMES, bgr=bgr, to_host=True), want)
    # u8 B,G,R frames in: the reference's BGR -> RGB, HWC -> CHW, float
    u8 = torch.from_numpy(tensor_to_cv2(FRAMES, bgr=True))
    assert torch.equal(st.stylize_clip(u8, u8=False), st.stylize_clip(FRAMES.floor(), u8=False))


def test_vit_forward_groups_equals_per_frame(st):
    with torch.no_grad():
        got = engine.vit_forward(st.vit_c, FRAMES, groups=3)
        want = [torch.cat(z) for z in zip(*(st.vit_c(FRAMES[i:i + 1]) for i in range(3)))]
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        engine.vit_forward(st.vit_c, FRAMES, groups=2)


def test_clip_argument_errors(st):
    with pytest.raises(ValueError):
        st.stylize_clip(FRAMES[0])                      # rank
    with pytest.raises(ValueError):
        st.stylize_clip(torch.zeros(2, 4, 32, 48))      # channels
    with pytest.raises(ValueError):
        st.stylize_clip(torch.zeros(2, 32, 48, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        st.stylize_clip(FRAMES, max_frames=0)
    fresh = VideoStylizer(st.vit_c, st.vit_s, st.ada)
    with pytest.raises(RuntimeError):
        fresh.stylize_clip(FRAMES)                      # before set_style
