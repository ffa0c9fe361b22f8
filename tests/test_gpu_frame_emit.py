"""Frame emit on the device: mhada_frame_emit element by element against the reference's output
expression (infer_video.py:94,110-112), padded rows, the fused last decoder layer
(mhada_conv3x3_out3_u8) bit for bit against the unfused pair in every dispatch form, and
VideoStylizer.stylize_u8 end to end."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from conftest import load_golden
from mhada_hip import _lib, ops, video
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"
SPECIALS = [0.0, -0.0, 0.99999994, 1.0, 254.99998, 255.0, 255.5, 256.0, -3.0, 1e30, float("inf"), float("-inf")]
FILL = 0xA5


def reference_frame(cs: torch.Tensor, bgr: bool) -> np.ndarray:
    """clamp -> permute -> numpy().astype(np.uint8) (-> RGB2BGR) on the CPU copy of cs [B][3][H][W]."""
    out = cs.detach().float().cpu().clamp(0, 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    return np.ascontiguousarray(out[..., ::-1]) if bgr else out


def padded_out(B, H, W, row_bytes):
    """A 0xA5-filled buffer of B * H rows of row_bytes plus one guard row, and the [B][H][W][3] view of it."""
    buf = torch.full(((B * H + 1) * row_bytes,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf.as_strided((B, H, W, 3), (H * row_bytes, row_bytes, 3, 1))


def check_padding(buf, B, H, W, row_bytes):
    rows = buf.cpu().numpy().reshape(B * H + 1, row_bytes)
    assert (rows[:B * H, 3 * W:] == FILL).all(), "a padding byte was written"
    assert (rows[B * H] == FILL).all(), "the guard row after the last image was written"


@functools.lru_cache(maxsize=None)
def emit_input(B, H, W):
    """Noise in [-20, 280] with the special values at the first and last pixel of the first row, of a
    middle row and of the image's last row, in every channel and image in turn."""
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
    x = torch.rand(B, 3, H, W, generator=g) * 300 - 20
    i = 0
    for b in range(B):
        for c in range(3):
            for y in sorted({0, H // 2, H - 1}):
                for xx in sorted({0, W - 1}):
                    x[b, c, y, xx] = SPECIALS[i % len(SPECIALS)]
                    i += 1
    return x


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 3), (2, 10, 67), (1, 4, 256), (3, 7, 130)])
def test_frame_emit_matches_reference_expression(shape, bgr):
    x = emit_input(*shape)
    got = ops.frame_emit(x.to(DEV), bgr=bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[1], shape[2], 3)
    np.testing.assert_array_equal(got.cpu().numpy(), reference_frame(x, bgr))
    # every special value somewhere (the 1-pixel image holds only the first few)
    if shape[1] * shape[2] > 1:
        want = dict(zip(SPECIALS, [0, 0, 0, 1, 254, 255, 255, 255, 0, 255, 255, 0]))
        rgb = ops.frame_emit(x.to(DEV), bgr=False).cpu().numpy()
        for v, u in want.items():
            idx = (x.permute(0, 2, 3, 1) == v).numpy()
            assert idx.any() and (rgb[idx] == u).all(), (v, u)
    # the public function on a device tensor is this kernel
    assert torch.equal(video.tensor_to_cv2(x.to(DEV), bgr=bgr), got)
    assert torch.equal(video.tensor_to_cv2(x[0].to(DEV), bgr=bgr), got[0])


def test_frame_emit_nan_is_zero():
    x = emit_input(2, 10, 67).clone()
    x[0, 0, 0, 0] = float("nan")
    x[1, 2, 9, 66] = float("nan")
    x[0, 1, 3, 5] = float("nan")
    got = ops.frame_emit(x.to(DEV), bgr=False).cpu().numpy()
    assert got[0, 0, 0, 0] == 0 and got[1, 9, 66, 2] == 0 and got[0, 3, 5, 1] == 0
    ok = ~torch.isnan(x).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(got[ok], reference_frame(torch.nan_to_num(x, nan=0.0), False)[ok])


@pytest.mark.parametrize("pad", [5, 1])
@pytest.mark.parametrize("shape", [(1, 5, 3), (2, 10, 67), (3, 7, 130)])
def test_frame_emit_padded_rows_keep_their_padding(shape, pad):
    B, H, W = shape
    x = emit_input(*shape)
    rb = 3 * W + pad  # 3W + 1: the rows start at every misalignment in turn
    for bgr in (True, False):
        buf, out = padded_out(B, H, W, rb)
        r = ops.frame_emit(x.to(DEV), bgr=bgr, out=out)
        assert r.data_ptr() == out.data_ptr()
        np.testing.assert_array_equal(out.cpu().numpy(), reference_frame(x, bgr))
        check_padding(buf, B, H, W, rb)


def test_frame_emit_rejects_short_rows_and_bad_arguments():
    x = emit_input(1, 5, 3).to(DEV)
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.frame_emit(x, out=buf.as_strided((1, 5, 3, 3), (40, 8, 3, 1)))  # row_bytes 8 < 3W = 9
    rc = _lib.load().mhada_frame_emit(x.data_ptr(), 1, 5, 3, buf.data_ptr(), 8, 1, None)
    assert rc != 0 and "row_bytes" in _lib.load().mhada_last_error().decode()
    assert _lib.load().mhada_frame_emit(None, 1, 5, 3, buf.data_ptr(), 9, 1, None) != 0
    assert _lib.load().mhada_frame_emit(x.data_ptr(), 1, 0, 3, buf.data_ptr(), 9, 1, None) != 0
    with pytest.raises(ValueError):
        ops.frame_emit(x.half())
    with pytest.raises(ValueError):
        ops.frame_emit(x[:, :2])
    w = torch.zeros(9, 32, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.conv3x3_out3_u8(torch.zeros(1, 4, 4, 32, device=DEV), w, torch.zeros(3, device=DEV),
                            out=torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)[..., :3])  # pixels not packed


# ---- fused = unfused ---------------------------------------------------------------------------------
FORMS = [  # (id, Cin, dtype, knobs) -> the kernel mhada_conv3x3_out3's dispatch picks
    ("f32_tile_c32", 32, torch.float32, {}),
    ("f32_tile_c64", 64, torch.float32, {}),
    ("bf16_mfma_c32", 32, torch.bfloat16, {}),
    ("bf16_mfma_c64", 64, torch.bfloat16, {}),
    ("f32_pixel_c128", 128, torch.float32, {}),
    ("bf16_pixel_c128", 128, torch.bfloat16, {}),
    ("f32_pixel_c64_knobs0", 64, torch.float32, dict(out3_tile=0, out3_mfma=0)),
    ("bf16_pixel_c64_knobs0", 64, torch.bfloat16, dict(out3_tile=0, out3_mfma=0)),
]
# (1, 2, 2): the smallest the entry accepts; (2, 6, 66): one pixel row past a 4-row tile, two columns past
# a 64-column tile; (1, 9, 130)
OUT3_SHAPES = [(1, 2, 2), (2, 6, 66), (1, 9, 130)]


def out3_inputs(Cin, dt, shape):
    """Inputs scaled so the layer's pre-activation is about N(127, 250^2): x uniform in [-1/2, 1/2), w
    normal with sigma = 250 / sqrt(9 Cin / 12), bias near 127.  About 30% of the outputs then lie below 0
    before the ReLU, 40% inside (0, 255) and 30% above 255.  (The seed is one at which the 12 values of
    the 2 x 2 image split at least 3 / 3 / 3 for every Cin, none within 8 of a band edge.)"""
    B, H, W = shape
    g = torch.Generator().manual_seed(49 + Cin)
    x = (torch.rand(B, H, W, Cin, generator=g) - 0.5).to(DEV).to(dt)
    w = (torch.randn(9, Cin, 3, generator=g) * (250.0 / (0.75 * Cin) ** 0.5)).to(DEV)
    b = torch.tensor([120.0, 127.5, 135.0], device=DEV)
    return x, w, b


@pytest.mark.parametrize("shape", OUT3_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_fused_out3_u8_equals_unfused_bit_for_bit(form, shape):
    _, Cin, dt, knobs = form
    B, H, W = shape
    x, w, b = out3_inputs(Cin, dt, shape)
    saved = {k: _lib.get_tuning(k) for k in knobs}
    try:
        for k, v in knobs.items():
            _lib.set_tuning(k, v)
        y32 = ops.conv3x3_out3(x, w, b, clamp255=True)
        # at least a tenth of the output values falls in each band: 0 (below 0 before the ReLU), inside
        # (0, 255), and clamped at 255
        n = y32.numel()
        lo, hi = int((y32 == 0).sum()), int((y32 == 255).sum())
        assert 10 * lo >= n and 10 * hi >= n and 10 * (n - lo - hi) >= n, (lo, n - lo - hi, hi)
        for bgr in (True, False):
            want = ops.frame_emit(y32, bgr=bgr)
            np.testing.assert_array_equal(want.cpu().numpy(), reference_frame(y32, bgr))
            got = ops.conv3x3_out3_u8(x, w, b, bgr=bgr)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
            assert torch.equal(got, want)
            for pad in (5, 1):
                rb = 3 * W + pad
                buf, out = padded_out(B, H, W, rb)
                r = ops.conv3x3_out3_u8(x, w, b, bgr=bgr, out=out)
                assert r.data_ptr() == out.data_ptr()
                assert torch.equal(out, want)
                check_padding(buf, B, H, W, rb)
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)


@pytest.mark.parametrize("form", FORMS[:6], ids=lambda f: f[0])
def test_existing_out3_entry_untouched_and_u8_repeatable(form):
    _, Cin, dt, _ = form
    x, w, b = out3_inputs(Cin, dt, (2, 6, 66))
    for clamp in (False, True):
        before = ops.conv3x3_out3(x, w, b, clamp255=clamp)
        u1 = ops.conv3x3_out3_u8(x, w, b)
        after = ops.conv3x3_out3(x, w, b, clamp255=clamp)
        u2 = ops.conv3x3_out3_u8(x, w, b)
        assert torch.equal(before, after)
        assert torch.equal(u1, u2)
    assert float(before.max()) == 255.0 and float(ops.conv3x3_out3(x, w, b).max()) > 255.0


def test_out3_u8_rejects_short_rows():
    x, w, b = out3_inputs(32, torch.float32, (1, 2, 2))
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rc = _lib.load().mhada_conv3x3_out3_u8(x.data_ptr(), ops.dt_code(x.dtype), w.data_ptr(), b.data_ptr(),
                                           buf.data_ptr(), 5, 1, 1, 2, 2, 32, None)
    assert rc != 0 and "row_bytes" in _lib.load().mhada_last_error().decode()


# ---- end to end --------------------------------------------------------------------------------------
def models(dtype, single=False):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = network.AdaAttnTransformer() if single else network.AdaAttnTransformerMultiHead()
    ada = load_recipe(ada, "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = dtype
    return vc, vs, ada


def golden_inputs():
    """The 64^2 B2 golden case's inputs (tests/test_gpu_parity.py builds them the same way)."""
    g = load_golden("full_64_b2")
    c = seeded_image(*map(int, g["content_shape"]), int(g["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, g["style_shape"]), int(g["seeds"][1])).to(DEV)
    return c, s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stylize_u8_equals_reference_expression_of_call(dtype):
    c, s = golden_inputs()
    st = video.VideoStylizer(*models(dtype))
    st.set_style(s)
    cs = st(c)  # fp32 [2][3][64][64], clamped
    assert cs.dtype == torch.float32 and tuple(cs.shape) == (2, 3, 64, 64)
    for bgr in (True, False):
        host = st.stylize_u8(c, bgr=bgr, to_host=True)  # the default route
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.shape == (2, 64, 64, 3)
        np.testing.assert_array_equal(host, reference_frame(cs, bgr))
        for fused in (True, False):  # the fused last layer and out3 + frame_emit: the same bits
            np.testing.assert_array_equal(st.stylize_u8(c, bgr=bgr, to_host=True, fused=fused), host)
        dev = st.stylize_u8(c, bgr=bgr)
        assert dev.is_cuda and dev.dtype == torch.uint8
        np.testing.assert_array_equal(dev.cpu().numpy(), host)
    # __call__ is what it was: fp32, and it equals the module call clamped
    with torch.no_grad():
        _, raw = st.ada(st.vit_c(c), st.fs)
    assert torch.equal(st(c), raw.clamp(0, 255))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stylize_u8_single_head_model(dtype):
    """The single-head AdaAttnTransformer returns cs alone (VideoStylizer.__call__ takes the multi-head
    model only), so the fp32 result is the module call's, clamped as __call__ clamps."""
    c, s = golden_inputs()
    vc, vs, ada = models(dtype, single=True)
    st = video.VideoStylizer(vc, vs, ada)
    st.set_style(s)
    with torch.no_grad():
        cs = ada(vc(c), st.fs).clamp(0, 255)
    for bgr in (True, False):
        for fused in (None, True, False):
            np.testing.assert_array_equal(st.stylize_u8(c, bgr=bgr, to_host=True, fused=fused),
                                          reference_frame(cs, bgr))


def test_stylize_u8_four_frames_two_host_buffers_and_warping_error():
    """Four consecutive frames with to_host=True: each returned array is an owning copy, so the arrays of
    frames t and t + 2 (which share a pinned buffer) stay distinct and correct after all four calls."""
    _, s = golden_inputs()
    vc, vs, ada = models(torch.bfloat16)
    s = s[:1].contiguous()
    st = video.VideoStylizer(vc, vs, ada)
    st.set_style(s)
    frames = [seeded_image(1, 64, 64, 20 + t).to(DEV) for t in range(4)]
    one = st.stylize_u8(frames[0][0], to_host=True)  # a [3][H][W] frame gives (H, W, 3)
    assert one.shape == (64, 64, 3)
    hosts = [st.stylize_u8(f, to_host=True) for f in frames]
    np.testing.assert_array_equal(one, hosts[0][0])
    # the last two u8 frames are kept for warping_error
    assert st.cur.dtype == torch.uint8 and st.prev.dtype == torch.uint8
    np.testing.assert_array_equal(st.cur.cpu().numpy(), hosts[3])
    np.testing.assert_array_equal(st.prev.cpu().numpy(), hosts[2])
    flow = (torch.rand(1, 2, 64, 64, generator=torch.Generator().manual_seed(5)) * 4 - 2).to(DEV)
    mask = (torch.rand(64, 64, generator=torch.Generator().manual_seed(6)) > 0.3).float().to(DEV)
    e = st.warping_error(flow, mask)
    prev01 = (st.prev.permute(0, 3, 1, 2).float() / 255.0).contiguous()
    cur01 = (st.cur.permute(0, 3, 1, 2).float() / 255.0).contiguous()
    assert torch.equal(e, video.warping_error(prev01, cur01, flow, mask))
    assert torch.equal(e, video.warping_error(st.prev, st.cur, flow, mask))
    assert float(e[0]) > 0
    # correct and distinct after the fact
    st2 = video.VideoStylizer(vc, vs, ada)
    st2.set_style(s)
    for t, f in enumerate(frames):
        np.testing.assert_array_equal(hosts[t], reference_frame(st2(f), True))
        assert hosts[t].flags.owndata
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(hosts[a], hosts[b])
            assert not np.shares_memory(hosts[a], hosts[b])
