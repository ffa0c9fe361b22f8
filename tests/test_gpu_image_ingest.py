"""The device image ingest (csrc/image_ingest.hip, ops.image_resize, mhada_hip.image) against PIL's recorded
outputs (tests/golden/pil_resize.npz).  The operator is integer arithmetic: every comparison is exact, u8 byte
for byte and fp32 bit for bit.

The kernels' workgroup tile is 64 pixels along x by 4 rows (vertical pass and copy) or 16 rows (horizontal
pass): (96, 200) -> (70, 131) writes 3 ragged x tiles, 6 horizontal-pass row tiles and 18 ragged vertical-pass
row tiles; (37, 53) -> (16, 24) and (17, 90) -> (33, 8) leave the horizontal pass a ragged last row tile."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pil_resize_ref as R
from conftest import load_golden
from mhada_hip import image, metrics, ops

DEV = "cuda"
IDS = [R.case_name(c, k) for c in R.CASES for k in R.KINDS]
PAIRS = [(c, k) for c in R.CASES for k in R.KINDS]
BOTH = R.CASES[0]       # (37, 53) -> (16, 24): both passes
TILES = R.CASES[-1]     # (96, 200) -> (70, 131)


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("pil_resize")


def pair(case, kind):
    n = R.case_name(case, kind)
    return gold()["in_" + n], gold()["out_" + n]


def planar255(u8: np.ndarray) -> torch.Tensor:
    """toTensor255 of a u8 [..., H, W, 3] image on the CPU: (v / 255) * 255 in fp32, channels planar"""
    t = torch.from_numpy(np.ascontiguousarray(u8)).to(torch.float32)
    return ((t / 255.0) * 255.0).movedim(-1, -3).contiguous()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool((a.cpu().contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def run(x: np.ndarray, out_hw, **kw):
    return ops.image_resize(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), out_hw, **kw)


@pytest.mark.parametrize("case,kind", PAIRS, ids=IDS)
def test_matches_pil_goldens(case, kind):
    x, want = pair(case, kind)
    u8, f32 = run(x, case[1])
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1,) + want.shape
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (1, 3) + case[1]
    diff = int((u8[0].cpu().numpy() != want).sum())
    print(f"{R.case_name(case, kind)}: {diff} differing bytes of {want.size}")
    assert diff == 0
    assert same_bits(f32[0], planar255(want))


def test_batch_of_two_equals_the_single_calls():
    for case in (BOTH, TILES):
        xs = np.stack([pair(case, "rand")[0], pair(case, "bin")[0]])
        want = np.stack([pair(case, "rand")[1], pair(case, "bin")[1]])
        u8, f32 = run(xs, case[1])
        assert np.array_equal(u8.cpu().numpy(), want)
        assert same_bits(f32, planar255(want))


@pytest.mark.parametrize("case", [BOTH, R.CASES[3], R.CASES[8], R.CASES[2]], ids=["both", "horizontal", "vertical", "copy"])
def test_padded_source_rows_and_padded_output(case):
    """Source rows of 3W + 5 bytes (two images, so the image stride counts) give the same result; with out_u8 a
    view of a wider buffer prefilled with 0xA5, every byte outside the images is still 0xA5."""
    (H, W), (Ho, Wo) = case
    xs = np.stack([pair(case, "rand")[0], pair(case, "bin")[0]])
    want = np.stack([pair(case, "rand")[1], pair(case, "bin")[1]])
    rb = 3 * W + 5
    buf = torch.full((2 * H * rb + 7,), 0x5A, dtype=torch.uint8, device=DEV)
    src = buf[3:3 + 2 * H * rb].as_strided((2, H, W, 3), (H * rb, rb, 3, 1))  # misaligned start as well
    src.copy_(torch.from_numpy(xs).to(DEV))
    orb = 3 * Wo + 7
    obuf = torch.full((2 * Ho * orb + 9,), 0xA5, dtype=torch.uint8, device=DEV)
    out = obuf[1:1 + 2 * Ho * orb].as_strided((2, Ho, Wo, 3), (Ho * orb, orb, 3, 1))
    u8, f32 = ops.image_resize(src, (Ho, Wo), out_u8=out)
    assert u8 is out
    assert np.array_equal(out.cpu().numpy(), want) and same_bits(f32, planar255(want))
    host = obuf.cpu().numpy()
    assert host[0] == 0xA5 and (host[1 + 2 * Ho * orb:] == 0xA5).all()
    rows = host[1:1 + 2 * Ho * orb].reshape(2 * Ho, orb)
    assert (rows[:, 3 * Wo:] == 0xA5).all()


def test_bgr_equals_the_channel_flipped_image():
    for case in (BOTH, R.CASES[2]):
        x, want = pair(case, "rand")
        u8, f32 = run(x[..., ::-1], case[1], bgr=True)
        assert np.array_equal(u8[0].cpu().numpy(), want) and same_bits(f32[0], planar255(want))


def test_single_output_calls_agree_with_both():
    x, want = pair(TILES, "rand")
    u8, none = run(x, TILES[1], want_f32=False)
    assert none is None and np.array_equal(u8[0].cpu().numpy(), want)
    none, f32 = run(x, TILES[1], want_u8=False)
    assert none is None and same_bits(f32[0], planar255(want))
    with pytest.raises(ValueError):
        run(x, TILES[1], want_u8=False, want_f32=False)


def test_table_cache_hit_and_new_size():
    """A second call at the same sizes (a cache hit) is identical; a call at a new size after it is correct: the
    cache does not hand back another size's tables."""
    x, want = pair(BOTH, "rand")
    first = run(x, BOTH[1])[0][0].cpu().numpy()
    again = run(x, BOTH[1])[0][0].cpu().numpy()
    assert np.array_equal(first, want) and np.array_equal(again, want)
    other = run(x, (19, 31))[0][0].cpu().numpy()  # new sizes on both axes, not a golden case
    assert np.array_equal(other, R.resize(x, 19, 31))
    swapped = run(x, (24, 16))[0][0].cpu().numpy()  # 37 -> 24 and 53 -> 16: the cached n_out values, other n_in
    assert np.array_equal(swapped, R.resize(x, 24, 16))
    assert np.array_equal(run(x, BOTH[1])[0][0].cpu().numpy(), first)


def test_image_module_agrees_with_ops():
    (H, W), (Ho, Wo) = BOTH
    x, want = pair(BOTH, "bin")
    u8, f32 = image.prepare(x, (Wo, Ho))  # size = (width, height)
    assert tuple(u8.shape) == (Ho, Wo, 3) and tuple(f32.shape) == (3, Ho, Wo) and u8.is_cuda and f32.is_cuda
    assert np.array_equal(u8.cpu().numpy(), want) and same_bits(f32, planar255(want))
    du8, df32 = image.prepare(torch.from_numpy(x).to(DEV), (Wo, Ho), DEV)
    assert np.array_equal(du8.cpu().numpy(), want) and same_bits(df32, planar255(want))
    assert same_bits(image.pil_to_tensor(x, (Wo, Ho)), planar255(want))
    assert np.array_equal(image.resize_u8(x, (Wo, Ho)).cpu().numpy(), want)
    with pytest.raises(ValueError):
        image.prepare(x.astype(np.float32), (Wo, Ho))


def test_image_module_takes_a_pil_image():
    Image = pytest.importorskip("PIL.Image")
    (H, W), (Ho, Wo) = TILES
    x, want = pair(TILES, "rand")
    u8, f32 = image.prepare(Image.fromarray(x), (Wo, Ho))
    assert np.array_equal(u8.cpu().numpy(), want) and same_bits(f32, planar255(want))
    gray = Image.fromarray(x[..., 0])  # mode "L": converted to RGB as the reference's .convert("RGB") does
    want_gray = np.asarray(gray.convert("RGB").resize((Wo, Ho), Image.BILINEAR))
    assert np.array_equal(image.resize_u8(gray, (Wo, Ho)).cpu().numpy(), want_gray)


def test_resized_frames_feed_the_metrics():
    """Plumbing: resize_u8's layout is what metrics.ssim reads — identical images score exactly 1."""
    x, _ = pair(TILES, "rand")
    a = image.resize_u8(x, (131, 70))
    b = image.resize_u8(x.copy(), (131, 70))
    assert float(metrics.ssim(a, b)) == 1.0
