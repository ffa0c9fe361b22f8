"""Frame emit, host side: video.tensor_to_cv2 on CPU tensors against the reference's output expression
(infer_video.py:94,110-112), its argument errors, and the byte bookkeeping of the HIP kernels' row
stores (csrc/ingest.hip frame_emit_kernel, csrc/common.h emit_store_px) restated in Python."""
import numpy as np
import pytest
import torch

from mhada_hip import video

SPECIALS = [0.0, -0.0, 0.99999994, 1.0, 254.99998, 255.0, 255.5, 256.0, -3.0, 1e30, float("inf"), float("-inf")]


def reference_frame(cs: torch.Tensor, bgr: bool) -> np.ndarray:
    """The literal reference expression: clamp -> permute -> numpy().astype(np.uint8) (-> RGB2BGR)."""
    out = cs.clamp(0, 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    return out[..., ::-1] if bgr else out


def special_tensor():
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 5, 7, generator=g) * 300 - 20  # uniform noise in [-20, 280]
    flat = x.view(-1)
    step = flat.numel() // len(SPECIALS)
    for i, v in enumerate(SPECIALS):
        flat[i * step] = v
    return x


@pytest.mark.parametrize("bgr", [True, False])
def test_tensor_to_cv2_cpu_equals_reference_expression(bgr):
    x = special_tensor()
    for v in SPECIALS:
        assert (x == v).any()
    got = video.tensor_to_cv2(x, bgr=bgr)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (2, 5, 7, 3)
    np.testing.assert_array_equal(got, reference_frame(x, bgr))
    one = video.tensor_to_cv2(x[1], bgr=bgr)
    assert one.shape == (5, 7, 3)
    np.testing.assert_array_equal(one, reference_frame(x, bgr)[1])
    # what the specials must come out as (truncation, not rounding; saturation at both ends)
    want = dict(zip(SPECIALS, [0, 0, 0, 1, 254, 255, 255, 255, 0, 255, 255, 0]))
    ref = reference_frame(x, False)
    for v, u in want.items():
        idx = (x.permute(0, 2, 3, 1) == v).numpy()
        assert (ref[idx] == u).all(), (v, u)


def test_tensor_to_cv2_argument_errors():
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(5, 7))                 # wrong rank
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(1, 2, 3, 5, 7))        # wrong rank
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(2, 4, 5, 7))           # channel count != 3
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(4, 5, 7))
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(3, 5, 7, dtype=torch.uint8))   # non-float dtype
    with pytest.raises(ValueError):
        video.tensor_to_cv2(torch.zeros(1, 3, 5, 7, dtype=torch.int32))


# ---- the kernels' head / body / tail split of a row, restated --------------------------------------
# No Python helper computes it (the wrappers pass row_bytes through); these transcribe the device code.
EMIT_SEG = 1024  # kEmitSeg, csrc/ingest.hip


def emit_row_stores(W, misalign):
    """frame_emit_kernel: the (row offset, width) of every store one row receives, the row starting
    `misalign` bytes past a 4-byte boundary.  Per segment of EMIT_SEG pixels: m = (address of its first
    byte) & 3, its n bytes sit at LDS [m, m + n); a whole LDS dword inside that range is one 4-byte
    store to the aligned address, a dword straddling an end is byte stores of the bytes inside."""
    stores = []
    for xs in range(0, W, EMIT_SEG):
        npx = min(EMIT_SEG, W - xs)
        start = 3 * xs                      # row offset of the segment's first byte
        m = (misalign + start) & 3
        n = 3 * npx
        d = 0
        while 4 * d < m + n:
            if 4 * d >= m and 4 * d + 4 <= m + n:
                assert (misalign + start - m + 4 * d) % 4 == 0   # the dword store is aligned
                stores.append((start - m + 4 * d, 4))
            else:
                for k in range(4):
                    if m <= 4 * d + k < m + n:
                        stores.append((start - m + 4 * d + k, 1))
            d += 1
    return stores


def fused_row_stores(W, misalign):
    """emit_store_px in the tile kernels of the last decoder layer: lanes x & 3 = 0..3 hold four
    consecutive pixels; a complete group ((x | 3) < W) whose first byte is 4-byte aligned leaves as
    three dword stores from lanes 0..2, every other pixel as three byte stores."""
    stores = []
    for x in range(W):
        q = x & 3
        if (x | 3) < W and (misalign + 3 * (x - q)) % 4 == 0:
            if q < 3:
                stores.append((3 * (x - q) + 4 * q, 4))
        else:
            stores += [(3 * x + k, 1) for k in range(3)]
    return stores


@pytest.mark.parametrize("split", [emit_row_stores, fused_row_stores])
@pytest.mark.parametrize("W", [1, 2, 3, 5, 21, 64, 67, 1024, 1030, 2049])
def test_row_split_covers_every_byte_once(W, split):
    for mis in range(4):
        hits = np.zeros(3 * W + 8, dtype=np.int64)
        for off, width in split(W, mis):
            assert 0 <= off and off + width <= 3 * W, (W, mis, off, width)  # no byte beyond 3W (or before the row)
            hits[off:off + width] += 1
        assert (hits[:3 * W] == 1).all(), (W, mis)
        assert (hits[3 * W:] == 0).all()
        if split is emit_row_stores and W <= EMIT_SEG:
            # head < 4 bytes, tail < 4 bytes, the body in dwords
            singles = sum(1 for _, w in split(W, mis) if w == 1)
            assert singles <= 6
