"""The SPLIT3 Winograd conv with one Winograd row per wave (wino_s3_rows_kernel, tuning wino_s3_rows = 1)
against wino_s3_kernel (wino_s3_rows = 0): the same MFMAs in the same order per accumulator and the same
transform and epilogue expressions, so the outputs are equal bit for bit (torch.equal) on every input.

Shapes: Cin 16 (one chunk, no steady state), 32 (the two-chunk unroll), 48 / 80 (odd chunk counts: the
tail branch); Cout 64 / 128 (the channel-block offset of the direct U loads); 16 x 16, 18 x 20 and 6 x 10
outputs at batch 2 (full blocks, partial 16 x 16 blocks, odd edge tiles); reflect pad, zero pad 1, zero
pad 2; bias / ReLU on and off, the mask, ldc = Cout + 4 over a NaN-filled buffer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"

SIZES = [(16, 16), (18, 20), (6, 10)]
B = 2


def conv(rows, x, u, bias, relu, pad_mode, pad, ldc, mask=None):
    Bn, H, W, _ = x.shape
    Ho, Wo = (H, W) if pad_mode == "reflect" else (H + 2 * (pad - 1), W + 2 * (pad - 1))
    out = torch.full((Bn, Ho, Wo, ldc), float("nan"), device=DEV)
    with _lib.tuning(wino_s3_rows=rows):
        return ops.conv3x3_wino(x, u, bias, relu, pad_mode, pad, out=out, relu_mask=mask)


def same(x, u, bias, relu, pad_mode, pad, ldc, Co, mask=None):
    y1 = conv(1, x, u, bias, relu, pad_mode, pad, ldc, mask)
    y0 = conv(0, x, u, bias, relu, pad_mode, pad, ldc, mask)
    assert not bool(torch.isnan(y0[..., :Co]).any())
    assert torch.equal(y1[..., :Co], y0[..., :Co])
    # columns past Cout are not touched by either kernel
    assert bool(torch.isnan(y1[..., Co:]).all()) and bool(torch.isnan(y0[..., Co:]).all())
    return y1


@pytest.mark.parametrize("pad_mode,pad", [("reflect", 1), ("zero", 1), ("zero", 2)])
@pytest.mark.parametrize("Co", [64, 128])
@pytest.mark.parametrize("Ci", [16, 32, 48, 80])
def test_wino_rows_bit_identical(Ci, Co, pad_mode, pad):
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + pad)
    w = (torch.randn(Co, 9 * Ci, generator=g) * (9 * Ci) ** -0.5).to(DEV)
    bias = torch.randn(Co, generator=g).to(DEV)
    u = ops.wino_weights(w)
    assert u.split3 is not None
    for Ho, Wo in SIZES:
        H, W = (Ho, Wo) if pad_mode == "reflect" else (Ho - 2 * (pad - 1), Wo - 2 * (pad - 1))
        x = (torch.rand(B, H, W, Ci, generator=g) * 400 - 120).to(DEV)
        mask = (torch.rand(B, Ho, Wo, Co + 4, generator=g) - 0.5).to(DEV)
        for b, relu in ((bias, True), (None, False), (bias, False), (None, True)):
            same(x, u, b, relu, pad_mode, pad, Co, Co)
        y = same(x, u, bias, True, pad_mode, pad, Co + 4, Co)
        ym = same(x, u, bias, True, pad_mode, pad, Co + 4, Co, mask)
        keep = mask[..., :Co] > 0
        assert torch.equal(ym[..., :Co], torch.where(keep, y[..., :Co], torch.zeros_like(y[..., :Co])))


@pytest.mark.parametrize("pad_mode,pad", [("reflect", 1), ("zero", 2)])
def test_wino_rows_wide_scales(pad_mode, pad):
    """Per-channel input scales 2^-20 .. 2^20 (the filter scaled inversely) and exact zeros, as in
    test_wino_split3_wide_scales: all three planes of V and U carry weight."""
    H, W, Ci, Co = 9, 13, 80, 128
    g = torch.Generator().manual_seed(11)
    sc = torch.exp2(torch.randint(-20, 21, (Ci,), generator=g).float())
    x = torch.randn(B, H, W, Ci, generator=g) * sc
    x[torch.rand(B, H, W, Ci, generator=g) < 0.1] = 0.0
    w = torch.randn(Co, 3, 3, Ci, generator=g) * (9 * Ci) ** -0.5 / sc.view(1, 1, 1, Ci)
    w[torch.rand(Co, 3, 3, Ci, generator=g) < 0.1] = 0.0
    u = ops.wino_weights(w.reshape(Co, -1).contiguous().to(DEV))
    bias = torch.randn(Co, generator=g).to(DEV)
    same(x.to(DEV), u, bias, False, pad_mode, pad, Co + 4, Co)
    same(x.to(DEV), u, None, True, pad_mode, pad, Co, Co)


def test_wino_rows_knob():
    """The knob is listed, takes 0 | 1 only, and the library reports what was set."""
    with _lib.tuning(wino_s3_rows=0):
        assert _lib.get_tuning("wino_s3_rows") == 0
    with pytest.raises(Exception):
        with _lib.tuning(wino_s3_rows=2):
            pass
