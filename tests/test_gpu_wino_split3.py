"""The fp32 Winograd conv as SPLIT3 products on the bf16 MFMA (wino_s3_kernel, tuning wino_split3):
against fp64 conv2d at the bound of test_conv3x3_wino (norm-relative 2e-6), the filters' plane
prepack against the fp32 U bit for bit, and the dispatch (Cin % 16, the knob, determinism).

Measured on MI355X (worst case of each group; the bound stays 2e-6): see DESIGN §3a."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"

BOUND = 2e-6  # test_conv3x3_wino's


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def strip(u):
    """The same U without the plane image: conv3x3_wino then calls mhada_conv3x3_wino (wino4)."""
    v = u.clone()
    assert getattr(v, "split3", None) is None
    return v


def reference(x, w, bias, relu, pad_mode, pad):
    xn = x.permute(0, 3, 1, 2).double()
    xp = F.pad(xn, (1, 1, 1, 1), mode="reflect") if pad_mode == "reflect" else F.pad(xn, (pad,) * 4)
    ref = F.conv2d(xp, w.double(), None if bias is None else bias.double())
    return torch.relu(ref) if relu else ref


def check(x, w, b, pad_mode, pad, ldc, tag):
    """Both epilogue forms and the mask against fp64; returns the worst error ratio new / wino4."""
    B, H, W, Ci = x.shape
    Co = w.shape[0]
    wp = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous()
    u = ops.wino_weights(wp)
    assert u.split3.shape == (Ci // 16, 16, 3, Co, 16) and u.split3.dtype == torch.bfloat16
    u4 = strip(u)
    Ho, Wo = (H, W) if pad_mode == "reflect" else (H + 2 * (pad - 1), W + 2 * (pad - 1))
    mask = (torch.rand(B, Ho, Wo, ldc, generator=torch.Generator().manual_seed(Ci)) - 0.5).to(DEV)
    worst = 0.0
    for bias, relu in ((b, True), (None, False)):
        ref = reference(x, w, bias, relu, pad_mode, pad)
        out = torch.full((B, Ho, Wo, ldc), 7.0, device=DEV)
        y = ops.conv3x3_wino(x, u, bias, relu, pad_mode, pad, out=out)
        with _lib.tuning(wino_split3=0):
            y0 = ops.conv3x3_wino(x, u, bias, relu, pad_mode, pad, out=torch.full((B, Ho, Wo, ldc), 7.0, device=DEV))
        y4 = ops.conv3x3_wino(x, u4, bias, relu, pad_mode, pad, out=torch.full((B, Ho, Wo, ldc), 7.0, device=DEV))
        e, e4 = rel(y[..., :Co].permute(0, 3, 1, 2), ref), rel(y4[..., :Co].permute(0, 3, 1, 2), ref)
        print(f"{tag} {pad_mode}{pad} B{B} {H}x{W} {Ci}->{Co} relu={int(relu)}: split3 {e:.3e} wino4 {e4:.3e} "
              f"ratio {e / max(e4, 1e-30):.2f}")
        worst = max(worst, e / max(e4, 1e-30))
        assert e < BOUND and e4 < BOUND
        assert bool((y[..., Co:] == 7.0).all()) and bool((y4[..., Co:] == 7.0).all())
        # knob off: the parent's kernel and bits
        assert torch.equal(y0, y4)
        # two runs of the new kernel agree bit for bit
        y2 = ops.conv3x3_wino(x, u, bias, relu, pad_mode, pad, out=torch.full((B, Ho, Wo, ldc), 7.0, device=DEV))
        assert torch.equal(y, y2)
        # the folded ReLU adjoint: zero exactly where mask <= 0, the same values elsewhere
        ym = ops.conv3x3_wino(x, u, bias, relu, pad_mode, pad, out=torch.full((B, Ho, Wo, ldc), 7.0, device=DEV),
                              relu_mask=mask)
        keep = mask[..., :Co] > 0
        assert torch.equal(ym[..., :Co], torch.where(keep, y[..., :Co], torch.zeros_like(y[..., :Co])))
        assert bool((ym[..., Co:] == 7.0).all())
    return worst


# Cin 16 / 32 / 48 / 64 / 256: one chunk, the ring wrap, an odd chunk count, many chunks; Cout 64 /
# 128 / 192; grids of one partial tile, partial tiles on both axes and several blocks; ldc > Cout
SHAPES = [(1, 2, 2, 16, 64, 64), (2, 3, 2, 32, 128, 132), (1, 9, 13, 48, 64, 64), (3, 17, 70, 256, 64, 64),
          (2, 33, 20, 64, 192, 196), (1, 9, 13, 256, 128, 128)]


@pytest.mark.parametrize("pad_mode,pad", [("reflect", 1), ("zero", 1), ("zero", 2)])
@pytest.mark.parametrize("B,H,W,Ci,Co,ldc", SHAPES)
def test_wino_split3_fp64(pad_mode, pad, B, H, W, Ci, Co, ldc):
    """Inputs at the decoder's scale (values up to a few hundred)."""
    x = (torch.rand(B, H, W, Ci, generator=torch.Generator().manual_seed(H * W + Ci)) * 400 - 120).to(DEV)
    w = rnd(Co, Ci, 3, 3, scale=(9 * Ci) ** -0.5, seed=2)
    check(x, w, rnd(Co, seed=3), pad_mode, pad, ldc, "scale")


@pytest.mark.parametrize("pad_mode,pad", [("reflect", 1), ("zero", 2)])
def test_wino_split3_wide_scales(pad_mode, pad):
    """Per-channel scales spread over 2^-20 .. 2^20 (input and filter scaled inversely, so every
    channel contributes alike and the second and third planes carry weight) and exact zeros."""
    B, H, W, Ci, Co = 2, 9, 13, 64, 128
    g = torch.Generator().manual_seed(11)
    sc = torch.exp2(torch.randint(-20, 21, (Ci,), generator=g).float())
    x = torch.randn(B, H, W, Ci, generator=g) * sc
    x[torch.rand(B, H, W, Ci, generator=g) < 0.1] = 0.0
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5 / sc.view(1, Ci, 1, 1)
    w[torch.rand(Co, Ci, 3, 3, generator=g) < 0.1] = 0.0
    check(x.to(DEV), w.to(DEV), rnd(Co, seed=3), pad_mode, pad, Co, "wide")


@pytest.mark.parametrize("Ci,Co", [(16, 64), (48, 128), (256, 192)])
def test_wino_split3_prepack_bit_exact(Ci, Co):
    """p0 + p1 + p2 of the plane image, summed smallest first in fp32, is the fp32 U."""
    wp = rnd(Co, 9 * Ci, scale=(9 * Ci) ** -0.5, seed=5)
    u = ops.wino_weights(wp)
    up = ops.wino_weights_split3(wp).float()  # [Ci/16][16][3][Co][16]
    s = (up[:, :, 2] + up[:, :, 1]) + up[:, :, 0]
    uu = u.view(Ci // 16, 2, 16, Co, 8).permute(0, 2, 3, 1, 4).reshape(Ci // 16, 16, Co, 16)
    assert torch.equal(s, uu)
    assert torch.equal(u.split3.float(), up)


@pytest.mark.parametrize("Ci", [8, 24])
def test_wino_split3_routing_cin(Ci):
    """Cin % 16 != 0 stays on wino4 whatever the knob."""
    x = (torch.rand(2, 9, 13, Ci, generator=torch.Generator().manual_seed(Ci)) - 0.3).to(DEV)
    wp = rnd(64, 9 * Ci, scale=(9 * Ci) ** -0.5, seed=2)
    u = ops.wino_weights(wp)
    assert getattr(u, "split3", None) is None
    outs = []
    for knob in (0, 1):
        with _lib.tuning(wino_split3=knob):
            outs.append(ops.conv3x3_wino(x, u, None, True))
    with _lib.tuning(wino_split3=1, wino4=1):
        y4 = ops.conv3x3_wino(x, strip(u), None, True)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], y4)
