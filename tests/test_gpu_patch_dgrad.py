"""mhada_patch_embed_dgrad (csrc/patch_dgrad.hip): the image gradient of the ViT's 8x8 / stride-8 patch
embedding, through ops.patch_embed_dgrad and train_fns.PatchEmbedFn, against the fp64
F.conv_transpose2d / F.conv2d autograd of the same layer (vit.py:105-117)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mhada_hip import ops, train_fns

DEV = "cuda"


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def ref64(dy, w, H, W):
    """fp64 conv_transpose2d of the token rows (CPU), zero rows below the last full patch."""
    B, N, C = dy.shape
    h, wp = H // 8, W // 8
    g = dy.double().cpu().view(B, h, wp, C).permute(0, 3, 1, 2)
    out = F.conv_transpose2d(g, w.double().cpu(), stride=8)
    return F.pad(out, (0, 0, 0, H - 8 * h))


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


SHAPES = [(1, 8, 8), (2, 24, 40), (1, 16, 264), (3, 72, 128), (1, 76, 64)]


@pytest.mark.parametrize("B,H,W,C", [(*s, 512) for s in SHAPES] + [(2, 24, 40, 256), (2, 24, 40, 1024)])
def test_exact_on_integers(B, H, W, C):
    """dy in [-8, 8], W in [-4, 4]: every partial sum is an integer below 2^24, so fp32 is exact in
    any order and the result equals the fp64 reference bit for bit — every index of the gather, the
    ragged strips (33 tokens per row) and the zero rows of H % 8 included.  The output buffer starts
    as NaN: every element must be written."""
    N = (H // 8) * (W // 8)
    dy = ints((B, N, C), -8, 8, 1).to(DEV)
    w = ints((C, 3, 8, 8), -4, 4, 2).to(DEV)
    out = torch.full((B, 3, H, W), float("nan"), device=DEV)
    res = ops.patch_embed_dgrad(dy, w, H, W, out=out)
    assert res is out
    got = out.cpu()
    assert not torch.isnan(got).any()
    ref = ref64(dy, w, H, W)
    assert torch.equal(got.double(), ref)
    if H % 8:
        assert torch.equal(got[:, :, 8 * (H // 8):], torch.zeros(B, 3, H % 8, W))
    # the allocating form returns the same values
    assert torch.equal(ops.patch_embed_dgrad(dy, w, H, W).cpu(), got)


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (3, 72, 128)])
def test_random_against_fp64_and_deterministic(B, H, W):
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(B, (H // 8) * (W // 8), 512, generator=g).to(DEV)
    w = (torch.randn(512, 3, 8, 8, generator=g) * 0.05).to(DEV)
    a = ops.patch_embed_dgrad(dy, w, H, W)
    e = rel(a.cpu(), ref64(dy, w, H, W))
    print(f"patch_embed_dgrad ({B}, {H}, {W}) rel vs fp64: {e:.3e}")
    assert e < 1e-5
    assert torch.equal(a, ops.patch_embed_dgrad(dy, w, H, W))  # same bits on a second call


def test_argument_errors():
    dy = torch.zeros(1, 6, 512, device=DEV)
    w = torch.zeros(512, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="mhada_patch_embed_dgrad.*multiple of 8"):
        ops.patch_embed_dgrad(dy[:, :4].contiguous(), w, 16, 20)  # W % 8 != 0
    with pytest.raises(ValueError, match="mhada_patch_embed_dgrad.*Ci must be 3"):
        ops.patch_embed_dgrad(dy, torch.zeros(512, 4, 8, 8, device=DEV), 16, 24)
    with pytest.raises(ValueError, match="mhada_patch_embed_dgrad.*multiple of 64"):
        ops.patch_embed_dgrad(torch.zeros(1, 6, 96, device=DEV), torch.zeros(96, 3, 8, 8, device=DEV), 16, 24)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.patch_embed_dgrad(torch.zeros(1, 512, 6, device=DEV).transpose(1, 2), w, 16, 24)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.patch_embed_dgrad(dy.double(), w, 16, 24)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.patch_embed_dgrad(dy, w.bfloat16(), 16, 24)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.patch_embed_dgrad(dy, w, 16, 24, out=torch.zeros(1, 3, 16, 24, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="do not match"):
        ops.patch_embed_dgrad(dy, w, 16, 32)
    ops.patch_embed_dgrad(dy, w, 16, 24)  # the valid call of the same operands


def test_patch_embed_fn_all_three_gradients():
    """Image, weight and bias all require grad: the three gradients against the fp64 conv2d autograd."""
    B, H, W = 2, 64, 64
    img = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(25)) * 255).to(DEV).requires_grad_(True)
    conv = torch.nn.Conv2d(3, 512, 8, stride=8).to(DEV)
    y = train_fns.PatchEmbedFn.apply(img, conv.weight, conv.bias)
    gy = torch.randn(*y.shape, generator=torch.Generator().manual_seed(26)).to(DEV)
    y.backward(gy)
    i64 = img.detach().double().cpu().requires_grad_(True)
    w64 = conv.weight.detach().double().cpu().requires_grad_(True)
    b64 = conv.bias.detach().double().cpu().requires_grad_(True)
    r = F.conv2d(i64, w64, b64, stride=8).flatten(2).transpose(1, 2)
    r.backward(gy.double().cpu())
    assert rel(y.cpu(), r) < 1e-5
    assert img.grad.shape == img.shape and img.grad.dtype == torch.float32
    assert rel(img.grad.cpu(), i64.grad) < 1e-5
    assert rel(conv.weight.grad.cpu(), w64.grad) < 1e-5 and rel(conv.bias.grad.cpu(), b64.grad) < 1e-5
