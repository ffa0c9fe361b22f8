"""Plain-torch restatement of the InceptionV3 trunk of SIFID (SIFID/inception.py over torchvision's
inception_v3), a seeded weight recipe, and the fp64 Fréchet distance in its nuclear-norm form.

The restatement is independent of ``network.inception``: modules named as torchvision names them
(``Conv2d_1a_3x3`` ... ``Mixed_7c``, ``.conv.weight`` / ``.bn.*``), evaluated with F.conv2d / F.batch_norm /
F.*_pool2d in whatever dtype the module holds (fp32 or, after ``.double()``, fp64).  tests/golden/
make_sifid_goldens.py hands ``build_torchvision`` to the reference's own InceptionV3 class as a stand-in for
``torchvision.models.inception_v3``; the tests use ``trunk`` as the fp64 yardstick.

The ImageNet weights (21.8 M parameters) cannot be committed, so ``recipe`` draws stand-ins from a seed:
conv weights Kaiming-scaled (std sqrt(2 / fan_in)), BatchNorm gamma in [0.8, 1.2], beta and running_mean
N(0, 0.1^2), running_var in [0.8, 1.2] — every layer maps unit-scale activations to unit-scale activations,
so the values stay O(1) through all 94 layers.  The three BatchNorms of block 0 instead hold what running
statistics are, the per-channel mean and variance of their conv's output, taken on a seeded noise image at
the REFERENCE's input scale (2 v / 255 / 255 - 1, within 0.008 of -1): without that the trunk would carry a
constant plus 0.3 % of image content, the zero padding of the borders would dominate every covariance, and
d^2 would be a rounding residue of tr S.  The statistics are evaluated in fp64 and rounded to a coarse grid
(means to 2^-14, variances to three digits), so every machine draws the same bits.  The last of the three
variances is multiplied by 64, so block 0 leaves with a standard deviation near 1 / 8 at the reference's scale
and near 32 at the unit scale (255 times the input): covariances there stay small enough for scipy's sqrtm to
pass the reference's own acceptance, an absolute 1e-3 on the imaginary part (sifid_score.py:173-177).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, pad=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        x = F.conv2d(x, self.conv.weight, None, self.conv.stride, self.conv.padding)
        x = F.batch_norm(x, self.bn.running_mean, self.bn.running_var, self.bn.weight, self.bn.bias, False, 0.0, 0.001)
        return F.relu(x)


def _seq(x, *mods):
    for m in mods:
        x = m(x)
    return x


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1)  # count_include_pad=True: / 9 everywhere


class InceptionA(nn.Module):
    def __init__(self, cin, pf):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, pad=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, pad=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, pad=1)
        self.branch_pool = BasicConv2d(cin, pf, 1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), _seq(x, self.branch5x5_1, self.branch5x5_2),
                          _seq(x, self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3),
                          self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, pad=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), _seq(x, self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3),
                          F.max_pool2d(x, 3, 2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), pad=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), pad=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), pad=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), pad=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), pad=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), pad=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), _seq(x, self.branch7x7_1, self.branch7x7_2, self.branch7x7_3),
                          _seq(x, self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4,
                               self.branch7x7dbl_5), self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), pad=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), pad=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def forward(self, x):
        return torch.cat([_seq(x, self.branch3x3_1, self.branch3x3_2),
                          _seq(x, self.branch7x7x3_1, self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4),
                          F.max_pool2d(x, 3, 2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), pad=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), pad=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, pad=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), pad=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), pad=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        bd = _seq(x, self.branch3x3dbl_1, self.branch3x3dbl_2)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(bd),
                          self.branch3x3dbl_3b(bd), self.branch_pool(_avg(x))], 1)


class TorchvisionInception(nn.Module):
    """The submodules of torchvision's Inception3 that SIFID/inception.py takes, under torchvision's names."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, pad=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)


DIMS = (64, 192, 768, 2048)
_TAPS = (("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"), ("Conv2d_3b_1x1", "Conv2d_4a_3x3"),
         ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"),
         ("Mixed_7a", "Mixed_7b", "Mixed_7c"))


def recipe(seed: int = 20260) -> dict:
    """The seeded stand-in weights, fp32, under torchvision's state_dict names."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, t in TorchvisionInception().state_dict().items():
        if name.endswith("conv.weight"):
            fan_in = t.shape[1] * t.shape[2] * t.shape[3]
            sd[name] = torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif name.endswith(("bn.weight", "bn.running_var")):
            sd[name] = 0.8 + 0.4 * torch.rand(t.shape, generator=g)
        elif name.endswith(("bn.bias", "bn.running_mean")):
            sd[name] = 0.1 * torch.randn(t.shape, generator=g)
        else:
            sd[name] = t.clone()  # num_batches_tracked
    # block 0: running statistics of a noise image at the reference's input scale (see the module text)
    x = 2 * (torch.randint(0, 256, (1, 3, 41, 41), generator=g).double() / 255 / 255) - 1
    for name, stride, pad in (("Conv2d_1a_3x3", 2, 0), ("Conv2d_2a_3x3", 1, 0), ("Conv2d_2b_3x3", 1, 1)):
        y = F.conv2d(x, sd[name + ".conv.weight"].double(), None, stride, pad)
        mean = torch.round(y.mean((0, 2, 3)) * 2 ** 14) / 2 ** 14
        var = torch.tensor([float(f"{v:.3g}") for v in y.var((0, 2, 3), unbiased=False).tolist()], dtype=torch.float64)
        if name == "Conv2d_2b_3x3":
            var = var * 64  # block 0 leaves with a standard deviation of 1 / 8: see the module text
        sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = mean.float(), var.float()
        x = F.relu(F.batch_norm(y, mean, var, sd[name + ".bn.weight"].double(), sd[name + ".bn.bias"].double(), False, 0.0,
                                0.001))
    return sd


def build_torchvision(sd=None, dtype=torch.float32) -> TorchvisionInception:
    net = TorchvisionInception()
    net.load_state_dict(recipe() if sd is None else sd, strict=True)
    return net.to(dtype).eval()


@torch.no_grad()
def trunk(net: TorchvisionInception, x: torch.Tensor, last: int = 3):
    """The four taps (dims 64 / 192 / 768 / 2048; inception.py:63-103, 137-146) of x [B][3][H][W] in [0, 1],
    NCHW, in the dtype of ``net``; blocks after ``last`` are not run."""
    x = 2 * x.to(next(net.parameters()).dtype) - 1
    taps = []
    for b, names in enumerate(_TAPS[:last + 1]):
        if b in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = _seq(x, *[getattr(net, n) for n in names])
        taps.append(x)
    return taps


def rows(feat: torch.Tensor) -> np.ndarray:
    """[1][C][H][W] -> fp64 rows [H * W][C] (sifid_score.py:119)."""
    return feat[0].permute(1, 2, 0).reshape(-1, feat.shape[1]).double().numpy()


def moments64(x: np.ndarray):
    """(mu, tr S, centred rows) of fp64 rows [n][C], S = np.cov(rowvar=False)."""
    mu = x.mean(axis=0)
    xc = x - mu
    return mu, (xc * xc).sum() / (x.shape[0] - 1), xc


def fd64(x1: np.ndarray, x2: np.ndarray) -> float:
    """d^2 (sifid_score.py:128-182) of two sets of fp64 rows in the nuclear-norm form: the non-zero eigenvalues
    of S1 S2 are the squared singular values of Xc1 Xc2^T / sqrt((n1 - 1)(n2 - 1))."""
    (m1, t1, c1), (m2, t2, c2) = moments64(np.asarray(x1, np.float64)), moments64(np.asarray(x2, np.float64))
    m = c1 @ c2.T / np.sqrt((x1.shape[0] - 1.0) * (x2.shape[0] - 1.0))
    d = m1 - m2
    return float(d @ d + t1 + t2 - 2.0 * np.linalg.svd(m, compute_uv=False).sum())


def norm_rel(a, ref) -> float:
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
