"""InceptionV3 trunk of SIFID — drop-in for ``MHAdaSTr/SIFID/inception.py:6-148``.

The reference takes torchvision's ``inception_v3`` with ImageNet weights (a network fetch this package
cannot make) and regroups its submodules as ``self.blocks``; here the same modules are built under the
same names, so the state_dict keys are the reference's, ``blocks.{b}.{i}[.branch…].{conv.weight,bn.*}``,
and a local torchvision checkpoint loads through ``load_torchvision``.  Blocks beyond
``max(output_blocks)`` are neither built nor run (inception.py:73-103).

``forward`` takes the image in [0, 1], NCHW, applies ``2 x - 1`` (inception.py:137-138) and returns the
feature MAPS of the selected blocks (no average pool: block 3 ends at Mixed_7c).  On a ROCm device it
runs the HIP kernels of csrc/conv2d.hip (fp32 NHWC; the first conv, whose input the reference's scale puts
within 0.008 of a constant, as a direct kernel evaluated in fp64; every conv with its eval-mode BatchNorm and
ReLU fused, every branch writing its slice of the block's concat buffer; inference only) and returns NCHW
views of NHWC storage; on the CPU aten.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _path  # noqa: F401
from mhada_hip import ops


class BasicConv2d(nn.Module):
    """torchvision's BasicConv2d: Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU."""

    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)
        self._pack = None

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)

    def _packed(self, device):
        """(filter [Cout][KH][KW][Cin'], scale, shift) on the device: the eval-mode BatchNorm as two fp32
        vectors, scale = gamma / sqrt(var + eps) and shift = beta - mean * scale evaluated in fp64.
        Rebuilt when a parameter or buffer was written or moved."""
        ts = (self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        key = (device,) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._pack is None or self._pack[0] != key:
            g, b, m, v = (t.detach().double() for t in ts[1:])
            scale = g / torch.sqrt(v + self.bn.eps)
            shift = b - m * scale
            self._pack = (key, ops.conv2d_pack_weight(self.conv.weight).to(device),
                          scale.float().contiguous().to(device), shift.float().contiguous().to(device),
                          scale.contiguous().to(device), shift.contiguous().to(device))
        return self._pack[1:]

    def hip(self, x, out=None, c_off=0):
        if self.training:
            raise NotImplementedError("network.InceptionV3 on the device is inference only: call .eval()")
        w, scale, shift = self._packed(x.device)[:3]
        return ops.conv2d(x, w, scale, shift, stride=self.conv.stride[0], padding=self.conv.padding, out=out, c_off=c_off)

    def hip_stem(self, image, normalize):
        """The trunk's first layer on the NCHW image: the direct fp64 kernel (csrc/conv2d.hip, "the stem"), with
        the BatchNorm's scale and shift kept in fp64."""
        if self.training:
            raise NotImplementedError("network.InceptionV3 on the device is inference only: call .eval()")
        w, _, _, scale64, shift64 = self._packed(image.device)
        return ops.conv2d_stem(image, w, scale64, shift64, stride=self.conv.stride[0], padding=self.conv.padding,
                               normalize=normalize)


def _buf(x, hw, c):
    return torch.empty(x.shape[0], hw[0], hw[1], c, device=x.device, dtype=torch.float32)


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)
        self.cout = 224 + pool_features

    def forward(self, x):
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b5, b3, bp], 1)

    def hip(self, x):
        out = _buf(x, x.shape[1:3], self.cout)
        self.branch1x1.hip(x, out, 0)
        self.branch5x5_2.hip(self.branch5x5_1.hip(x), out, 64)
        self.branch3x3dbl_3.hip(self.branch3x3dbl_2.hip(self.branch3x3dbl_1.hip(x)), out, 128)
        self.branch_pool.hip(ops.avgpool3(x), out, 224)
        return out


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)
        self.cout = 480 + cin

    def forward(self, x):
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)

    def hip(self, x):
        out = _buf(x, ops.conv2d_out_hw(x.shape[1], x.shape[2], (3, 3), 2, (0, 0)), self.cout)
        self.branch3x3.hip(x, out, 0)
        self.branch3x3dbl_3.hip(self.branch3x3dbl_2.hip(self.branch3x3dbl_1.hip(x)), out, 384)
        ops.maxpool3s2(x, out, 480)
        return out


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def _chains(self):
        return ((self.branch7x7_1, self.branch7x7_2, self.branch7x7_3),
                (self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5))

    def forward(self, x):
        outs = [self.branch1x1(x)]
        for chain in self._chains():
            y = x
            for m in chain:
                y = m(y)
            outs.append(y)
        outs.append(self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1)))
        return torch.cat(outs, 1)

    def hip(self, x):
        out = _buf(x, x.shape[1:3], 768)
        self.branch1x1.hip(x, out, 0)
        for off, chain in zip((192, 384), self._chains()):
            y = x
            for m in chain[:-1]:
                y = m.hip(y)
            chain[-1].hip(y, out, off)
        self.branch_pool.hip(ops.avgpool3(x), out, 576)
        return out


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)
        self.cout = 512 + cin

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)

    def hip(self, x):
        out = _buf(x, ops.conv2d_out_hw(x.shape[1], x.shape[2], (3, 3), 2, (0, 0)), self.cout)
        self.branch3x3_2.hip(self.branch3x3_1.hip(x), out, 0)
        self.branch7x7x3_4.hip(self.branch7x7x3_3.hip(self.branch7x7x3_2.hip(self.branch7x7x3_1.hip(x))), out, 320)
        ops.maxpool3s2(x, out, 512)
        return out


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b3, bd, bp], 1)

    def hip(self, x):
        out = _buf(x, x.shape[1:3], 2048)
        self.branch1x1.hip(x, out, 0)
        b3 = self.branch3x3_1.hip(x)
        self.branch3x3_2a.hip(b3, out, 320)
        self.branch3x3_2b.hip(b3, out, 704)
        bd = self.branch3x3dbl_2.hip(self.branch3x3dbl_1.hip(x))
        self.branch3x3dbl_3a.hip(bd, out, 1088)
        self.branch3x3dbl_3b.hip(bd, out, 1472)
        self.branch_pool.hip(ops.avgpool3(x), out, 1856)
        return out


# torchvision's module names in the order of the reference's blocks (inception.py:63-103); None = the
# MaxPool2d(3, 2) that opens blocks 1 and 2
_BLOCKS = (
    ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"),
    (None, "Conv2d_3b_1x1", "Conv2d_4a_3x3"),
    (None, "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"),
    ("Mixed_7a", "Mixed_7b", "Mixed_7c"),
)
_BUILD = {
    "Conv2d_1a_3x3": lambda: BasicConv2d(3, 32, kernel_size=3, stride=2),
    "Conv2d_2a_3x3": lambda: BasicConv2d(32, 32, kernel_size=3),
    "Conv2d_2b_3x3": lambda: BasicConv2d(32, 64, kernel_size=3, padding=1),
    "Conv2d_3b_1x1": lambda: BasicConv2d(64, 80, kernel_size=1),
    "Conv2d_4a_3x3": lambda: BasicConv2d(80, 192, kernel_size=3),
    "Mixed_5b": lambda: InceptionA(192, 32),
    "Mixed_5c": lambda: InceptionA(256, 64),
    "Mixed_5d": lambda: InceptionA(288, 64),
    "Mixed_6a": lambda: InceptionB(288),
    "Mixed_6b": lambda: InceptionC(768, 128),
    "Mixed_6c": lambda: InceptionC(768, 160),
    "Mixed_6d": lambda: InceptionC(768, 160),
    "Mixed_6e": lambda: InceptionC(768, 192),
    "Mixed_7a": lambda: InceptionD(768),
    "Mixed_7b": lambda: InceptionE(1280),
    "Mixed_7c": lambda: InceptionE(2048),
}
_IGNORED = ("AuxLogits.", "fc.")  # and the key "transform_input", if a checkpoint carries it


class InceptionV3(nn.Module):
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}  # inception.py:14-19

    def __init__(self, output_blocks=[DEFAULT_BLOCK_INDEX], resize_input=False, normalize_input=True,
                 requires_grad=False):
        super().__init__()
        if resize_input:
            raise NotImplementedError("network.InceptionV3: resize_input=True (the bilinear resize to 299 x 299) is not "
                                      "ported; the reference's SIFID runs with resize_input=False")
        output_blocks = [int(b) for b in output_blocks]
        if not output_blocks or min(output_blocks) < 0 or max(output_blocks) > 3:
            raise ValueError(f"network.InceptionV3: output_blocks must be block indices 0..3, got {output_blocks}")
        self.resize_input = False
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        self.blocks = nn.ModuleList()
        for names in _BLOCKS[:self.last_needed_block + 1]:
            self.blocks.append(nn.Sequential(*[nn.MaxPool2d(kernel_size=3, stride=2) if n is None else _BUILD[n]()
                                               for n in names]))
        for p in self.parameters():
            p.requires_grad = requires_grad
        self.eval()

    def forward(self, inp):
        if inp.is_cuda:
            if torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in self.parameters())):
                raise NotImplementedError("network.InceptionV3 on the device is inference only (no gradients)")
            return self._forward_hip(inp)
        x = 2 * inp - 1 if self.normalize_input else inp
        outp = []
        for idx, block in enumerate(self.blocks):
            x = block(x)
            if idx in self.output_blocks:
                outp.append(x)
        return outp

    @torch.no_grad()
    def _forward_hip(self, inp):
        x = self.blocks[0][0].hip_stem(inp.float(), self.normalize_input)  # 2 x - 1 is fused into the stem
        outp = []
        for idx, block in enumerate(self.blocks):
            for j, m in enumerate(block):
                if idx == 0 and j == 0:
                    continue
                x = ops.maxpool3s2(x) if isinstance(m, nn.MaxPool2d) else m.hip(x)
            if idx in self.output_blocks:
                outp.append(x.permute(0, 3, 1, 2))
        return outp

    @staticmethod
    def torchvision_names():
        """{torchvision module name: this class's module path}, for all four blocks."""
        return {n: f"blocks.{b}.{i}" for b, names in enumerate(_BLOCKS) for i, n in enumerate(names) if n is not None}

    def load_torchvision(self, src) -> None:
        """ImageNet weights from a LOCAL torchvision checkpoint — the file that
        ``models.inception_v3(weights="Inception_V3_Weights.IMAGENET1K_V1")`` (inception.py:60) downloads
        (``inception_v3_google-1a9a5a14.pth``), a path to it or its state_dict, loaded with
        ``weights_only=True``: ``Conv2d_1a_3x3.*``, ``Mixed_5b.*`` ... load into ``blocks.{b}.{i}.*``.
        ``AuxLogits.*``, ``fc.*`` and ``transform_input`` are ignored, and so are the layers of blocks this
        instance did not build; any other key is an error, every tensor of the built blocks must be
        present (``num_batches_tracked`` excepted, which old checkpoints lack) and shapes must match."""
        sd = torch.load(src, map_location="cpu", weights_only=True) if not isinstance(src, dict) else src
        names = self.torchvision_names()
        own = {}
        for key, val in sd.items():
            if key == "transform_input" or key.startswith(_IGNORED):
                continue
            head, _, rest = key.partition(".")
            if head not in names or not rest:
                raise KeyError(f"load_torchvision: unexpected key {key}")
            if int(names[head].split(".")[1]) <= self.last_needed_block:
                own[f"{names[head]}.{rest}"] = val
        want = [k for k in self.state_dict() if not k.endswith("num_batches_tracked")]
        missing = [k for k in want if k not in own]
        if missing:
            raise KeyError(f"load_torchvision: {len(missing)} tensors missing, first {missing[0]}")
        self.load_state_dict(own, strict=True)
