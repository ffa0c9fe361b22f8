"""The fused temporal losses (csrc/temporal.hip) without a GPU: the three entries are exported under
ABI 18, reject bad arguments on the host, and the public *_hip functions and VideoTrainer keep the
mhada_hip.losses route on the CPU."""
import ctypes
import os

import pytest
import torch

from mhada_hip import _lib
from mhada_hip import losses as L
from mhada_hip.video import feature_level_temporal_loss_hip, output_level_temporal_loss_hip

ENTRIES = ("mhada_temporal_loss_fwd", "mhada_temporal_loss_bwd", "mhada_flow_mask_resize")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_temporal_entries_are_exported_under_abi_18():
    lib = _lib_or_skip()
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_temporal_entries_reject_bad_arguments_without_a_launch():
    """A null pointer, a negative size and a misaligned pointer return MHADA_ERR_ARG on the host (no
    GPU here: a launch would fail differently).  The pointers are host addresses that are never
    dereferenced; the stride arrays are read on the host."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    st = (ctypes.c_longlong * 4)(3 * 4 * 4, 4 * 4, 4, 1)

    def fwd(x1=p, m=p, work=p, C=3, c1=None, c2=None, s1=st):
        return lib.mhada_temporal_loss_fwd(x1, s1, p, st, p, m, c1, c2, work, p, 1, C, 4, 4, None)

    def bwd(x2=p, dx1=p, sd1=st, work=p, H=4, g=p):
        return lib.mhada_temporal_loss_bwd(p, st, x2, st, p, p, None, None, work, g, dx1, sd1, p, st, 1, 3, H, 4, None)

    def resize(flow=p, fmask=p, Hf=2):
        return lib.mhada_flow_mask_resize(flow, p, p, fmask, 1, 4, 4, Hf, 2, None)

    bad = [(lambda: fwd(x1=None), "fwd"), (lambda: fwd(m=None), "fwd"), (lambda: fwd(work=None), "fwd"),
           (lambda: fwd(s1=None), "fwd"), (lambda: fwd(C=-1), "fwd"), (lambda: fwd(c1=p), "fwd"),
           (lambda: bwd(x2=None), "bwd"), (lambda: bwd(g=None), "bwd"), (lambda: bwd(sd1=None), "bwd"),
           (lambda: bwd(H=-4), "bwd"), (lambda: resize(flow=None), "resize"), (lambda: resize(Hf=-2), "resize"),
           (lambda: resize(Hf=0), "resize")]
    names = {"fwd": b"mhada_temporal_loss_fwd", "bwd": b"mhada_temporal_loss_bwd", "resize": b"mhada_flow_mask_resize"}
    for fn, which in bad:
        assert fn() == 1
        assert names[which] in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    neg = (ctypes.c_longlong * 4)(48, 16, -4, 1)
    assert fwd(s1=neg) == 1 and b"negative stride" in lib.mhada_last_error()
    misaligned = [(lambda: fwd(x1=p + 2), "fwd"), (lambda: fwd(work=p + 4), "fwd"), (lambda: bwd(dx1=p + 1), "bwd"),
                  (lambda: bwd(work=p + 4), "bwd"), (lambda: resize(fmask=p + 2), "resize")]
    for fn, which in misaligned:
        assert fn() == 1
        assert names[which] in lib.mhada_last_error() and b"misaligned" in lib.mhada_last_error()


def _inputs(seed=0, B=2, H=9, W=11, C=6, h=3, w=4):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    flow = 2.5 * r(B, 2, H, W)
    mask = (torch.rand(B, H, W, generator=g) > 0.3).float()
    return r(B, 3, H, W), r(B, 3, H, W), r(B, 3, H, W), r(B, 3, H, W), r(B, C, h, w), r(B, C, h, w), flow, mask


def test_hip_functions_on_cpu_tensors_equal_the_losses_module():
    c1, c2, cs1, cs2, f1, f2, flow, mask = _inputs()
    mse = torch.nn.MSELoss(reduction="none")
    cs1.requires_grad_(True)
    f1.requires_grad_(True)
    a = output_level_temporal_loss_hip(c1, c2, cs1, cs2, flow, mask)
    b = L.output_level_temporal_loss(c1, c2, cs1, cs2, flow, mask, mse)
    assert a.dim() == 0 and torch.equal(a, b)
    assert torch.equal(torch.autograd.grad(a, cs1)[0], torch.autograd.grad(b, cs1)[0])
    a = feature_level_temporal_loss_hip(f1, f2, flow, mask)
    b = L.feature_level_temporal_loss(f1, f2, flow, mask, mse)
    assert a.dim() == 0 and torch.equal(a, b)
    assert torch.equal(torch.autograd.grad(a, f1)[0], torch.autograd.grad(b, f1)[0])


def test_video_trainer_keeps_the_aten_losses_on_cpu_modules():
    from mhada_hip.train import Trainer, VideoTrainer
    from test_train_cpu import build
    mods = build()
    assert VideoTrainer(*mods).fused_temporal_losses is False
    assert not hasattr(Trainer(*mods), "fused_temporal_losses")
