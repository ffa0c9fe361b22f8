"""The bf16 training attention without a GPU: its entry points exist in ABI 18 (no bump) and validate
their arguments on the host, the Python ops refuse CPU tensors, and Trainer takes the
``attn_precision`` switch."""
import ctypes
import os

import pytest
import torch

from mhada_hip import _lib, autograd_path, ops
from mhada_hip.train import Trainer, VideoTrainer
from test_train_cpu import build

BF16_ENTRIES = ("mhada_attn_train_bf16_workspace", "mhada_attn_train_fwd_bf16", "mhada_attn_train_bwd_bf16")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_bf16_training_entries_were_added_to_abi_18():
    lib = _lib_or_skip()
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18
    for name in BF16_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_bf16_workspace_sizes():
    """Forward: Q, K rows + V'^T and the hi / lo planes of V'^2^T; backward: Q, Q^T, K, K^T, V' and the
    hi / lo planes of V'^2 as rows, dmo rows, the hi / lo planes of dmo^T — bf16, the transposed images
    padded to ceil64 columns, and D_row in fp32 — each rounded up to 256 bytes."""
    lib = _lib_or_skip()

    def seg(elems):
        return (2 * elems + 255) // 256 * 256

    for BH, Nc, Ns in ((2, 128, 64), (3, 100, 70), (1, 37, 300), (2, 33, 4), (1, 0, 5)):
        cP, sP = (Nc + 63) // 64 * 64, (Ns + 63) // 64 * 64
        fwd = seg(BH * Nc * 64) + seg(BH * Ns * 64) + 3 * seg(BH * 64 * sP)
        bwd = seg(BH * Nc * 64) + seg(BH * 64 * cP) + 4 * seg(BH * Ns * 64) + seg(BH * 64 * sP) \
            + seg(BH * Nc * 128) + 2 * seg(BH * 128 * cP) + seg(BH * Nc * 2)
        assert lib.mhada_attn_train_bf16_workspace(BH, Nc, Ns, 0) == fwd
        assert lib.mhada_attn_train_bf16_workspace(BH, Nc, Ns, 1) == bwd
    for bad in ((0, 4, 4), (2, -1, 4), (2, 4, 0), (2, (1 << 30) + 1, 4)):
        assert lib.mhada_attn_train_bf16_workspace(*bad, 0) == -1
        assert b"mhada_attn_train_bf16_workspace:" in lib.mhada_last_error()


def test_bf16_training_entries_reject_bad_arguments_without_a_launch():
    """A null pointer, non-positive sizes, sizes above 2^30 and a workspace that is missing, unaligned
    or too small return MHADA_ERR_ARG on the host (no GPU here: a launch would fail differently).  The
    pointers are host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 40

    def fwd(Nc=4, q=p, Ns=4, BH=2, ws=p, size=big):
        return lib.mhada_attn_train_fwd_bf16(q, p, p, p, p, p, p, ws, size, BH, Nc, Ns, None)

    def bwd(Nc=4, q=p, Ns=4, BH=2, ws=p, size=big, phases=3, lse=p, dmo=p, dq=p):
        return lib.mhada_attn_train_bwd_bf16(q, p, p, lse, dmo, p, dq, p, p, ws, size, BH, Nc, Ns, phases, None)

    for fn, name, back in ((fwd, BF16_ENTRIES[1], 0), (bwd, BF16_ENTRIES[2], 1)):
        for kw in (dict(q=None), dict(ws=None), dict(Nc=-1), dict(Ns=0), dict(Ns=-3), dict(BH=0)):
            assert fn(**kw) == 1, kw
            err = lib.mhada_last_error()
            assert name.encode() + b":" in err and b"bad args" in err
        assert fn(Nc=(1 << 30) + 1) == 1 and b"2^30" in lib.mhada_last_error()
        need = lib.mhada_attn_train_bf16_workspace(2, 4, 4, back)
        assert need > 0
        for kw in (dict(size=need - 1), dict(size=0), dict(ws=p + 4)):
            assert fn(**kw) == 1, kw
            err = lib.mhada_last_error()
            assert name.encode() + b":" in err and b"workspace" in err
    # the backward's phases: 1 (pre-pass) needs dmo but no outputs, 2 (kernels) the reverse
    for kw in (dict(phases=0), dict(phases=4), dict(phases=1, dmo=None), dict(phases=2, dq=None),
               dict(phases=2, lse=None), dict(phases=3, dmo=None), dict(phases=3, dq=None)):
        assert bwd(**kw) == 1, kw
        assert b"mhada_attn_train_bwd_bf16:" in lib.mhada_last_error() and b"bad args" in lib.mhada_last_error()
    # an empty query side is legal for the forward and for the pre-pass: nothing to launch
    assert fwd(Nc=0) == 0 and bwd(Nc=0, phases=1, lse=None, dq=None) == 0


def test_ops_need_device_tensors():
    q = torch.zeros(1, 4, 64)
    before = dict(ops.BF16_TRAIN_COUNTS)
    with pytest.raises(RuntimeError, match="need ROCm device tensors"):
        ops.attn_train_fwd_bf16(q, q, q, q)
    with pytest.raises(RuntimeError, match="need ROCm device tensors"):
        ops.attn_train_bwd_bf16(q, q, q, torch.zeros(1, 4), torch.zeros(1, 4, 128), torch.zeros(1, 4, 128))
    assert ops.BF16_TRAIN_COUNTS == before  # a refused call is not counted


def test_trainer_takes_the_attention_precision_switch():
    mods = build()
    assert Trainer(*mods).attn_precision == "fp32"
    assert Trainer(*mods, attn_precision="bf16").attn_precision == "bf16"
    assert VideoTrainer(*mods, attn_precision="bf16").attn_precision == "bf16"
    for bad in ("fp16", "BF16", "", None):
        with pytest.raises(ValueError, match="attn_precision"):
            Trainer(*mods, attn_precision=bad)


def test_train_attn_context_sets_and_restores_the_mode():
    assert autograd_path.TRAIN_ATTN == "hip"
    with autograd_path.train_attn("bf16"):
        assert autograd_path.TRAIN_ATTN == "bf16"
        with pytest.raises(RuntimeError):
            with autograd_path.train_attn("torch"):
                assert autograd_path.TRAIN_ATTN == "torch"
                raise RuntimeError("leave by exception")
        assert autograd_path.TRAIN_ATTN == "bf16"
    assert autograd_path.TRAIN_ATTN == "hip"
    with pytest.raises(ValueError):
        with autograd_path.train_attn("fp8"):
            pass
    assert autograd_path.TRAIN_ATTN == "hip"
    # the mode never moves CPU tensors off the aten path
    import network
    blk = network.AdaAttnTransformerMultiHead().adaAttnHead[0]
    with autograd_path.train_attn("bf16"):
        assert not autograd_path._fused_train_attn(blk, torch.zeros(1, 512, 2, 2))
