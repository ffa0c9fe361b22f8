"""Tensor-level wrappers over the C-ABI (one function per entry point of include/mhada_hip.h).

Every wrapper takes ROCm device tensors, validates shapes/dtypes on the host, launches on the
current stream of the operands' device (with that device made current for the call, so modules
moved with ``.to('cuda:1')`` work without ``set_device``) and allocates outputs through the
torch caching allocator (the library itself never allocates).  No wrapper has a CPU or aten
fallback.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import A_CONV3X3, A_CONV3X3_UP2, A_CONV3X3_ZERO, A_PATCH8, A_ROWS, A_SPLIT3, BF16, BF16X3, F32, GemmArgs, GemmTnArgs

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype}; the HIP path computes in float32 or bfloat16")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_gpu(*ts: Optional[torch.Tensor]) -> None:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("mhada_hip ops need ROCm device tensors (the MI355X path has no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"mhada_hip ops need all operands on one device, got {dev} and {t.device}")


def _call(name: str, dev_tensor: torch.Tensor, *args) -> None:
    """Launch entry point ``name`` with ``dev_tensor``'s device current, on that device's current
    stream (appended as the last argument); raise on a non-zero status."""
    idx = dev_tensor.device.index
    guard = contextlib.nullcontext() if idx is None or idx == torch.cuda.current_device() \
        else torch.cuda.device(idx)
    with guard:
        rc = getattr(_lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, name)


def gemm(*, a: torch.Tensor, w: torch.Tensor, c: torch.Tensor, M: int, N: int, K: int,
         compute: torch.dtype, a_mode: int = A_ROWS, lda: int = 0, sa=(0, 0), nb=(1, 1),
         a_mu: Optional[torch.Tensor] = None, smu=(0, 0), img=(0, 0, 0),
         ldw: int = 0, sw=(0, 0), bias: Optional[torch.Tensor] = None, sb=(0, 0),
         r: Optional[torch.Tensor] = None, ldr: int = 0, sr=(0, 0),
         ldc: int = 0, sc=(0, 0), relu: bool = False, pad: int = 0,
         c2: Optional[torch.Tensor] = None, ldc2: int = 0, sc2=(0, 0),
         vt: Optional[torch.Tensor] = None, ldt: int = 0, svt=(0, 0), c2_planes: bool = False,
         col_scale: Optional[torch.Tensor] = None, out_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_gemm``: C[z] = act(A[z] W[z]^T + bias[z]) + R[z]; strides in elements.  Optional
    c2 (a bf16 copy of an fp32 C; ``c2_planes``: C's three bf16 planes [3][M][ldc2], the next
    SPLIT3 GEMM's operand, with C None = not written) and vt (the transposed V' image of the
    K|V' projection).  ``col_scale`` (fp32 [N]): ``mhada_gemm_half2`` on fp16 HALF2 operands instead;
    with ``out_scale`` (fp32 [N]) ``mhada_gemm_half2_planes``: c2 is fp16 [2][M][ldc2], the HALF2 planes of
    out_scale[n] times the fp32 result, and C may be None."""
    _need_gpu(a, w, c, a_mu, bias, r, c2, vt, col_scale, out_scale)
    half2 = col_scale is not None
    if half2 and (a.dtype != torch.float16 or col_scale.dtype != torch.float32 or col_scale.numel() < N):
        raise ValueError("col_scale (fp32 [N]) goes with fp16 HALF2 operands")
    h2out = out_scale is not None
    if h2out and (not half2 or c2 is None or c2.dtype != torch.float16 or c2_planes
                  or out_scale.dtype != torch.float32 or out_scale.numel() < N):
        raise ValueError("out_scale (fp32 [N]) goes with col_scale and an fp16 c2 [2][M][ldc2]")
    if c is None and not c2_planes and not h2out:
        raise ValueError("gemm: C may be None only with c2_planes")
    if c2 is not None and ((c2.dtype != torch.bfloat16 and not h2out) or (c is not None and c.dtype != torch.float32)):
        raise ValueError("c2 is the bf16 copy of an fp32 C")
    if c2_planes and (c2 is None or c2.shape[0] != 3 or not c2.is_contiguous()):
        raise ValueError("c2_planes needs c2 = contiguous bf16 [3][M][ldc2]")
    if vt is not None and vt.dtype != c.dtype:
        raise ValueError("vt has the dtype of C")
    if w.dtype != compute:
        raise ValueError("W must already be in the compute dtype")
    for t in (a_mu, bias):
        if t is not None and t.dtype != torch.float32:
            raise ValueError("a_mu / bias must be float32")
    if r is not None and r.dtype != (c.dtype if c is not None else torch.float32):
        raise ValueError("residual dtype must equal the output dtype (fp32 for a c2_planes-only output)")
    args = GemmArgs()
    args.M, args.N, args.K = M, N, K
    args.nb1, args.nb2 = nb
    args.compute = BF16 if half2 else dt_code(compute)  # (mhada_gemm_half2 reads neither dtype)
    args.a_mode = a_mode
    args.a, args.a_dtype, args.lda = a.data_ptr(), BF16 if half2 else dt_code(a.dtype), lda
    args.sa1, args.sa2 = sa
    args.a_mu = _ptr(a_mu)
    args.smu1, args.smu2 = smu
    args.img_c, args.img_h, args.img_w = img
    args.w, args.ldw = w.data_ptr(), ldw
    args.sw1, args.sw2 = sw
    args.bias = _ptr(bias)
    args.sb1, args.sb2 = sb
    args.r = _ptr(r)
    args.r_dtype = dt_code(r.dtype) if r is not None else 0
    args.ldr = ldr
    args.sr1, args.sr2 = sr
    args.c, args.c_dtype, args.ldc = _ptr(c), dt_code(c.dtype) if c is not None else F32, ldc
    args.sc1, args.sc2 = sc
    args.relu = int(relu)
    args.pad = int(pad)
    args.c2, args.ldc2 = _ptr(c2), ldc2
    args.sc21, args.sc22 = sc2
    args.vt, args.ldt = _ptr(vt), ldt
    args.svt1, args.svt2 = svt
    args.c2_planes = int(c2_planes)
    if h2out:
        _call("mhada_gemm_half2_planes", a, ctypes.byref(args), col_scale.data_ptr(), out_scale.data_ptr())
    elif half2:
        _call("mhada_gemm_half2", a, ctypes.byref(args), col_scale.data_ptr())
    else:
        _call("mhada_gemm", a, ctypes.byref(args))
    return c if c is not None else c2


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out_dtype: torch.dtype,
           residual: Optional[torch.Tensor] = None, relu: bool = False,
           relu_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M][K] @ w[N][K]^T + bias (+relu) (+residual) -> [M][N] of out_dtype.  ``relu_mask``
    (fp32 [M][N], instead of a residual): the result is zeroed where relu_mask <= 0 (a ReLU
    adjoint folded into a gradient GEMM's epilogue, mhada_gemm relu = 2)."""
    M, K = x.shape
    N = w.shape[0]
    c = torch.empty(M, N, device=x.device, dtype=out_dtype)
    if relu_mask is not None:
        if residual is not None or relu or out_dtype != torch.float32 or relu_mask.dtype != torch.float32 \
                or relu_mask.shape != (M, N) or not relu_mask.is_contiguous():
            raise ValueError("linear: relu_mask needs fp32 output, a contiguous fp32 [M][N] mask, no residual / relu")
        return gemm(a=x, w=w, c=c, M=M, N=N, K=K, compute=w.dtype, lda=x.stride(0), ldw=w.stride(0),
                    bias=bias, r=relu_mask, ldr=N, ldc=N, relu=2)
    return gemm(a=x, w=w, c=c, M=M, N=N, K=K, compute=w.dtype, lda=x.stride(0), ldw=w.stride(0),
                bias=bias, r=residual, ldr=N if residual is not None else 0, ldc=N, relu=relu)


def patch_embed(img: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pos: Optional[torch.Tensor],
                patch: int = 8) -> torch.Tensor:
    """img (B,3,H,W) fp32 -> tokens [B][N][C] fp32 (+ pos [N][C] broadcast over B)."""
    if patch != 8:
        raise ValueError("the HIP patch embedding implements patch_size=8 (the reference default)")
    B, Ci, H, W = img.shape
    h, wd = H // 8, W // 8
    N, C = h * wd, w.shape[0]
    out = torch.empty(B, N, C, device=img.device, dtype=torch.float32)
    return gemm(a=img, w=w, c=out, M=N, N=C, K=Ci * 64, compute=w.dtype, a_mode=A_PATCH8,
                sa=(Ci * H * W, 0), nb=(B, 1), img=(Ci, H, W), ldw=w.stride(0), bias=bias,
                r=pos, ldr=C, sr=(0, 0), ldc=C, sc=(N * C, 0))


def patch_embed_dgrad(dy: torch.Tensor, w: torch.Tensor, H: int, W: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_patch_embed_dgrad``: the image gradient of the 8x8 / stride-8 patch embedding.  dy
    [B][(H//8)(W//8)][C] fp32 token rows, w the conv weight (C, Ci, 8, 8) or its [C][64 Ci] view ->
    (B, Ci, H, W) fp32.  The kernel writes every element (zeros in the H % 8 rows the forward
    ignores); ``out``: a contiguous fp32 (B, Ci, H, W) buffer to write into."""
    _need_gpu(dy, w, out)
    for t, what in ((dy, "dy"), (w, "w"), (out, "out")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"patch_embed_dgrad: {what} must be contiguous float32")
    if dy.dim() != 3 or w.dim() not in (2, 4) or w.shape[0] != dy.shape[2] or (w.dim() == 4 and w.shape[2:] != (8, 8)) \
            or (w.dim() == 2 and w.shape[1] % 64):
        raise ValueError(f"patch_embed_dgrad: dy [B][N][C] and w (C, Ci, 8, 8) or [C][64 Ci], got "
                         f"{tuple(dy.shape)} and {tuple(w.shape)}")
    B, N, C = dy.shape
    Ci = w.shape[1] if w.dim() == 4 else w.shape[1] // 64
    if H < 8 or W < 8 or N != (H // 8) * (W // 8):
        raise ValueError(f"patch_embed_dgrad: {N} token rows do not match a {H} x {W} image")
    if out is None:
        # H % 8 rows below the last patch: zeros (the kernel writes them too, for a caller's ``out``)
        out =(torch.zeros if H % 8 else torch.empty)(B, Ci, H, W, device=dy.device, dtype=torch.float32)
    elif out.shape != (B, Ci, H, W):
        raise ValueError(f"patch_embed_dgrad: out must be {(B, Ci, H, W)}, got {tuple(out.shape)}")
    _call("mhada_patch_embed_dgrad", dy, dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, C, Ci, H, W)
    return out


# fp32 3x3 convs run as Winograd F(2x2,3x3) (csrc/wino.hip) where the shape allows it; False
# forces the implicit-GEMM direct product (A/B measurements, tests).
WINO = True


def wino_eligible(x: torch.Tensor, w: torch.Tensor, upsample: bool) -> bool:
    """The Winograd kernel's constraints (csrc/wino.hip): fp32, Cin % 8, Cout % 64, >= 2x2 pixels
    and 32-bit element offsets (B*H*W*Cin and the output's B*H*W*Cout < 2^31); anything else runs
    on the implicit-GEMM conv."""
    return (WINO and w.dtype == torch.float32 and x.dtype == torch.float32 and not upsample
            and x.shape[-1] % 8 == 0 and w.shape[0] % 64 == 0 and x.shape[1] >= 2 and x.shape[2] >= 2
            and x.numel() < 2 ** 31 and x.numel() // x.shape[-1] * w.shape[0] < 2 ** 31)


# Winograd weight gradients for the eligible training convs (tests flip this to compare with the TN GEMM)
WINO_WGRAD = True


def wgrad_wino_eligible(x: torch.Tensor, g: torch.Tensor, cout: int) -> bool:
    """mhada_conv3x3_wgrad_wino's constraints: fp32 NHWC x [B][H][W][Cin] and g [B][H][W][ldg],
    Cin % 64 == 0, Cout % 64 == 0, H even, W % 16 == 0, 32-bit element offsets."""
    if not (WINO_WGRAD and x.is_cuda and x.dtype == torch.float32 and g.dtype == torch.float32):
        return False
    B, H, W, ci = x.shape
    return (ci % 64 == 0 and cout % 64 == 0 and H % 2 == 0 and W % 16 == 0 and g.shape[:3] == x.shape[:3]
            and g.shape[3] >= cout and g.shape[3] % 4 == 0 and x.is_contiguous() and g.is_contiguous()
            and B * H * W * max(ci, g.shape[3]) < 2 ** 31)


def conv3x3_wgrad_wino(x: torch.Tensor, g: torch.Tensor, cout: int, pad_mode: str = "reflect",
                       bias: bool = True):
    """``mhada_conv3x3_wgrad_wino``: the weight gradient [Cout][9*Cin] (k = tap*Cin + ci, the
    gemm_tn layout) and the bias gradient [Cout] (or None) of a pad-1 3x3 conv, from its input x
    and output gradient g (NHWC fp32)."""
    _need_gpu(x, g)
    B, H, W, ci = x.shape
    lib = _lib.load()
    S = lib.mhada_conv3x3_wgrad_wino_splits(B, H, W, ci, cout)
    if S <= 0:
        raise ValueError("conv3x3_wgrad_wino: ineligible shape")
    work = torch.empty(S * (16 * cout * ci + (cout if bias else 0)), device=x.device, dtype=torch.float32)
    dw = torch.empty(cout, 9 * ci, device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if bias else None
    _call("mhada_conv3x3_wgrad_wino", x, x.data_ptr(), g.data_ptr(), dw.data_ptr(),
          db.data_ptr() if bias else None, work.data_ptr(), work.numel(), B, H, W, ci, cout, g.shape[3],
          _lib.PAD_REFLECT if pad_mode == "reflect" else _lib.PAD_ZERO)
    return dw, db


def wino_weights_split3(w: torch.Tensor) -> torch.Tensor:
    """``mhada_wino_weights_split3``: w packed [Cout][9*Cin] fp32 (Cin % 16 == 0) -> the three
    round-to-nearest bf16 planes of U, [Cin/16][16][3][Cout][16] (p0 + p1 + p2 = the U of
    ``wino_weights``)."""
    _need_gpu(w)
    Co, K = w.shape
    Ci = K // 9
    if w.dtype != torch.float32 or K != 9 * Ci or Ci % 16 or not w.is_contiguous():
        raise ValueError("wino_weights_split3 needs a contiguous fp32 [Cout][9*Cin] weight, Cin % 16 == 0")
    up = torch.empty(Ci // 16, 16, 3, Co, 16, device=w.device, dtype=torch.bfloat16)
    _call("mhada_wino_weights_split3", w, w.data_ptr(), up.data_ptr(), Co, Ci)
    return up


def wino_weights(w: torch.Tensor) -> torch.Tensor:
    """``mhada_wino_weights``: w packed [Cout][9*Cin] fp32 -> U [Cin/8][16][Cout][8].  For
    Cin % 16 == 0 the result also carries the plane image of ``wino_weights_split3`` (attribute
    ``split3``), which ``conv3x3_wino`` hands to the SPLIT3 kernel."""
    _need_gpu(w)
    Co, K = w.shape
    Ci = K // 9
    if w.dtype != torch.float32 or K != 9 * Ci or not w.is_contiguous():
        raise ValueError("wino_weights needs a contiguous fp32 [Cout][9*Cin] weight")
    u = torch.empty(Ci // 8, 16, Co, 8, device=w.device, dtype=torch.float32)
    _call("mhada_wino_weights", w, w.data_ptr(), u.data_ptr(), Co, Ci)
    if Ci % 16 == 0:
        u.split3 = wino_weights_split3(w)
    return u


def conv3x3_wino(x: torch.Tensor, u: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True,
                 pad_mode: str = "reflect", pad: int = 1, out: Optional[torch.Tensor] = None,
                 relu_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_conv3x3_wino`` / ``mhada_conv3x3_wino_split3``: fp32 NHWC conv3x3 from the
    transformed filters ``u`` of ``wino_weights``; ``relu_mask`` (the output's layout): zero the
    outputs where relu_mask <= 0 (a folded ReLU adjoint)."""
    _need_gpu(x, u, bias, out, relu_mask)
    B, H, W, Ci = x.shape
    Co = u.shape[2]
    if x.dtype != torch.float32 or not x.is_contiguous() or u.shape[0] * 8 != Ci:
        raise ValueError("conv3x3_wino: contiguous fp32 NHWC input matching the filters")
    if pad_mode == "reflect":
        mode, Ho, Wo, pad = _lib.PAD_REFLECT, H, W, 1
    elif pad_mode == "zero":
        mode, Ho, Wo = _lib.PAD_ZERO, H + 2 * (pad - 1), W + 2 * (pad - 1)
    else:
        raise ValueError(f"pad_mode {pad_mode!r}")
    y = torch.empty(B, Ho, Wo, Co, device=x.device, dtype=torch.float32) if out is None else out
    if y.shape[:3] != (B, Ho, Wo) or y.dtype != torch.float32 or y.shape[-1] < Co or not y.is_contiguous():
        raise ValueError("conv3x3_wino: bad output buffer")
    if relu_mask is not None and (relu_mask.shape != y.shape or relu_mask.dtype != torch.float32
                                  or not relu_mask.is_contiguous()):
        raise ValueError("conv3x3_wino: relu_mask must be a contiguous fp32 tensor shaped like the output")
    up = getattr(u, "split3", None)
    if up is not None:  # the library takes the SPLIT3 kernel (tuning wino_split3) or falls back to u
        _call("mhada_conv3x3_wino_split3", x, x.data_ptr(), u.data_ptr(), up.data_ptr(), _ptr(bias), y.data_ptr(),
              B, H, W, Ci, Co, y.shape[-1], mode, pad, int(relu), _ptr(relu_mask))
    else:
        _call("mhada_conv3x3_wino", x, x.data_ptr(), u.data_ptr(), _ptr(bias), y.data_ptr(), B, H, W, Ci, Co,
              y.shape[-1], mode, pad, int(relu), _ptr(relu_mask))
    return y


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out_dtype: torch.dtype,
            upsample: bool, relu: bool = True, pad_mode: str = "reflect", pad: int = 1,
            out: Optional[torch.Tensor] = None, wino_u: Optional[torch.Tensor] = None,
            relu_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC x [B][H][W][Cin] -> NHWC [B][H'][W'][Cout]; ReflectionPad2d(1)+conv3x3(+ReLU),
    optionally on bilinear-x2(x), or (pad_mode "zero") a zero-padded conv with padding `pad`
    (1: same size, 2: the full correlation, H' = H + 2).  w packed [Cout][9*Cin] in the compute
    dtype.  ``out`` may be a preallocated [B][H'][W'][ldc >= Cout] buffer (channel padding).
    fp32 runs as Winograd F(2x2,3x3) when the shape allows (``wino_u``: cached transformed
    filters of ``w``).  ``relu_mask`` (fp32, shaped like the output): zero the outputs where
    relu_mask <= 0 — a ReLU adjoint folded into a dgrad (in the Winograd output stage; a separate
    mhada_relu_bwd pass on the implicit-GEMM path)."""
    B, H, W, Ci = x.shape
    Co = w.shape[0]
    if out_dtype == torch.float32 and wino_eligible(x, w, upsample) and x.is_contiguous():
        u = wino_u if wino_u is not None else wino_weights(w)
        return conv3x3_wino(x, u, bias, relu, pad_mode, pad, out, relu_mask)
    if relu_mask is not None:
        return relu_bwd(conv3x3(x, w, bias, out_dtype, upsample, relu, pad_mode, pad, out), relu_mask)
    if pad_mode == "zero":
        if upsample:
            raise ValueError("zero-padded conv3x3 has no fused upsample")
        Ho, Wo = H + 2 * (pad - 1), W + 2 * (pad - 1)
        mode = A_CONV3X3_ZERO
    elif pad_mode == "reflect":
        Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
        mode = A_CONV3X3_UP2 if upsample else A_CONV3X3
        pad = 0
    else:
        raise ValueError(f"pad_mode {pad_mode!r}")
    y = torch.empty(B, Ho, Wo, Co, device=x.device, dtype=out_dtype) if out is None else out
    return gemm(a=x, w=w, c=y, M=B * Ho * Wo, N=Co, K=9 * Ci, compute=w.dtype, a_mode=mode, img=(Ci, H, W),
                ldw=w.stride(0), bias=bias, ldc=y.shape[-1], relu=relu, pad=pad)


def upsample2x(x: torch.Tensor) -> torch.Tensor:
    """NHWC bilinear x2 (align_corners=False)."""
    _need_gpu(x)
    B, H, W, C = x.shape
    y = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=x.dtype)
    _call("mhada_upsample2x", x, x.data_ptr(), y.data_ptr(), dt_code(x.dtype), B, H, W, C)
    return y


def conv3x3_out3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, clamp255: bool = False) -> torch.Tensor:
    B, H, W, Ci = x.shape
    _need_gpu(x, w, bias)
    y = torch.empty(B, 3, H, W, device=x.device, dtype=torch.float32)
    _call("mhada_conv3x3_out3", x, x.data_ptr(), dt_code(x.dtype), w.data_ptr(), bias.data_ptr(),
                                        y.data_ptr(), B, H, W, Ci, int(clamp255))
    return y


def conv3x3_out3_u8(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, bgr: bool = True,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_conv3x3_out3_u8``: the last decoder layer writing the cv2-ready u8 frame [B][H][W][3]
    (B,G,R for ``bgr``, else R,G,B) — bit for bit ``frame_emit(conv3x3_out3(x, w, bias, clamp255=True))``
    with no fp32 frame in between.  ``out``: as in frame_emit."""
    B, H, W, Ci = x.shape
    _need_gpu(x, w, bias, out)
    out = _u8_frames(out, B, H, W, x.device)
    _call("mhada_conv3x3_out3_u8", x, x.data_ptr(), dt_code(x.dtype), w.data_ptr(), bias.data_ptr(),
          out.data_ptr(), out.stride(1), int(bgr), B, H, W, Ci)
    return out


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, out_dtype: torch.dtype, eps: float) -> torch.Tensor:
    _need_gpu(x, g, b)
    rows, cols = x.shape
    y = torch.empty(rows, cols, device=x.device, dtype=out_dtype)
    _call("mhada_layernorm", x, x.data_ptr(), y.data_ptr(), dt_code(out_dtype), g.data_ptr(), b.data_ptr(),
                                     rows, cols, eps)
    return y


# fp32 GEMMs whose A comes from a LayerNorm (the ViT's QKV and MLP1) run as SPLIT3 products on the
# bf16 MFMA (mhada_gemm a_mode MHADA_A_SPLIT3): fp32-accurate — against fp64 their error is below
# the fp32 MFMA path's (tools/split_bf16_probe.py) — and 1.4-1.5x faster.  False: the fp32 MFMA.
F32_SPLIT = True


# The fp32 forward's two 512 x 512 out-projections (the ViT's attention out_proj and the MHAda block's
# out_conv) as SPLIT3 GEMMs where their tiles fill the chip: the producing attention kernels write the
# bf16 planes themselves (vit_batch_attn_split3, attn_split3_planes) and no fp32 copy.  False: both stay
# on the fp32 MFMA GEMM, fed by fp32 attention outputs.
F32_SPLIT_OUTPROJ = True


def layernorm_split3(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    """``mhada_layernorm`` with y_dtype MHADA_BF16X3: the fp32 LayerNorm of x as three bf16 planes
    [3][rows][cols] (y = p0 + p1 + p2 to 2^-25 relative), the A operand of ``linear_split3``."""
    _need_gpu(x, g, b)
    rows, cols = x.shape
    y = torch.empty(3, rows, cols, device=x.device, dtype=torch.bfloat16)
    _call("mhada_layernorm", x, x.data_ptr(), y.data_ptr(), BF16X3, g.data_ptr(), b.data_ptr(), rows, cols, eps)
    return y


def split3_weight(w: torch.Tensor) -> torch.Tensor:
    """An fp32 weight [N][K0] (K0 % 64 == 0) as the SPLIT3 GEMM's W operand: its bf16 planes q0 + q1 +
    q2 (8 + 8 + 8 mantissa bits) interleaved per 64-column chunk kk as q1 | q0 | q2 | q0 | q1 | q0
    -> [N][6 K0] bf16, the GEMM's K-tile 6 kk + t (one-time weight preparation, cached with the
    module's other prepared weights)."""
    w = w.float()
    N, K0 = w.shape
    if K0 % 64:
        raise ValueError("split3_weight: K0 must be a multiple of 64")
    q0 = w.bfloat16()
    r = w - q0.float()
    q1 = r.bfloat16()
    q2 = (r - q1.float()).bfloat16()
    terms = torch.stack([t.view(N, K0 // 64, 64) for t in (q1, q0, q2, q0, q1, q0)], dim=2)
    return terms.reshape(N, 6 * K0).contiguous()


def split3_weight_dev(w: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """``mhada_split3_weight``: split3_weight(w) (or of w.t()) in one device launch, bit-identical to
    split3_weight — the training step re-splits its weights after every optimizer step."""
    _need_gpu(w)
    if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 2:
        raise ValueError("split3_weight_dev needs a contiguous float32 matrix")
    N, K0 = (w.shape[1], w.shape[0]) if transposed else w.shape
    if K0 % 64:
        raise ValueError("split3_weight_dev: K0 must be a multiple of 64")
    out = torch.empty(N, 6 * K0, device=w.device, dtype=torch.bfloat16)
    _call("mhada_split3_weight", w, w.data_ptr(), out.data_ptr(), N, K0, int(transposed))
    return out


def split3_rows(x: torch.Tensor) -> torch.Tensor:
    """``mhada_split3_rows``: a contiguous fp32 matrix [M][K0] as its three bf16 planes [3][M][K0] (the
    ``linear_split3`` A operand of an activation or gradient that no LayerNorm produced)."""
    _need_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("split3_rows needs a contiguous float32 [M][K0] matrix")
    y = torch.empty(3, *x.shape, device=x.device, dtype=torch.bfloat16)
    _call("mhada_split3_rows", x, x.data_ptr(), y.data_ptr(), x.numel())
    return y


def linear_split3(planes: torch.Tensor, w6: torch.Tensor, bias: Optional[torch.Tensor], out_dtype: torch.dtype,
                  residual: Optional[torch.Tensor] = None, relu: bool = False,
                  out_planes: bool = False, relu_mask: Optional[torch.Tensor] = None, both: bool = False):
    """fp32-accurate x @ w^T (+bias, relu, residual) from x's bf16 planes [3][M][K0] and
    ``split3_weight(w)`` [N][6 K0]: the six significant cross products summed in fp32 accumulators
    on the bf16 MFMA (mhada_gemm MHADA_A_SPLIT3).  ``out_planes``: return the fp32 result as its
    three bf16 planes [3][M][N] (the next SPLIT3 GEMM's operand) instead of an fp32 [M][N].
    ``relu_mask`` (fp32 [M][N], as ``linear``'s): the result zeroed where relu_mask <= 0.  ``both``: return
    (the fp32 result, its three bf16 planes) from the one epilogue — for a result that is kept in fp32
    (saved for a backward) and also feeds a SPLIT3 GEMM."""
    if planes.dim() != 3 or planes.shape[0] != 3 or planes.dtype != torch.bfloat16 or not planes.is_contiguous():
        raise ValueError("linear_split3: planes must be contiguous bf16 [3][M][K0]")
    _, M, K0 = planes.shape
    N = w6.shape[0]
    if w6.dtype != torch.bfloat16 or w6.shape[1] != 6 * K0:
        raise ValueError("linear_split3: w6 must be split3_weight(w), bf16 [N][6*K0]")
    if out_planes:
        if out_dtype != torch.float32:
            raise ValueError("linear_split3: out_planes splits an fp32 result")
        c2 = torch.empty(3, M, N, device=planes.device, dtype=torch.bfloat16)
        return gemm(a=planes, w=w6, c=None, M=M, N=N, K=6 * K0, compute=torch.bfloat16, a_mode=A_SPLIT3, lda=K0,
                    ldw=6 * K0, bias=bias, r=residual, ldr=N if residual is not None else 0, ldc=N, relu=relu,
                    c2=c2, ldc2=N, c2_planes=True)
    c = torch.empty(M, N, device=planes.device, dtype=out_dtype)
    c2 = None
    if both:
        if out_dtype != torch.float32:
            raise ValueError("linear_split3: both splits an fp32 result")
        c2 = torch.empty(3, M, N, device=planes.device, dtype=torch.bfloat16)
    if relu_mask is not None:
        if residual is not None or relu or out_dtype != torch.float32 or relu_mask.dtype != torch.float32 \
                or relu_mask.shape != (M, N) or not relu_mask.is_contiguous():
            raise ValueError("linear_split3: relu_mask needs fp32 output, a contiguous fp32 [M][N] mask, no residual / relu")
        gemm(a=planes, w=w6, c=c, M=M, N=N, K=6 * K0, compute=torch.bfloat16, a_mode=A_SPLIT3, lda=K0,
             ldw=6 * K0, bias=bias, r=relu_mask, ldr=N, ldc=N, relu=2, c2=c2, ldc2=N if both else 0, c2_planes=both)
    else:
        gemm(a=planes, w=w6, c=c, M=M, N=N, K=6 * K0, compute=torch.bfloat16, a_mode=A_SPLIT3, lda=K0,
             ldw=6 * K0, bias=bias, r=residual, ldr=N if residual is not None else 0, ldc=N, relu=relu,
             c2=c2, ldc2=N if both else 0, c2_planes=both)
    return (c, c2) if both else c


# The LayerNorm-fed fp32 GEMMs (the ViT's QKV and MLP1) as HALF2 products instead of SPLIT3: three fp16
# products of two-plane operands where SPLIT3 takes six bf16 products of three-plane operands.  fp16
# lacks range, so both operands are scaled by exact powers of two chosen from bounds that do not depend
# on the data: |LayerNorm(x)| <= sqrt(C) max|gamma| + max|beta|, and the weight rows are known.  False:
# SPLIT3, with the same kernels and launches as before this switch existed.
F32_HALF2 = True

_H2_MIN = 2.0 ** -14  # smallest normal fp16: the plane writers flush what is below
_H2_SCALE_WINDOW = (2.0 ** -40, 2.0 ** 40)


def _half2_planes(v: torch.Tensor):
    """fp32 v -> (hi, lo) fp16: hi = fp16_rn(v), lo = fp16_rn(v - hi), subnormal plane values flushed to zero."""
    hi = v.half()
    hi = torch.where(hi.abs() < _H2_MIN, torch.zeros_like(hi), hi)
    lo = (v - hi.float()).half()
    lo = torch.where(lo.abs() < _H2_MIN, torch.zeros_like(lo), lo)
    return hi, lo


def half2_a_scale(gamma: torch.Tensor, beta: torch.Tensor) -> Optional[float]:
    """s_a = 2^floor(log2(32768 / Y)) for a LayerNorm with these parameters, Y = sqrt(C) max|gamma| +
    max|beta| >= |y|; None where Y is zero or not finite or s_a leaves [2^-40, 2^40] (the layer keeps SPLIT3)."""
    Y = math.sqrt(gamma.numel()) * float(gamma.detach().abs().max()) + float(beta.detach().abs().max())
    if not math.isfinite(Y) or Y <= 0.0:
        return None
    q = 32768.0 / Y
    if not math.isfinite(q) or q <= 0.0:
        return None
    s_a = 2.0 ** (math.frexp(q)[1] - 1)
    return s_a if _H2_SCALE_WINDOW[0] <= s_a <= _H2_SCALE_WINDOW[1] else None


def half2_weight(w: torch.Tensor):
    """An fp32 weight [N][K0] (K0 % 64 == 0) as the HALF2 GEMM's W operand -> (w2, t): per row n the scale
    t_n = 2^(14 - floor(log2 max_k |w_nk|)) (1 for a zero or non-finite row, at most 2^127), the planes hi | lo of t_n w
    interleaved per 64-column chunk -> w2 fp16 [N][2 K0], and t fp32 [N]."""
    w = w.float()
    N, K0 = w.shape
    if K0 % 64:
        raise ValueError("half2_weight: K0 must be a multiple of 64")
    m = w.abs().amax(dim=1)
    ok = torch.isfinite(m) & (m > 0)
    e = torch.frexp(torch.where(ok, m, torch.ones_like(m)))[1]  # m = f 2^e, f in [0.5, 1)
    # 2^min(15 - e, 127) built from its bits (torch.ldexp goes through pow, inexact on the device)
    t = ((127 + torch.clamp(15 - e, max=127)).to(torch.int32) << 23).view(torch.float32)
    t = torch.where(ok, t, torch.ones_like(m))
    hi, lo = _half2_planes(w * t[:, None])
    w2 = torch.stack([p.view(N, K0 // 64, 64) for p in (hi, lo)], dim=2)
    return w2.reshape(N, 2 * K0).contiguous(), t


def half2_weight_dev(w: torch.Tensor):
    """``mhada_half2_weight``: half2_weight(w) in one device launch, bit-identical to it."""
    _need_gpu(w)
    if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 2 or w.shape[1] % 64:
        raise ValueError("half2_weight_dev needs a contiguous float32 [N][K0] matrix, K0 % 64 == 0")
    N, K0 = w.shape
    w2 = torch.empty(N, 2 * K0, device=w.device, dtype=torch.float16)
    t = torch.empty(N, device=w.device, dtype=torch.float32)
    _call("mhada_half2_weight", w, w.data_ptr(), w2.data_ptr(), t.data_ptr(), N, K0)
    return w2, t


def half2_prepare(gamma: torch.Tensor, beta: torch.Tensor, w: torch.Tensor) -> Optional[dict]:
    """The HALF2 form of one LayerNorm-fed linear layer, decided once at preparation time: dict(s_a, w2,
    cs) with cs[n] = 1 / (s_a t_n), or None — the layer keeps SPLIT3 — where Y is zero or not finite, a
    weight row is not finite, or a scale leaves [2^-40, 2^40]."""
    s_a = half2_a_scale(gamma, beta)
    if s_a is None or w.shape[1] % 64 or not bool(torch.isfinite(w).all()):
        return None
    w2, t = half2_weight_dev(w.float().contiguous()) if w.is_cuda else half2_weight(w)
    lo, hi = _H2_SCALE_WINDOW
    if float(t.min()) < lo or float(t.max()) > hi:
        return None
    return dict(s_a=s_a, w2=w2, cs=(1.0 / (s_a * t.double())).float().contiguous())


def layernorm_half2(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float, s_a: float) -> torch.Tensor:
    """``mhada_layernorm_half2``: the fp32 LayerNorm of x, times the power of two s_a, as two fp16 planes
    [2][rows][cols] (hi, lo), the A operand of ``linear_half2``."""
    _need_gpu(x, g, b)
    rows, cols = x.shape
    y = torch.empty(2, rows, cols, device=x.device, dtype=torch.float16)
    _call("mhada_layernorm_half2", x, x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr(), rows, cols, eps, s_a)
    return y


def linear_half2(planes: torch.Tensor, w2: torch.Tensor, cs: torch.Tensor, bias: Optional[torch.Tensor],
                 out_dtype: torch.dtype, residual: Optional[torch.Tensor] = None, relu: bool = False,
                 out_planes: bool = False, out_scale: Optional[torch.Tensor] = None):
    """fp32-accurate x @ w^T (+bias, relu, residual) from ``layernorm_half2`` planes [2][M][K0],
    ``half2_weight(w)`` [N][2 K0] and cs [N]: A_lo W_hi + A_hi W_hi + A_hi W_lo in fp32 accumulators on the
    fp16 MFMA, column n times cs[n] (mhada_gemm_half2).  ``out_planes``: the fp32 result as its three
    bf16 planes [3][M][N] (the next SPLIT3 GEMM's operand) instead of an fp32 [M][N]; with ``out_scale``
    (fp32 [N], ``half2_chain_prepare``'s u) as the two fp16 planes [2][M][N] of out_scale[n] times it, the
    A operand of ``linear_half2_planes`` (mhada_gemm_half2_planes)."""
    if planes.dim() != 3 or planes.shape[0] != 2 or planes.dtype != torch.float16 or not planes.is_contiguous():
        raise ValueError("linear_half2: planes must be contiguous fp16 [2][M][K0]")
    _, M, K0 = planes.shape
    N = w2.shape[0]
    if w2.dtype != torch.float16 or w2.shape[1] != 2 * K0 or not w2.is_contiguous():
        raise ValueError("linear_half2: w2 must be half2_weight(w), fp16 [N][2*K0]")
    kw = dict(a=planes, w=w2, M=M, N=N, K=K0, compute=torch.float16, lda=K0, ldw=2 * K0, bias=bias, r=residual,
              ldr=N if residual is not None else 0, ldc=N, relu=relu, col_scale=cs)
    if out_planes:
        if out_dtype != torch.float32:
            raise ValueError("linear_half2: out_planes splits an fp32 result")
        if out_scale is not None:
            c2 = torch.empty(2, M, N, device=planes.device, dtype=torch.float16)
            return gemm(c=None, c2=c2, ldc2=N, out_scale=out_scale, **kw)
        c2 = torch.empty(3, M, N, device=planes.device, dtype=torch.bfloat16)
        return gemm(c=None, c2=c2, ldc2=N, c2_planes=True, **kw)
    if out_scale is not None:
        raise ValueError("linear_half2: out_scale goes with out_planes")
    return gemm(c=torch.empty(M, N, device=planes.device, dtype=out_dtype), **kw)


# The HALF2 chain: the two fp32 ViT GEMMs whose A operand no LayerNorm writes but whose magnitude the
# layer's parameters still bound — MLP2 (A = relu(MLP1(LayerNorm x))) and the attention out-projection (A =
# the batch-axis attention output, a convex combination over the images of V = a slice of QKV(LayerNorm
# x)) — as HALF2 products too.  With y = LayerNorm(x) = gamma xhat + beta and sum xhat^2 <= C, column k of
# y W^T + b is bounded by Z_k = sqrt(C) ||gamma * w_k||_2 + |beta . w_k + b_k| (Cauchy-Schwarz); the ReLU
# and the convex combination keep the bound.  The producer writes fp16 planes of u_k v_k, u_k = 2^floor(
# log2(32768 / Z_k)), and the consumer's weight is prepared from w / u.  Takes effect only with F32_HALF2;
# False: MLP2 and the out-projection stay SPLIT3 with the launches made before this switch existed.
F32_HALF2_CHAIN = True
# The out-projection half of the chain has its own switch, and it is off by default: with it on, the ViT's
# out-projection no longer goes through linear_split3, and tests/test_gpu_proj_split3.py::
# test_engine_routes_both_out_projections_to_split3 counts exactly that at the default switches.  That test
# describes the routing before the chain; turning this on by default is a decision for whoever owns it
# (tests/test_gpu_half2_chain.py runs and checks the route with the switch on).  Takes effect only with
# F32_HALF2_CHAIN.
F32_HALF2_CHAIN_OUTPROJ = False


def half2_chain_bound(gamma: torch.Tensor, beta: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]):
    """Z [N] in fp64: Z_k = sqrt(C) ||gamma * w[k]||_2 + |beta . w[k] + b[k]| >= |LayerNorm(x) . w[k] + b[k]|
    for every x, for a LayerNorm over C columns with these parameters."""
    g, be, W = gamma.detach().double(), beta.detach().double(), w.detach().double()
    off = W @ be
    if b is not None:
        off = off + b.detach().double()
    return math.sqrt(g.numel()) * (W * g[None, :]).norm(dim=1) + off.abs()


def half2_out_scale(Z: torch.Tensor) -> Optional[torch.Tensor]:
    """u [N] fp32, u_k = 2^floor(log2(32768 / Z_k)) (so u_k Z_k <= 32768, a factor two below the fp16 maximum);
    None where a Z is zero or not finite or a u leaves [2^-40, 2^40]."""
    Z = Z.detach().double()
    if not bool((torch.isfinite(Z) & (Z > 0)).all()):
        return None
    q = 32768.0 / Z
    if not bool((torch.isfinite(q) & (q > 0)).all()):
        return None
    e = torch.frexp(q)[1] - 1  # q = f 2^(e + 1), f in [0.5, 1)
    if int(e.min()) < -40 or int(e.max()) > 40:
        return None
    return ((127 + e).to(torch.int32) << 23).view(torch.float32)  # 2^e built from its bits: exact


def half2_chain_prepare(gamma: torch.Tensor, beta: torch.Tensor, w_p: torch.Tensor, b_p: Optional[torch.Tensor],
                        w_c: torch.Tensor) -> Optional[dict]:
    """The HALF2 form of a linear layer w_c [N][K0] whose input column k is bounded by the producer
    LayerNorm(gamma, beta) -> w_p [K0][C], b_p (half2_chain_bound; a ReLU or a convex combination of such
    rows may sit between), decided once at preparation time: dict(u, w2, cs) — u fp32 [K0] the producer's
    per-column output scale, w2 = half2_weight(w_c / u) (exact: u are powers of two), cs[n] = 1 / t_n — or
    None (the layer keeps SPLIT3) where a parameter or a bound is zero or not finite, or a u, a t or a row's
    largest |w_c / u| leaves [2^-40, 2^40]."""
    ts = [t for t in (gamma, beta, w_p, b_p, w_c) if t is not None]
    if w_c.shape[1] % 64 or w_c.shape[1] != w_p.shape[0] or not all(bool(torch.isfinite(t).all()) for t in ts):
        return None
    u = half2_out_scale(half2_chain_bound(gamma, beta, w_p, b_p))
    if u is None:
        return None
    lo, hi = _H2_SCALE_WINDOW
    wu = (w_c.detach().float() / u.to(w_c.device)[None, :]).contiguous()
    m = wu.abs().amax(dim=1)
    if not bool(torch.isfinite(m).all()) or float(m.min()) < lo or float(m.max()) > hi:
        return None
    w2, t = half2_weight_dev(wu) if wu.is_cuda else half2_weight(wu)
    if float(t.min()) < lo or float(t.max()) > hi:
        return None
    return dict(u=u.to(w_c.device).contiguous(), w2=w2, cs=(1.0 / t.double()).float().contiguous())


def linear_half2_planes(planes: torch.Tensor, w2: torch.Tensor, cs: torch.Tensor, bias: Optional[torch.Tensor],
                        residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The consumer of the HALF2 chain: fp32-accurate x @ w^T (+bias, residual) -> fp32 [M][N] from the fp16
    planes [2][M][K0] of u x that ``linear_half2(out_scale=u)`` or ``vit_batch_attn_half2`` wrote and
    ``half2_chain_prepare``'s w2, cs (mhada_gemm_half2)."""
    if planes.dim() != 3 or planes.shape[0] != 2 or planes.dtype != torch.float16 or not planes.is_contiguous():
        raise ValueError("linear_half2_planes: planes must be contiguous fp16 [2][M][K0]")
    _, M, K0 = planes.shape
    N = w2.shape[0]
    if w2.dtype != torch.float16 or w2.shape[1] != 2 * K0 or not w2.is_contiguous():
        raise ValueError("linear_half2_planes: w2 must be half2_weight(w / u), fp16 [N][2*K0]")
    return gemm(a=planes, w=w2, c=torch.empty(M, N, device=planes.device, dtype=torch.float32), M=M, N=N, K=K0,
                compute=torch.float16, lda=K0, ldw=2 * K0, bias=bias, r=residual,
                ldr=N if residual is not None else 0, ldc=N, col_scale=cs)


def vit_batch_attn(qkv: torch.Tensor, L: int, ntok: int, heads: int, groups: int = 1) -> torch.Tensor:
    """``mhada_vit_batch_attn`` on qkv [L][ntok][3C]; ``groups`` > 1: the L images are that many
    independent calls of L / groups images each (consecutive slices), attended separately."""
    _need_gpu(qkv)
    C = qkv.shape[-1] // 3
    if L % groups:
        raise ValueError("vit_batch_attn: L must be a multiple of groups")
    out = torch.empty(L, ntok, C, device=qkv.device, dtype=qkv.dtype)
    Lg, es = L // groups, qkv.element_size()
    for g in range(groups):
        _call("mhada_vit_batch_attn", qkv, qkv.data_ptr() + g * Lg * ntok * 3 * C * es,
              out.data_ptr() + g * Lg * ntok * C * es, dt_code(qkv.dtype), Lg, ntok, heads, C // heads)
    return out


VIT_ATTN_SPLIT3_MAX_L = 8  # mhada_vit_batch_attn_split3 refuses longer batch axes (and head widths != 64)


def _one_per_group(what: str, L: int, groups: int) -> None:
    if groups < 1 or L % groups:
        raise ValueError(f"{what}: L must be a positive multiple of groups")
    if L != groups:
        raise ValueError(f"{what}: only L / groups == 1 (one image per group) is built; "
                         "vit_batch_attn(groups=) loops over any grouping")


def _vit_batch_attn(what: str, planes: int, qkv, L: int, ntok: int, heads: int, out_scale=None, groups=None):
    """The one-launch forms of ``vit_batch_attn`` (entry point "mhada_" + what) on qkv [L][ntok][3C].  ``planes``
    0: the output [L][ntok][C] in qkv's dtype; 3: fp32 qkv, the output as its three bf16 planes
    [3][L * ntok][C]; 2: fp32 qkv, out_scale[c] times the output as two fp16 planes [2][L * ntok][C].
    ``groups``: the grouped entries (the L images as that many independent calls; one image per group)."""
    _need_gpu(qkv, out_scale)
    if groups is not None:
        _one_per_group(what, L, groups)
    C = qkv.shape[-1] // 3
    if (planes and qkv.dtype != torch.float32) or not qkv.is_contiguous():
        raise ValueError(f"{what} needs contiguous {'float32 ' if planes else ''}qkv")
    if planes == 2 and (out_scale.dtype != torch.float32 or out_scale.numel() != C or not out_scale.is_contiguous()):
        raise ValueError(f"{what}: out_scale must be contiguous float32 [C]")
    if planes:
        out = torch.empty(planes, L * ntok, C, device=qkv.device,
                          dtype=torch.bfloat16 if planes == 3 else torch.float16)
        form = (L * ntok * C,) + ((out_scale.data_ptr(),) if planes == 2 else ())
    else:
        out = torch.empty(L, ntok, C, device=qkv.device, dtype=qkv.dtype)
        form = (dt_code(qkv.dtype),)
    _call("mhada_" + what, qkv, qkv.data_ptr(), out.data_ptr(), *form, L, ntok, heads, C // heads,
          *(() if groups is None else (groups,)))
    return out


def vit_batch_attn_split3(qkv: torch.Tensor, L: int, ntok: int, heads: int) -> torch.Tensor:
    """``mhada_vit_batch_attn_split3``: ``vit_batch_attn`` of fp32 qkv [L][ntok][3C] with the result as its three
    bf16 planes [3][L * ntok][C] (bit-identical to ``split3_rows`` of the fp32 output), the A operand of
    ``linear_split3``.  head_dim 64 and L <= 8; other shapes raise."""
    return _vit_batch_attn("vit_batch_attn_split3", 3, qkv, L, ntok, heads)


def vit_batch_attn_half2(qkv: torch.Tensor, L: int, ntok: int, heads: int, out_scale: torch.Tensor) -> torch.Tensor:
    """``mhada_vit_batch_attn_half2``: ``vit_batch_attn`` of fp32 qkv [L][ntok][3C] with out_scale[c] times the
    result as two fp16 planes [2][L * ntok][C] (bit-identical to ``_half2_planes`` of that product), the A
    operand of ``linear_half2_planes``.  head_dim 64 and L <= 8; other shapes raise."""
    return _vit_batch_attn("vit_batch_attn_half2", 2, qkv, L, ntok, heads, out_scale)


def vit_batch_attn_grouped(qkv: torch.Tensor, L: int, ntok: int, heads: int, groups: int) -> torch.Tensor:
    """``mhada_vit_batch_attn_grouped``: ``vit_batch_attn`` with the L images of qkv [L][ntok][3C] taken as
    ``groups`` independent calls, in ONE launch (the group comes from the grid); bit-identical to
    ``vit_batch_attn`` on each group's slice.  Built for L / groups == 1 (the clip route): the output is V."""
    return _vit_batch_attn("vit_batch_attn_grouped", 0, qkv, L, ntok, heads, groups=groups)


def vit_batch_attn_split3_grouped(qkv: torch.Tensor, L: int, ntok: int, heads: int, groups: int) -> torch.Tensor:
    """``mhada_vit_batch_attn_split3_grouped``: the grouped form of ``vit_batch_attn_split3`` (planes
    [3][L * ntok][C]); L / groups == 1, head_dim 64."""
    return _vit_batch_attn("vit_batch_attn_split3_grouped", 3, qkv, L, ntok, heads, groups=groups)


def vit_batch_attn_half2_grouped(qkv: torch.Tensor, L: int, ntok: int, heads: int, out_scale: torch.Tensor,
                                 groups: int) -> torch.Tensor:
    """``mhada_vit_batch_attn_half2_grouped``: the grouped form of ``vit_batch_attn_half2`` (fp16 planes
    [2][L * ntok][C]); L / groups == 1, head_dim 64."""
    return _vit_batch_attn("vit_batch_attn_half2_grouped", 2, qkv, L, ntok, heads, out_scale, groups)


def pos_embed(pos: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    _need_gpu(pos)
    _, C, bh, bw = pos.shape
    out = torch.empty(oh * ow, C, device=pos.device, dtype=torch.float32)
    _call("mhada_pos_embed", pos, pos.data_ptr(), out.data_ptr(), C, bh, bw, oh, ow)
    return out


def pos_embed_bwd(g: torch.Tensor, bh: int, bw: int) -> torch.Tensor:
    """``mhada_pos_embed_bwd``: token-major gradient g [oh][ow][C] -> (1, C, bh, bw)."""
    _need_gpu(g)
    oh, ow, C = g.shape
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("pos_embed_bwd needs a contiguous float32 [oh][ow][C] gradient")
    out = torch.empty(1, C, bh, bw, device=g.device, dtype=torch.float32)
    _call("mhada_pos_embed_bwd", g, g.data_ptr(), out.data_ptr(), C, bh, bw, oh, ow)
    return out


def instnorm_bwd(dy: torch.Tensor, y: torch.Tensor, rs: torch.Tensor) -> torch.Tensor:
    """``mhada_instnorm_bwd``: token rows dy, y [B][N][C], rstd [B][C] -> dx."""
    _need_gpu(dy, y, rs)
    for t in (dy, y, rs):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("instnorm_bwd needs contiguous float32 operands")
    B, N, C = y.shape
    if dy.shape != y.shape or rs.shape != (B, C):
        raise ValueError("instnorm_bwd: shape mismatch")
    splits = max(1, min(N // 32, 2048 // max(1, B * ((C + 63) // 64))))
    work = torch.empty(splits * B * C * 2 + B * C, device=y.device, dtype=torch.float64)
    dx = torch.empty_like(y)
    _call("mhada_instnorm_bwd", y, dy.data_ptr(), y.data_ptr(), rs.data_ptr(), dx.data_ptr(), work.data_ptr(), B, N, C,
          splits)
    return dx


def attn_train_bwd_prep(dout: torch.Tensor, x: torch.Tensor, mo: torch.Tensor):
    """``mhada_attn_train_bwd_prep``: (dx, dmo, dd) of the MHAda core's elementwise head."""
    _rows64(dout, x, mo)
    BH, Nc, _ = x.shape
    if dout.shape != x.shape or mo.shape != (BH, Nc, 128):
        raise ValueError("attn_train_bwd_prep: bad shapes")
    dx = torch.empty_like(x)
    dmo = torch.empty_like(mo)
    dd = torch.empty(BH, Nc, device=x.device, dtype=torch.float32)
    _call("mhada_attn_train_bwd_prep", x, dout.data_ptr(), x.data_ptr(), mo.data_ptr(), dx.data_ptr(), dmo.data_ptr(),
          dd.data_ptr(), BH * Nc)
    return dx, dmo, dd


def attn_train_bwd_prep_hd(dout: torch.Tensor, x: torch.Tensor, mo: torch.Tensor):
    """``mhada_attn_train_bwd_prep_hd``: ``attn_train_bwd_prep`` with rows of D = 32 | 128 channels."""
    _rows64(dout, x, mo)
    D = _train_hd_width("attn_train_bwd_prep_hd", x)
    BH, Nc, _ = x.shape
    if dout.shape != x.shape or mo.shape != (BH, Nc, 2 * D):
        raise ValueError("attn_train_bwd_prep_hd: bad shapes")
    dx = torch.empty_like(x)
    dmo = torch.empty_like(mo)
    dd = torch.empty(BH, Nc, device=x.device, dtype=torch.float32)
    _call("mhada_attn_train_bwd_prep_hd", x, dout.data_ptr(), x.data_ptr(), mo.data_ptr(), dx.data_ptr(),
          dmo.data_ptr(), dd.data_ptr(), BH * Nc, D)
    return dx, dmo, dd


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, planes: bool = False):
    """``mhada_layernorm_fwd``: fp32 rows [M][C] -> (y fp32, stats [M][2]); ``planes``: also y's three bf16
    planes [3][M][C] (``mhada_layernorm_fwd_split3``) -> (y, stats, planes)."""
    _need_gpu(x, gamma, beta)
    for t in (x, gamma, beta):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("layernorm_fwd needs contiguous float32 operands")
    M, C = x.shape
    y = torch.empty_like(x)
    st = torch.empty(M, 2, device=x.device, dtype=torch.float32)
    if planes:
        pl = torch.empty(3, M, C, device=x.device, dtype=torch.bfloat16)
        _call("mhada_layernorm_fwd_split3", x, x.data_ptr(), y.data_ptr(), pl.data_ptr(), st.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), M, C, float(eps))
        return y, st, pl
    _call("mhada_layernorm_fwd", x, x.data_ptr(), y.data_ptr(), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
          M, C, float(eps))
    return y, st


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, st: torch.Tensor, gamma: torch.Tensor):
    """``mhada_layernorm_bwd``: -> (dx, dgamma, dbeta)."""
    _need_gpu(x, dy, st, gamma)
    for t in (x, dy, st, gamma):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("layernorm_bwd needs contiguous float32 operands")
    M, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    nw = ((M + 127) // 128 * 2 + 2) * C
    work = torch.empty(nw, device=x.device, dtype=torch.float32)
    _call("mhada_layernorm_bwd", x, x.data_ptr(), dy.data_ptr(), st.data_ptr(), gamma.data_ptr(), dx.data_ptr(),
          dg.data_ptr(), db.data_ptr(), work.data_ptr(), nw, M, C)
    return dx, dg, db


_ROUTE = (0, 0)


def routed(x: int) -> int:
    """x as the form-routing rules count it: x * mul / div inside ``route_as``, else x."""
    mul, div = _ROUTE
    return x * mul // div if div else x


@contextlib.contextmanager
def route_as(mul: int, div: int):
    """Within the block, every rule that chooses a kernel form from the rows or the batch of a call — here
    (``engine._split3_fills``, ``instnorm_stats``' splits) and in the library (``mhada_set_route``: the fp32
    GEMM's tile-fill rule, the attention's waves per block) — evaluates them times mul / div: a chunk of
    ``div`` frames then takes the forms a clip of ``mul`` frames takes (``VideoStylizer.stylize_clip``)."""
    global _ROUTE
    saved = _ROUTE
    _ROUTE = (mul, div)
    _lib.check(_lib.load().mhada_set_route(mul, div), "mhada_set_route")
    try:
        yield
    finally:
        _ROUTE = saved
        _lib.check(_lib.load().mhada_set_route(*saved), "mhada_set_route")


def instnorm_stats(x: torch.Tensor, eps: float = 1e-5):
    """x [B][N][C] fp32 -> (mu, rstd) [B][C] fp32."""
    _need_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 3:
        raise ValueError(f"instnorm_stats needs contiguous float32 token rows [B][N][C], got {x.dtype} "
                         f"{tuple(x.shape)}")
    B, N, C = x.shape
    splits = max(1, min(N // 32, 2048 // max(1, routed(B) * ((C + 63) // 64))))
    mu = torch.empty(B, C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(B, C, device=x.device, dtype=torch.float32)
    work = torch.empty(splits, B, C, 2, device=x.device, dtype=torch.float64)
    _call("mhada_instnorm_stats", x, x.data_ptr(), mu.data_ptr(), rstd.data_ptr(), work.data_ptr(), B, N, C,
                                          splits, eps)
    return mu, rstd


LOG2E = 1.4426950408889634


HD_WIDTHS = (32, 128)  # head widths of the *_hd entry points (csrc/attn_hd.hip); 64 has its own kernels


def _hd_width(what: str, D: int) -> None:
    if D not in HD_WIDTHS:
        raise ValueError(f"{what}: head width must be 32 or 128 (64 has its own entry point), got {D}")


def _fold_block(what: str, hd: bool, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype, kscale):
    """fold_block (``hd`` False: W* [H][64][64], no checks of its own) and fold_block_hd (W* [H][D][D], D = 32 |
    128, every operand checked); entry point "mhada_" + what, which at ``hd`` also takes D."""
    ts = (wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s)
    if hd:
        _need_gpu(*ts)
    B, C = rstd_c.shape
    H, D = wf.shape[0], wf.shape[1] if hd else 64
    if hd:
        _hd_width(what, D)
        for t, shape in ((wf, (H, D, D)), (wg, (H, D, D)), (wh, (H, D, D)), (bg, (H, D)), (bh, (H, D)),
                         (rstd_c, (B, H * D)), (mu_s, (B, H * D)), (rstd_s, (B, H * D))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{what}: needs contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype}")
        dt_code(dtype)
    dev = wf.device
    wq = torch.empty(B, H, D, D, device=dev, dtype=dtype)
    wkv = torch.empty(B, H, 2 * D, D, device=dev, dtype=dtype)
    bkv = torch.empty(H, 2 * D, device=dev, dtype=torch.float32)
    v_mu = torch.empty(B, C, device=dev, dtype=torch.float32)
    if not hd:  # fold_block has always checked the device after allocating
        _need_gpu(*ts)
    _call("mhada_" + what, wf, *(t.data_ptr() for t in ts), wq.data_ptr(), wkv.data_ptr(), bkv.data_ptr(),
          v_mu.data_ptr(), kscale, dt_code(dtype), B, H, *((D,) if hd else ()))
    return wq, wkv, bkv, v_mu


def _fold_block_shared(what: str, fold, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype, kscale):
    """``fold`` (fold_block | fold_block_hd) with one style's statistics [1][C] repeated for the B frames."""
    B, C = rstd_c.shape
    if mu_s.shape != (1, C) or rstd_s.shape != (1, C):
        raise ValueError(f"{what}: the style statistics must be [1][{C}], got {tuple(mu_s.shape)} / "
                         f"{tuple(rstd_s.shape)}")
    wq, wkv, bkv, v_mu = fold(wf, wg, wh, bg, bh, rstd_c, mu_s.expand(B, C).contiguous(),
                              rstd_s.expand(B, C).contiguous(), dtype, kscale)
    return wq, wkv[:1], bkv, v_mu[:1]


def fold_block(wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype: torch.dtype, kscale: float = LOG2E):
    """Per-call weight fold of one MHAda block (include/mhada_hip.h).  kscale = log2(e) puts K
    in the softmax attention's log2 units (mhada_attn's K contract); 1.0 for cosine."""
    return _fold_block("fold_block", False, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype, kscale)


def fold_block_shared(wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype: torch.dtype, kscale: float = LOG2E):
    """``fold_block`` for B content frames (rstd_c [B][C]) against ONE style (mu_s, rstd_s [1][C]): wq
    [B][H][64][64] per frame; wkv [1][H][128][64], bkv and v_mu [1][C] of the style.  The existing entry with
    the style statistics repeated (B x C floats): no kernel of its own, so the bits are fold_block's."""
    return _fold_block_shared("fold_block_shared", fold_block, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype,
                              kscale)


def fold_block_hd(wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype: torch.dtype, kscale: float = LOG2E):
    """``mhada_fold_block_hd``: fold_block for W* [H][D][D], D = 32 | 128."""
    return _fold_block("fold_block_hd", True, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype, kscale)


def fold_block_hd_shared(wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s, dtype: torch.dtype, kscale: float = LOG2E):
    """``fold_block_hd`` for B content frames (rstd_c [B][C]) against ONE style (mu_s, rstd_s [1][C]): wq
    [B][H][D][D] per frame; wkv [1][H][2D][D], bkv and v_mu [1][C] of the style.  As ``fold_block_shared``."""
    return _fold_block_shared("fold_block_hd_shared", fold_block_hd, wf, wg, wh, bg, bh, rstd_c, mu_s, rstd_s,
                              dtype, kscale)


def transpose_v(kv: torch.Tensor) -> torch.Tensor:
    _need_gpu(kv)
    B, H, Ns, _ = kv.shape
    ldt = (Ns + 63) // 64 * 64
    vt = torch.empty(B, H, 128, ldt, device=kv.device, dtype=kv.dtype)
    _call("mhada_transpose_v", kv, kv.data_ptr(), vt.data_ptr(), dt_code(kv.dtype), B, H, Ns)
    return vt


def cosine_prep(q: Optional[torch.Tensor], kv: Optional[torch.Tensor]) -> None:
    """L2-normalise Q rows and/or the K half of KV rows in place (either may be None)."""
    _need_gpu(q, kv)
    ref = q if q is not None else kv
    if q is not None and kv is not None and q.shape[:2] != kv.shape[:2]:
        raise ValueError(f"cosine_prep: q {tuple(q.shape)} and kv {tuple(kv.shape)} differ in batch or heads; "
                         "normalise them in two calls")
    B, H = ref.shape[0], ref.shape[1]
    Nc = q.shape[2] if q is not None else 0
    Ns = kv.shape[2] if kv is not None else 0
    _call("mhada_cosine_prep", ref, _ptr(q), _ptr(kv), dt_code(ref.dtype), B, H, Nc, Ns)


def cosine_moments(kv: torch.Tensor, vt: torch.Tensor) -> torch.Tensor:
    """``mhada_cosine_moments``: the style-side moments [B][H][65][132] fp32 of the linear cosine
    activation from the normalised K half of kv and the V'^T | V'^2^T image vt.  The keys are split
    so that about 512 workgroups run (fixed-order sum of the splits: deterministic)."""
    _need_gpu(kv, vt)
    B, H, Ns, _ = kv.shape
    if vt.shape != (B, H, 128, (Ns + 63) // 64 * 64) or vt.dtype != kv.dtype:
        raise ValueError(f"cosine_moments: vt {tuple(vt.shape)} does not match kv {tuple(kv.shape)}")
    splits = max(1, min((Ns + 63) // 64, -(-512 // (B * H))))
    mom = torch.empty(B, H, 65, 132, device=kv.device, dtype=torch.float32)
    work = torch.empty(splits, B * H * 65 * 132, device=kv.device, dtype=torch.float32) if splits > 1 else None
    _call("mhada_cosine_moments", kv, kv.data_ptr(), vt.data_ptr(), dt_code(kv.dtype), B, H, Ns, mom.data_ptr(),
          _ptr(work), splits)
    return mom


def _shared_style(what: str, q, fcs, fcs_mu, fcs_rstd, v_mu) -> None:
    B, H, Nc, D = q.shape
    C = H * 64
    if D != 64 or not q.is_contiguous() or fcs.shape != (B, Nc, C) or fcs_mu.shape != (B, C) \
            or fcs_rstd.shape != (B, C) or v_mu.shape != (1, C):
        raise ValueError(f"{what}: needs q [B][H][Nc][64], fcs [B][Nc][{C}], per-frame statistics [B][{C}] and "
                         f"one style's v_mu [1][{C}]; got q {tuple(q.shape)}, fcs {tuple(fcs.shape)}, "
                         f"v_mu {tuple(v_mu.shape)}")
    for t in (fcs, fcs_mu, fcs_rstd, v_mu):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: fcs, its statistics and v_mu must be contiguous float32")


def _cosine_attn(what: str, shared: bool, q, mom, fcs, fcs_mu, fcs_rstd, v_mu):
    _need_gpu(q, mom, fcs, fcs_mu, fcs_rstd, v_mu)
    if shared:
        _shared_style(what, q, fcs, fcs_mu, fcs_rstd, v_mu)
    B, H, Nc, _ = q.shape
    Bs = 1 if shared else B
    if mom.shape != (Bs, H, 65, 132) or mom.dtype != torch.float32 or (shared and not mom.is_contiguous()):
        raise ValueError(f"{what}: mom must be fp32 [{Bs}][{H}][65][132]{' of one style, contiguous' if shared else ''}"
                         f", got {tuple(mom.shape)} {mom.dtype}")
    out = torch.empty(B, Nc, H * 64, device=q.device, dtype=q.dtype)
    _call("mhada_" + what, q, q.data_ptr(), mom.data_ptr(), fcs.data_ptr(), fcs_mu.data_ptr(),
          fcs_rstd.data_ptr(), v_mu.data_ptr(), out.data_ptr(), dt_code(q.dtype), B, H, Nc)
    return out


def cosine_attn(q, mom, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_cosine_attn``: mhada_attn's output for the cosine activation from normalised q and
    the style moments of cosine_moments."""
    return _cosine_attn("cosine_attn", False, q, mom, fcs, fcs_mu, fcs_rstd, v_mu)


def cosine_attn_shared(q, mom, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_cosine_attn_shared``: ``cosine_attn`` of B frames (normalised q [B][H][Nc][64], fcs and statistics
    per frame) against ONE style (mom [1][H][65][132] of cosine_moments, v_mu [1][C]); every frame gets the bits
    of ``cosine_attn`` with mom and v_mu repeated B times.  fp32 or bf16."""
    return _cosine_attn("cosine_attn_shared", True, q, mom, fcs, fcs_mu, fcs_rstd, v_mu)


def _mhada_attn(what: str, shared: bool, q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu, activation: int):
    """mhada_attn (no checks of its own; vt may be None) and mhada_attn_shared (one style's kv / vt, checked)."""
    _need_gpu(q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu)
    if shared:
        _shared_style(what, q, fcs, fcs_mu, fcs_rstd, v_mu)
    B, H, Nc, _ = q.shape
    Ns = kv.shape[2]
    ldt = (Ns + 63) // 64 * 64
    if shared and (kv.shape != (1, H, Ns, 128) or vt.shape != (1, H, 128, ldt) or kv.dtype != q.dtype
                   or vt.dtype != q.dtype or not kv.is_contiguous() or not vt.is_contiguous()):
        raise ValueError(f"{what}: kv / vt must be one style's contiguous [1][{H}][Ns][128] / "
                         f"[1][{H}][128][{ldt}] of q's dtype, got {tuple(kv.shape)} / {tuple(vt.shape)}")
    out = torch.empty(B, Nc, H * 64, device=q.device, dtype=q.dtype)
    _call(what, q, q.data_ptr(), kv.data_ptr(), _ptr(vt), fcs.data_ptr(), fcs_mu.data_ptr(), fcs_rstd.data_ptr(),
          v_mu.data_ptr(), out.data_ptr(), dt_code(q.dtype), B, H, Nc, Ns, activation)
    return out


def mhada_attn(q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu, activation: int) -> torch.Tensor:
    return _mhada_attn("mhada_attn", False, q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu, activation)


def mhada_attn_shared(q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_attn_shared``: the softmax ``mhada_attn`` of B frames (q [B][H][Nc][64], fcs and statistics
    per frame) against ONE style (kv [1][H][Ns][128], vt [1][H][128][ceil64(Ns)], v_mu [1][C]); every frame
    gets the bits of ``mhada_attn`` with the style operands repeated B times.  fp32 or bf16."""
    return _mhada_attn("mhada_attn_shared", True, q, kv, vt, fcs, fcs_mu, fcs_rstd, v_mu, _lib.ACT_SOFTMAX)


def cosine_prep_hd(q: Optional[torch.Tensor], kv: Optional[torch.Tensor]) -> None:
    """``mhada_cosine_prep_hd``: L2-normalise the rows of q [B][H][Nc][D] and / or the K half of
    kv [B][H][Ns][2D] in place (either may be None), D = 32 | 128."""
    _need_gpu(q, kv)
    if q is None and kv is None:
        raise ValueError("cosine_prep_hd: needs q or kv")
    ref = q if q is not None else kv
    D = q.shape[-1] if q is not None else kv.shape[-1] // 2
    _hd_width("cosine_prep_hd", D)
    for t, w in ((q, D), (kv, 2 * D)):
        if t is not None and (t.dim() != 4 or t.shape[-1] != w or t.dtype != ref.dtype or not t.is_contiguous()
                              or t.shape[:2] != ref.shape[:2]):
            raise ValueError(f"cosine_prep_hd: needs contiguous q [B][H][Nc][{D}] / kv [B][H][Ns][{2 * D}] of one "
                             f"dtype, got {tuple(t.shape)} {t.dtype}")
    B, H = ref.shape[0], ref.shape[1]
    Nc = q.shape[2] if q is not None else 0
    Ns = kv.shape[2] if kv is not None else 0
    if Nc == 0 and Ns == 0:
        return
    _call("mhada_cosine_prep_hd", ref, _ptr(q) if Nc else None, _ptr(kv) if Ns else None, dt_code(ref.dtype), B, H,
          D, Nc, Ns)


def _attn_hd(what: str, shared: bool, q, kv, fcs, fcs_mu, fcs_rstd, v_mu, activation: int):
    """attn_hd and attn_hd_shared (kv and v_mu with a leading batch of 1); entry point "mhada_" + what."""
    _need_gpu(q, kv, fcs, fcs_mu, fcs_rstd, v_mu)
    bs = "1" if shared else "B"
    if q.dim() != 4 or kv.dim() != 4:
        raise ValueError(f"{what}: needs q [B][H][Nc][D] and kv [{bs}][H][Ns][2D], got {tuple(q.shape)} / "
                         f"{tuple(kv.shape)}")
    B, H, Nc, D = q.shape
    Ns = kv.shape[2]
    _hd_width(what, D)
    C = H * D
    Bs = 1 if shared else B
    if kv.shape != (Bs, H, Ns, 2 * D) or kv.dtype != q.dtype or not q.is_contiguous() or not kv.is_contiguous():
        raise ValueError(f"{what}: needs contiguous q [B][H][Nc][{D}] and kv [{bs}][H][Ns][{2 * D}] of one dtype, got "
                         f"{tuple(q.shape)} {q.dtype} / {tuple(kv.shape)} {kv.dtype}")
    if Nc <= 0 or Ns <= 0:
        raise ValueError(f"{what}: needs Nc > 0 and Ns > 0, got {Nc} / {Ns}")
    for t, shape in ((fcs, (B, Nc, C)), (fcs_mu, (B, C)), (fcs_rstd, (B, C)), (v_mu, (Bs, C))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: needs contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype}")
    out = torch.empty(B, Nc, C, device=q.device, dtype=q.dtype)
    _call("mhada_" + what, q, q.data_ptr(), kv.data_ptr(), fcs.data_ptr(), fcs_mu.data_ptr(), fcs_rstd.data_ptr(),
          v_mu.data_ptr(), out.data_ptr(), dt_code(q.dtype), B, H, D, Nc, Ns, activation)
    return out


def attn_hd(q, kv, fcs, fcs_mu, fcs_rstd, v_mu, activation: int) -> torch.Tensor:
    """``mhada_attn_hd``: the fused MHAda attention at D = 32 | 128 from q [B][H][Nc][D] and kv
    [B][H][Ns][2D] (K | V'); out [B][Nc][D H] in q's dtype."""
    return _attn_hd("attn_hd", False, q, kv, fcs, fcs_mu, fcs_rstd, v_mu, activation)


def attn_hd_shared(q, kv, fcs, fcs_mu, fcs_rstd, v_mu, activation: int) -> torch.Tensor:
    """``mhada_attn_hd_shared``: ``attn_hd`` of B frames (q [B][H][Nc][D], fcs and statistics per frame) against
    ONE style (kv [1][H][Ns][2D], v_mu [1][C]); every frame gets the bits of ``attn_hd`` with kv and v_mu repeated
    B times.  D = 32 | 128, both activations, fp32 or bf16."""
    return _attn_hd("attn_hd_shared", True, q, kv, fcs, fcs_mu, fcs_rstd, v_mu, activation)


WIDE_WIDTH = 512  # the head width of mhada_attn_wide (csrc/attn_wide.hip): one head over all channels
# bf16 single-head softmax blocks run mhada_attn_wide (measured faster than the fp32 mhada_loss_attn route at
# this width, tools/attn_wide_ab.py).  False: bf16 blocks take the fp32 route as well.
BF16_WIDE_ATTN = True


def attn_wide(q, k, v, fcs, fcs_mu, fcs_rstd, v_mu, want_bf16: bool = False):
    """``mhada_attn_wide``: the fused single-head AdaAttN softmax attention at D = 512 on the bf16 MFMA from
    bf16 q [B][Nc][512] (log2 units), k [B][Ns][512] and v [B][Ns][512] (V', centred, no bias); fcs
    [B][Nc][512] and fcs_mu / fcs_rstd / v_mu [B][512] fp32.  Returns out [B][Nc][512] fp32, or with
    ``want_bf16`` the pair (out, its bf16 rounding)."""
    _need_gpu(q, k, v, fcs, fcs_mu, fcs_rstd, v_mu)
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError(f"attn_wide: needs q [B][Nc][{WIDE_WIDTH}], k and v [B][Ns][{WIDE_WIDTH}], got "
                         f"{tuple(q.shape)} / {tuple(k.shape)} / {tuple(v.shape)}")
    B, Nc, D = q.shape
    Ns = k.shape[1]
    if D != WIDE_WIDTH:
        raise ValueError(f"attn_wide: head width must be {WIDE_WIDTH}, got {D}")
    if k.shape != (B, Ns, D) or v.shape != (B, Ns, D):
        raise ValueError(f"attn_wide: needs k and v [B][Ns][{D}] matching q, got {tuple(q.shape)} / {tuple(k.shape)} / "
                         f"{tuple(v.shape)}")
    for t in (q, k, v):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError(f"attn_wide: q, k, v must be contiguous bfloat16, got {t.dtype}")
    if Nc <= 0 or Ns <= 0:
        raise ValueError(f"attn_wide: needs Nc > 0 and Ns > 0, got {Nc} / {Ns}")
    for t, shape in ((fcs, (B, Nc, D)), (fcs_mu, (B, D)), (fcs_rstd, (B, D)), (v_mu, (B, D))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"attn_wide: needs contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype}")
    out = torch.empty(B, Nc, D, device=q.device, dtype=torch.float32)
    out16 = torch.empty(B, Nc, D, device=q.device, dtype=torch.bfloat16) if want_bf16 else None
    _call("mhada_attn_wide", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), fcs.data_ptr(), fcs_mu.data_ptr(),
          fcs_rstd.data_ptr(), v_mu.data_ptr(), out.data_ptr(), _ptr(out16), BF16, B, Nc, Ns, D)
    return (out, out16) if want_bf16 else out


# The fp32 softmax MHAda attention as SPLIT3 products on the bf16 MFMA (mhada_attn_split3): fp32-accurate
# (against fp64 at or below the fp32 MFMA kernel's error) and faster.  False: the fp32 MFMA kernel.
F32_SPLIT_ATTN = True


def split3_kv(kv: torch.Tensor, vt: torch.Tensor) -> torch.Tensor:
    """``mhada_split3_kv``: the fp32 K half of kv [B][H][Ns][128] and the fp32 V'^T | V'^2^T image vt
    [B][H][128][ceil64(Ns)] as the bf16 plane image [B][H][576 ceil64(Ns)] of ``attn_split3``."""
    _need_gpu(kv, vt)
    B, H, Ns, _ = kv.shape
    ldt = (Ns + 63) // 64 * 64
    if kv.dtype != torch.float32 or vt.dtype != torch.float32 or vt.shape != (B, H, 128, ldt) \
            or kv.shape[3] != 128 or not kv.is_contiguous() or not vt.is_contiguous():
        raise ValueError(f"split3_kv: needs contiguous fp32 kv [B][H][Ns][128] and vt [B][H][128][{ldt}], "
                         f"got {tuple(kv.shape)} / {tuple(vt.shape)}")
    img = torch.empty(B, H, 576 * ldt, device=kv.device, dtype=torch.bfloat16)
    _call("mhada_split3_kv", kv, kv.data_ptr(), vt.data_ptr(), img.data_ptr(), B, H, Ns)
    return img


def kv_proj_split3(fs: torch.Tensor, mu_s: torch.Tensor, wkv: torch.Tensor, bkv: torch.Tensor) -> torch.Tensor:
    """``mhada_kv_proj_split3``: the MHAda block's K|V' projection of the fp32 style tokens fs [B][Ns][64H]
    (centred by mu_s [B][64H], folded fp32 weights wkv [B][H][128][64] and bias bkv [H][128] of
    ``fold_block``) written straight as the ``attn_split3`` plane image [B][H][576 ceil64(Ns)]."""
    _need_gpu(fs, mu_s, wkv, bkv)
    B, Ns, C = fs.shape
    H = C // 64
    for t in (fs, mu_s, wkv, bkv):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("kv_proj_split3 needs contiguous float32 operands")
    if C % 64 or mu_s.shape != (B, C) or wkv.shape != (B, H, 128, 64) or bkv.shape != (H, 128):
        raise ValueError(f"kv_proj_split3: bad shapes fs {tuple(fs.shape)} mu {tuple(mu_s.shape)} "
                         f"wkv {tuple(wkv.shape)} bkv {tuple(bkv.shape)}")
    ldt = (Ns + 63) // 64 * 64
    img = torch.empty(B, H, 576 * ldt, device=fs.device, dtype=torch.bfloat16)
    _call("mhada_kv_proj_split3", fs, fs.data_ptr(), mu_s.data_ptr(), wkv.data_ptr(), bkv.data_ptr(), img.data_ptr(),
          B, H, Ns)
    return img


def _attn_split3(what: str, shared: bool, planes: bool, q, img, Ns: int, fcs, fcs_mu, fcs_rstd, v_mu):
    """The four attn_split3* ops (entry point "mhada_" + what): the output as fp32 rows [B][Nc][64 H] or
    (``planes``) its three bf16 planes [3][B * Nc][64 H]; the style's plane image img at batch B or (``shared``,
    with the shared-style operand checks) at batch 1."""
    _need_gpu(q, img, fcs, fcs_mu, fcs_rstd, v_mu)
    if shared:
        _shared_style(what, q, fcs, fcs_mu, fcs_rstd, v_mu)
    B, H, Nc, _ = q.shape
    ldt = (Ns + 63) // 64 * 64
    if shared and (q.dtype != torch.float32 or img.dtype != torch.bfloat16 or img.shape != (1, H, 576 * ldt)
                   or not img.is_contiguous()):
        raise ValueError(f"{what}: q must be fp32 and img one style's bf16 [1][{H}][576*{ldt}], got "
                         f"{q.dtype} / {tuple(img.shape)}")
    if not shared and (q.dtype != torch.float32 or not q.is_contiguous() or img.dtype != torch.bfloat16
                       or img.shape != (B, H, 576 * ldt)):
        raise ValueError(f"{what}: q must be contiguous fp32 and img bf16 [B][H][576*{ldt}], got "
                         f"{q.dtype} / {tuple(img.shape)}")
    out = torch.empty(3, B * Nc, H * 64, device=q.device, dtype=torch.bfloat16) if planes else \
        torch.empty(B, Nc, H * 64, device=q.device, dtype=torch.float32)
    _call("mhada_" + what, q, q.data_ptr(), img.data_ptr(), fcs.data_ptr(), fcs_mu.data_ptr(),
          fcs_rstd.data_ptr(), v_mu.data_ptr(), out.data_ptr(), B, H, Nc, Ns)
    return out


def attn_split3(q, img, Ns: int, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_attn_split3``: mhada_attn's fp32 softmax output from fp32 q [B][H][Nc][64] and the
    ``split3_kv`` plane image of Ns keys."""
    return _attn_split3("attn_split3", False, False, q, img, Ns, fcs, fcs_mu, fcs_rstd, v_mu)


def attn_split3_planes(q, img, Ns: int, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_attn_split3_planes``: ``attn_split3``'s output as its three bf16 planes [3][B * Nc][64 H]
    (bit-identical to ``split3_rows`` of it), the A operand of the out_conv ``linear_split3``."""
    return _attn_split3("attn_split3_planes", False, True, q, img, Ns, fcs, fcs_mu, fcs_rstd, v_mu)


def attn_split3_shared(q, img, Ns: int, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_attn_split3_shared``: ``attn_split3`` of B frames against ONE style's plane image
    [1][H][576 ceil64(Ns)] and v_mu [1][C]; every frame gets ``attn_split3``'s bits."""
    return _attn_split3("attn_split3_shared", True, False, q, img, Ns, fcs, fcs_mu, fcs_rstd, v_mu)


def attn_split3_planes_shared(q, img, Ns: int, fcs, fcs_mu, fcs_rstd, v_mu) -> torch.Tensor:
    """``mhada_attn_split3_planes_shared``: ``attn_split3_planes`` of B frames against ONE style; planes
    [3][B * Nc][64 H]."""
    return _attn_split3("attn_split3_planes_shared", True, True, q, img, Ns, fcs, fcs_mu, fcs_rstd, v_mu)


def _rows64(*ts: torch.Tensor) -> None:
    _need_gpu(*ts)
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("training attention operands must be contiguous float32")


def _train_hd_width(what: str, t: torch.Tensor) -> int:
    D = t.shape[-1] if t.dim() == 3 else -1
    if D not in (32, 128):
        raise ValueError(f"{what}: rows of 32 or 128 floats (64: the op without _hd), got {tuple(t.shape)}")
    return D


def _train_shapes(what: str, D: Optional[int], q, k, v, *others, lax: str = ""):
    """The operand checks of every training-attention op -> (BH, Nc, Ns, D): contiguous fp32 device tensors, q (BH,
    Nc, D), k and v (BH, Ns, D) with Ns > 0, and ``others``, (tensor, kind) pairs in the op's argument order: kind
    "q" is shaped like q (x), "row" (BH, Nc) (lse, dd), "wide" (BH, Nc, 2D) ([M' | E2'] and its gradient).
    D None: 32 | 128, read from q (the _hd ops).  ``lax``: the 64-wide fp32 ops check what they always have and
    no more — "fwd" takes k of any rank and Ns = 0, "bwd" also leaves q's width unchecked."""
    _rows64(q, k, v, *(t for t, _ in others))
    if D is None:
        D = _train_hd_width(what, q)
    BH, Nc, d = q.shape if q.dim() == 3 else (0, 0, -1)
    Ns = k.shape[1] if k.dim() == 3 or (lax and q.dim() == 3) else -1
    want = {"q": tuple(q.shape), "row": (BH, Nc), "wide": (BH, Nc, 2 * D)}
    if q.dim() != 3 or (d != D and lax != "bwd") or k.shape != (BH, Ns, D) or v.shape != k.shape \
            or (Ns <= 0 and not lax) or any(tuple(t.shape) != want[kind] for t, kind in others):
        raise ValueError(f"{what}: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}, others "
                         + " ".join(str(tuple(t.shape)) for t, _ in others))
    return BH, Nc, Ns, D


def _train_fwd_out(q: torch.Tensor, D: int):
    """The forward's outputs: out' like q, [M' | E2'] (BH, Nc, 2D), lse2 (BH, Nc)."""
    BH, Nc, _ = q.shape
    return (torch.empty_like(q), torch.empty(BH, Nc, 2 * D, device=q.device, dtype=torch.float32),
            torch.empty(BH, Nc, device=q.device, dtype=torch.float32))


def attn_train_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, x: torch.Tensor):
    """``mhada_attn_train_fwd``: q, x (BH, Nc, 64); k, v (BH, Ns, 64) with v centred.
    Returns out' (BH, Nc, 64), [M' | E2'] (BH, Nc, 128), lse2 (BH, Nc)."""
    BH, Nc, Ns, _ = _train_shapes("attn_train_fwd", 64, q, k, v, (x, "q"), lax="fwd")
    out, mo, lse = _train_fwd_out(q, 64)
    if TRAIN_FWD_S3:
        # SPLIT3 products on the bf16 MFMA (csrc/attn_split3.hip) over a bf16 plane image of k, v
        # (workspace, freed after)
        img = torch.empty(BH, 576 * ((Ns + 63) // 64 * 64), device=q.device, dtype=torch.bfloat16)
        _call("mhada_attn_train_fwd_split3", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), img.data_ptr(), x.data_ptr(),
              out.data_ptr(), mo.data_ptr(), lse.data_ptr(), BH, Nc, Ns)
    elif TRAIN_FWD_VT:
        # the inference fp32 attention structure on a V'^T | V'^2^T image (workspace, freed after)
        vt = torch.empty(BH, 128, (Ns + 63) // 64 * 64, device=q.device, dtype=torch.float32)
        _call("mhada_attn_train_fwd_vt", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), vt.data_ptr(), x.data_ptr(),
              out.data_ptr(), mo.data_ptr(), lse.data_ptr(), BH, Nc, Ns)
    else:
        _call("mhada_attn_train_fwd", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), x.data_ptr(), out.data_ptr(),
              mo.data_ptr(), lse.data_ptr(), BH, Nc, Ns)
    return out, mo, lse


# attn_train_fwd: TRAIN_FWD_S3 = mhada_attn_train_fwd_split3 (round 6, the default): S on the fp32
# MFMA, P V' / P V'^2 as SPLIT3 products on the bf16 MFMA with per-group sums added in fp32
# (csrc/attn_split3.hip) — 450 -> 433 ms per 512^2 B8 training step; the 64^2 video-training golden's
# gradient norms within 3.3e-4 (the fp32-MFMA forward: 4.9e-4;
# tools/video_golden_ab.py, profiles/r06_train_fwd_s3_acc_ab.log).  TRAIN_FWD_VT =
# mhada_attn_train_fwd_vt (the fp32-MFMA inference structure, round 4) when TRAIN_FWD_S3 is off;
# both off = the round-1 kernel (A/B, tests).
TRAIN_FWD_S3 = True
TRAIN_FWD_VT = True


# Largest dS spill (BH * Nc * Ns fp32) the training backward takes (512^2 batch 8, the three
# AdaFormer calls batched: 12.9 GB, reused across the step's attention calls by the caching
# allocator); larger problems, or spill=False, recompute S and dA in the query-stationary dQ
# kernel instead.  The choice depends on the shapes and this budget only — never on the device's
# free memory — so a step's dQ bits are reproducible run to run (the two paths sum dQ in different
# fp32 orders).  A spill that does not fit raises the allocator's OOM instead of switching paths.
DS_SPILL_BYTES = 16 << 30
# Per-(b, h) slice bound of the kernel's 32-bit dS buffer offsets ((Nc + 32) * Ns, attn_train.hip)
DS_SPILL_MAX_ROWS = 0x7fff0000 // 4
# Which backward each attn_train_bwd call took ("spill" / "recompute"): tests and tools read it.
BWD_PATH_COUNTS = {"spill": 0, "recompute": 0}


def ds_spill_eligible(BH: int, Nc: int, Ns: int) -> bool:
    """The shape rule of attn_train_bwd's default path (see DS_SPILL_BYTES)."""
    return Ns % 4 == 0 and 4 * BH * Nc * Ns <= DS_SPILL_BYTES and (Nc + 32) * Ns <= DS_SPILL_MAX_ROWS


def transpose64(x: torch.Tensor) -> torch.Tensor:
    """``mhada_transpose64``: fp32 [BH][N][64] -> [BH][64][ceil64(N)] (columns >= N zero)."""
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 3 or x.shape[-1] != 64:
        raise ValueError("transpose64: fp32 [BH][N][64]")
    x = x.contiguous()
    BH, N, _ = x.shape
    ldt = (N + 63) // 64 * 64
    out = torch.empty(BH, 64, ldt, device=x.device, dtype=torch.float32)
    _call("mhada_transpose64", x, x.data_ptr(), out.data_ptr(), BH, N, ldt)
    return out


def attn_train_bwd(q, k, v, lse, dmo, dd, spill: Optional[bool] = None):
    """``mhada_attn_train_bwd``: returns dq (BH, Nc, 64), dk, dv (BH, Ns, 64).  With the dS spill
    (default when ``ds_spill_eligible``): ``mhada_attn_train_dkv`` writes dS and dQ = dS K runs as
    one batched GEMM (896 instead of 1280 FLOP per query-key-head pair)."""
    BH, Nc, Ns, _ = _train_shapes("attn_train_bwd", 64, q, k, v, (lse, "row"), (dmo, "wide"), (dd, "row"),
                                   lax="bwd")
    auto = spill is None
    if auto:
        spill = ds_spill_eligible(BH, Nc, Ns)
    ds = None
    if spill:
        try:
            ds = torch.empty(BH, Nc, Ns, device=q.device, dtype=torch.float32)
        except torch.cuda.OutOfMemoryError:
            # the shape rule chose the spill but the device has no room for dS (a smaller card or a
            # larger batch): the recompute backward needs no workspace (same gradients to fp32 order)
            if not auto:
                raise
            spill = False
    BWD_PATH_COUNTS["spill" if spill else "recompute"] += 1
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    if not spill:
        _call("mhada_attn_train_bwd", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
              dd.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), BH, Nc, Ns)
        return dq, dk, dv
    if Ns % 4:
        raise ValueError("attn_train_bwd: the dS spill needs Ns % 4 == 0")
    _call("mhada_attn_train_dkv", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
          dd.data_ptr(), dk.data_ptr(), dv.data_ptr(), ds.data_ptr(), BH, Nc, Ns)
    if TRAIN_DQ_S3 and Ns % 32 == 0:
        ldt = (Ns + 63) // 64 * 64
        gemm_n64_split3(ds, transpose64_split3(k), dq, BH, Nc, Ns, ldt)
    else:
        kt = transpose64(k)  # W[n = d][k = key] of the NT GEMM, rows padded to ceil64(Ns)
        ldt = kt.shape[-1]
        gemm(a=ds, w=kt, c=dq, M=Nc, N=64, K=Ns, compute=torch.float32, lda=Ns, sa=(Nc * Ns, 0), nb=(BH, 1),
             ldw=ldt, sw=(64 * ldt, 0), ldc=64, sc=(Nc * 64, 0))
    return dq, dk, dv


# Calls of the dQ-only backward (attn_train_dq / attn_train_dq_hd), counted apart from BWD_PATH_COUNTS.
DQ_ONLY_COUNTS = {"dq_only": 0}


def attn_train_dq(q, k, v, lse, dmo, dd):
    """``mhada_attn_train_dq``: the dq (BH, Nc, 64) of ``attn_train_bwd(..., spill=False)`` alone — the
    query-stationary recompute kernel, bit-identical to that call's dq; dk and dv are not computed
    (a feature inversion: the key / value side carries no gradient)."""
    BH, Nc, Ns, _ = _train_shapes("attn_train_dq", 64, q, k, v, (lse, "row"), (dmo, "wide"), (dd, "row"),
                                   lax="bwd")
    DQ_ONLY_COUNTS["dq_only"] += 1
    dq = torch.empty_like(q)
    _call("mhada_attn_train_dq", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
          dd.data_ptr(), dq.data_ptr(), BH, Nc, Ns)
    return dq


def attn_train_fwd_hd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, x: torch.Tensor):
    """``mhada_attn_train_fwd_hd``: ``attn_train_fwd`` at head width D = 32 | 128 (csrc/attn_train.hip):
    q, x (BH, Nc, D); k, v (BH, Ns, D) with v centred.  Returns out' (BH, Nc, D), [M' | E2'] (BH, Nc, 2D),
    lse2 (BH, Nc).  One fp32-MFMA kernel; the TRAIN_FWD_* knobs are 64-wide only."""
    BH, Nc, Ns, D = _train_shapes("attn_train_fwd_hd", None, q, k, v, (x, "q"))
    out, mo, lse = _train_fwd_out(q, D)
    _call("mhada_attn_train_fwd_hd", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), x.data_ptr(), out.data_ptr(),
          mo.data_ptr(), lse.data_ptr(), BH, D, Nc, Ns)
    return out, mo, lse


def attn_train_bwd_hd(q, k, v, lse, dmo, dd):
    """``mhada_attn_train_bwd_hd``: ``attn_train_bwd`` at head width D = 32 | 128: returns dq (BH, Nc, D),
    dk, dv (BH, Ns, D).  Always the recompute backward (no dS spill at these widths, no workspace);
    BWD_PATH_COUNTS counts the 64-wide paths only."""
    BH, Nc, Ns, D = _train_shapes("attn_train_bwd_hd", None, q, k, v, (lse, "row"), (dmo, "wide"), (dd, "row"))
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    _call("mhada_attn_train_bwd_hd", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
          dd.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), BH, D, Nc, Ns)
    return dq, dk, dv


def attn_train_dq_hd(q, k, v, lse, dmo, dd):
    """``mhada_attn_train_dq_hd``: ``attn_train_dq`` at head width D = 32 | 128 — the dq of
    ``attn_train_bwd_hd`` alone, bit-identical to it."""
    BH, Nc, Ns, D = _train_shapes("attn_train_dq_hd", None, q, k, v, (lse, "row"), (dmo, "wide"), (dd, "row"))
    DQ_ONLY_COUNTS["dq_only"] += 1
    dq = torch.empty_like(q)
    _call("mhada_attn_train_dq_hd", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), dmo.data_ptr(),
          dd.data_ptr(), dq.data_ptr(), BH, D, Nc, Ns)
    return dq


# Calls of the bf16 training attention (attn_train_fwd_bf16 / attn_train_bwd_bf16): tests and tools
# read it, as BWD_PATH_COUNTS for the fp32 paths (which these calls do not touch).
BF16_TRAIN_COUNTS = {"fwd": 0, "bwd": 0}


def _bf16_workspace(q: torch.Tensor, BH: int, Nc: int, Ns: int, backward: bool) -> torch.Tensor:
    n = _lib.load().mhada_attn_train_bf16_workspace(BH, Nc, Ns, int(backward))
    if n < 0:
        raise ValueError("attn_train_bf16: bad sizes")
    return torch.empty(max(n, 16), device=q.device, dtype=torch.uint8)


def attn_train_fwd_bf16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, x: torch.Tensor):
    """``mhada_attn_train_fwd_bf16``: ``attn_train_fwd`` with Q K^T, P V' and P V'^2 on the bf16 MFMA
    (csrc/attn_train_bf16.hip; fp32 accumulation and softmax): fp32 q, x (BH, Nc, 64); k, v (BH, Ns, 64)
    with v centred.  Returns fp32 out' (BH, Nc, 64), [M' | E2'] (BH, Nc, 128), lse2 (BH, Nc).  The bf16
    operand images live in a workspace freed after the call."""
    BH, Nc, Ns, _ = _train_shapes("attn_train_fwd_bf16", 64, q, k, v, (x, "q"))
    out, mo, lse = _train_fwd_out(q, 64)
    ws = _bf16_workspace(q, BH, Nc, Ns, False)
    BF16_TRAIN_COUNTS["fwd"] += 1
    _call("mhada_attn_train_fwd_bf16", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), x.data_ptr(), out.data_ptr(),
          mo.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), BH, Nc, Ns)
    return out, mo, lse


def attn_train_bwd_bf16_prepass(q, k, v, dmo, mo) -> torch.Tensor:
    """Phase 1 of ``mhada_attn_train_bwd_bf16``: the bf16 operand images and D_row = sum_c bf16(dmo) mo
    of the backward, written into a new workspace that ``attn_train_bwd_bf16_run`` consumes.  dmo is
    dead afterwards: a caller that drops it before the run keeps the peak memory lower
    (MHAdaAttnBf16Fn.backward)."""
    BH, Nc, Ns, _ = _train_shapes("attn_train_bwd_bf16", 64, q, k, v, (dmo, "wide"), (mo, "wide"))
    ws = _bf16_workspace(q, BH, Nc, Ns, True)
    _call("mhada_attn_train_bwd_bf16", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), None, dmo.data_ptr(),
          mo.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), BH, Nc, Ns, 1)
    return ws


def attn_train_bwd_bf16_run(q, k, v, lse, ws: torch.Tensor):
    """Phase 2 of ``mhada_attn_train_bwd_bf16``: the dQ and dK / dV' kernels on the workspace of
    ``attn_train_bwd_bf16_prepass`` (same q, k, v).  Returns fp32 dq (BH, Nc, 64), dk, dv (BH, Ns, 64)."""
    _need_gpu(ws)
    BH, Nc, Ns, _ = _train_shapes("attn_train_bwd_bf16", 64, q, k, v, (lse, "row"))
    if ws.dtype != torch.uint8:
        raise ValueError("attn_train_bwd_bf16: bad shapes (the workspace is uint8)")
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    BF16_TRAIN_COUNTS["bwd"] += 1
    _call("mhada_attn_train_bwd_bf16", q, q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr(), None, None,
          dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), ws.numel(), BH, Nc, Ns, 2)
    return dq, dk, dv


def attn_train_bwd_bf16(q, k, v, lse, dmo, mo):
    """``mhada_attn_train_bwd_bf16``: ``attn_train_bwd`` on the bf16 MFMA (the recompute form: a
    query-stationary dQ kernel and a key-stationary dK / dV' kernel, no dS spill, no SPLIT3 GEMM):
    fp32 operands of ``attn_train_bwd``'s shapes, returns fp32 dq (BH, Nc, 64), dk, dv (BH, Ns, 64).
    Where ``attn_train_bwd`` takes D_row (``attn_train_bwd_prep``'s dd) this takes the forward's
    ``mo`` (BH, Nc, 128): the library forms D_row = sum_c bf16(dmo) mo from the rounded dmo it
    multiplies with, so that dS = P (dA - D_row) cancels where the softmax is peaked.
    = ``attn_train_bwd_bf16_prepass`` + ``attn_train_bwd_bf16_run``."""
    _rows64(lse)
    return attn_train_bwd_bf16_run(q, k, v, lse, attn_train_bwd_bf16_prepass(q, k, v, dmo, mo))


# dQ = dS K of the dS-spill backward as SPLIT3 products on the bf16 MFMA (csrc/gemm_n64_split3.hip,
# round 6) where Ns % 32 == 0; False: the fp32-MFMA N <= 64 GEMM (gemm_n64_kernel)
TRAIN_DQ_S3 = True


def transpose64_split3(k: torch.Tensor) -> torch.Tensor:
    """``mhada_transpose64_split3``: fp32 [BH][N][64] -> the bf16 planes of its transpose [3][BH * 64][ldt]
    (ldt = ceil64(N), columns >= N zero) = ``split3_rows(transpose64(k))`` in one pass."""
    _need_gpu(k)
    if k.dtype != torch.float32 or k.dim() != 3 or k.shape[-1] != 64:
        raise ValueError("transpose64_split3: fp32 [BH][N][64]")
    k = k.contiguous()
    BH, N, _ = k.shape
    ldt = (N + 63) // 64 * 64
    out = torch.empty(3, BH * 64, ldt, device=k.device, dtype=torch.bfloat16)
    _call("mhada_transpose64_split3", k, k.data_ptr(), out.data_ptr(), BH, N, ldt)
    return out


def gemm_n64_split3(ds: torch.Tensor, kt_planes: torch.Tensor, dq: torch.Tensor, BH: int, Nc: int, Ns: int,
                    ldt: int):
    """``mhada_gemm_n64_split3``: dq [BH][Nc][64] = ds [BH][Nc][Ns] @ K where kt_planes = the three bf16
    planes [3][BH * 64][ldt] of K^T (``split3_rows(transpose64(k))``)."""
    if ds.dtype != torch.float32 or not ds.is_contiguous() or ds.shape != (BH, Nc, Ns):
        raise ValueError("gemm_n64_split3: ds must be contiguous float32 [BH][Nc][Ns]")
    if kt_planes.dtype != torch.bfloat16 or kt_planes.shape != (3, BH * 64, ldt) or not kt_planes.is_contiguous():
        raise ValueError("gemm_n64_split3: kt_planes must be contiguous bf16 [3][BH*64][ldt]")
    if dq.dtype != torch.float32 or not dq.is_contiguous() or dq.shape != (BH, Nc, 64):
        raise ValueError("gemm_n64_split3: dq must be contiguous float32 [BH][Nc][64]")
    _call("mhada_gemm_n64_split3", ds, ds.data_ptr(), kt_planes.data_ptr(), dq.data_ptr(), BH, Nc, Ns, Ns, Nc * Ns,
          ldt, 64 * ldt, BH * 64 * ldt, 64, Nc * 64)


# ---- video path: optical-flow warping (NCHW fp32) ---------------------------------------
_PADDING = {"zeros": 0, "border": 1}


def _padding_code(padding_mode: str) -> int:
    try:
        return _PADDING[padding_mode]
    except KeyError:
        raise ValueError(f"padding_mode {padding_mode!r}: the HIP warp implements 'zeros' and 'border'")


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32")
    return t.contiguous()


def warp(x: torch.Tensor, flow: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    """``mhada_warp``: x [B][C][H][W], flow [B][2][H][W] -> warped x (utilities.py:100-118)."""
    _need_gpu(x, flow)
    x, flow = _f32c(x, "x"), _f32c(flow, "flow")
    B, C, H, W = x.shape
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError(f"flow must be [B,2,H,W] = {[B, 2, H, W]}, got {list(flow.shape)}")
    y = torch.empty_like(x)
    _call("mhada_warp", x, x.data_ptr(), flow.data_ptr(), y.data_ptr(), B, C, H, W,
                                _padding_code(padding_mode))
    return y


def warp_bwd(gy: torch.Tensor, flow: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    """``mhada_warp_bwd``: the gradient of warp(x, flow) w.r.t. x for the output gradient gy."""
    _need_gpu(gy, flow)
    gy, flow = _f32c(gy, "gy"), _f32c(flow, "flow")
    B, C, H, W = gy.shape
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError(f"flow must be [B,2,H,W] = {[B, 2, H, W]}, got {list(flow.shape)}")
    gx = torch.zeros_like(gy)
    _call("mhada_warp_bwd", gy, gy.data_ptr(), flow.data_ptr(), gx.data_ptr(), B, C, H, W, _padding_code(padding_mode))
    return gx


def flow_warp_mask(flo01: torch.Tensor, flo10: torch.Tensor, padding_mode: str = "zeros",
                   threshold: float = 2) -> torch.Tensor:
    """``mhada_flow_warp_mask``: flo01, flo10 [2][H][W] -> mask [H][W] (utilities.py:121-151)."""
    _need_gpu(flo01, flo10)
    flo01, flo10 = _f32c(flo01, "flo01"), _f32c(flo10, "flo10")
    if flo01.dim() != 3 or flo01.shape[0] != 2 or flo01.shape != flo10.shape:
        raise ValueError("flows must both be [2,H,W]")
    H, W = flo01.shape[1:]
    mask = torch.empty(H, W, device=flo01.device, dtype=torch.float32)
    _call("mhada_flow_warp_mask", flo01, flo01.data_ptr(), flo10.data_ptr(), mask.data_ptr(), H, W,
                                          float(threshold), _padding_code(padding_mode))
    return mask


def warp_l1(cs1: torch.Tensor, cs2: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """``mhada_warp_l1``: per-image sum(mask * |cs2 - warp(cs1, flow)|) / (C*H*W)."""
    _need_gpu(cs1, cs2, flow, mask)
    cs1, cs2, flow, mask = (_f32c(t, n) for t, n in ((cs1, "cs1"), (cs2, "cs2"), (flow, "flow"), (mask, "mask")))
    B, C, H, W = cs1.shape
    if cs2.shape != cs1.shape or tuple(flow.shape) != (B, 2, H, W) or tuple(mask.shape) != (B, H, W):
        raise ValueError("warp_l1: cs1/cs2 [B,C,H,W], flow [B,2,H,W], mask [B,H,W]")
    work = torch.empty(B * ((H * W + 255) // 256), device=cs1.device, dtype=torch.float64)
    out = torch.empty(B, device=cs1.device, dtype=torch.float32)
    _call("mhada_warp_l1", cs1, cs1.data_ptr(), cs2.data_ptr(), flow.data_ptr(), mask.data_ptr(),
                                   work.data_ptr(), out.data_ptr(), B, C, H, W)
    return out


# ---- video path: the temporal losses of train_video.py (csrc/temporal.hip) ------------------
TEMPORAL_WORK_WORDS = 1 + 2 * 2048  # MHADA_TEMPORAL_WORK_WORDS


def _strides4(t: torch.Tensor):
    """The element strides {b, c, y, x} of a 4-d tensor as the host array the temporal entries read."""
    return (ctypes.c_longlong * 4)(*t.stride())


def _temporal_args(x1, x2, flow, m, c1, c2, what):
    _need_gpu(x1, x2, flow, m)
    if x1.dim() != 4 or x1.shape != x2.shape or x1.dtype != torch.float32 or x2.dtype != torch.float32:
        raise ValueError(f"{what}: x1 / x2 must be float32 [B,C,H,W] of one shape")
    B, C, H, W = x1.shape
    flow, m = _f32c(flow, "flow"), _f32c(m, "mask")
    if tuple(flow.shape) != (B, 2, H, W) or tuple(m.shape) != (B, H, W):
        raise ValueError(f"{what}: flow [B,2,H,W] and mask [B,H,W] must match x1 {list(x1.shape)}")
    if (c1 is None) != (c2 is None):
        raise ValueError(f"{what}: c1 and c2 go together")
    if c1 is not None:
        _need_gpu(c1, c2)
        c1, c2 = _f32c(c1, "c1"), _f32c(c2, "c2")
        if tuple(c1.shape) != (B, 3, H, W) or c2.shape != c1.shape:
            raise ValueError(f"{what}: c1 / c2 must be [B,3,H,W] = {[B, 3, H, W]}")
    if any(s < 0 for s in x1.stride() + x2.stride()):
        raise ValueError(f"{what}: negative strides")
    return flow, m, c1, c2


def temporal_loss_fwd(x1: torch.Tensor, x2: torch.Tensor, flow: torch.Tensor, m: torch.Tensor,
                      c1: Optional[torch.Tensor] = None, c2: Optional[torch.Tensor] = None):
    """``mhada_temporal_loss_fwd``: sum(m (x2 - warp(x1, flow) - t)^2) / (C #{m != 0}) as a 0-d device
    tensor, with no host synchronisation; t = the luminance of c2 - warp(c1, flow) when c1 / c2 are
    given (lossfn.py:50-66), else 0 (lossfn.py:81-86).  x1 / x2 [B,C,H,W] in any strided layout
    (contiguous NCHW or channels_last: no copy).  Returns (loss, work); ``work`` (int64, word 0 the
    count of m != 0) is what ``temporal_loss_bwd`` takes."""
    flow, m, c1, c2 = _temporal_args(x1, x2, flow, m, c1, c2, "temporal_loss_fwd")
    B, C, H, W = x1.shape
    work = torch.empty(TEMPORAL_WORK_WORDS, device=x1.device, dtype=torch.int64)
    out = torch.empty((), device=x1.device, dtype=torch.float32)
    _call("mhada_temporal_loss_fwd", x1, x1.data_ptr(), _strides4(x1), x2.data_ptr(), _strides4(x2), flow.data_ptr(),
          m.data_ptr(), None if c1 is None else c1.data_ptr(), None if c2 is None else c2.data_ptr(),
          work.data_ptr(), out.data_ptr(), B, C, H, W)
    return out, work


def temporal_loss_bwd(x1: torch.Tensor, x2: torch.Tensor, flow: torch.Tensor, m: torch.Tensor,
                      c1: Optional[torch.Tensor], c2: Optional[torch.Tensor], work: torch.Tensor, g: torch.Tensor,
                      need_dx1: bool = True, need_dx2: bool = True, dx1: Optional[torch.Tensor] = None,
                      dx2: Optional[torch.Tensor] = None):
    """``mhada_temporal_loss_bwd``: (dx1, dx2) of ``temporal_loss_fwd`` for the upstream gradient g (a
    device scalar; no synchronisation) and the forward's ``work``.  dx2 is deterministic; dx1 is an
    atomic scatter like ``warp_bwd``'s.  ``dx1`` (ZEROED) / ``dx2`` may be given as [B,C,H,W] float32
    tensors of any strides; by default they take x1's / x2's layout."""
    flow, m, c1, c2 = _temporal_args(x1, x2, flow, m, c1, c2, "temporal_loss_bwd")
    B, C, H, W = x1.shape
    g = g.to(torch.float32).reshape(1)
    if work.dtype != torch.int64 or work.numel() < 1 or not work.is_contiguous():
        raise ValueError("temporal_loss_bwd: work must be temporal_loss_fwd's int64 workspace")
    if need_dx1 and dx1 is None:
        dx1 = torch.zeros_like(x1)
    if need_dx2 and dx2 is None:
        dx2 = torch.empty_like(x2)
    for d in (dx1, dx2):
        if d is not None and (d.shape != x1.shape or d.dtype != torch.float32 or d.device != x1.device
                              or any(s < 0 for s in d.stride())):
            raise ValueError("temporal_loss_bwd: dx1 / dx2 must be float32 [B,C,H,W] like x1 on its device")
    if dx1 is None and dx2 is None:
        return None, None
    _call("mhada_temporal_loss_bwd", x1, x1.data_ptr(), _strides4(x1), x2.data_ptr(), _strides4(x2), flow.data_ptr(),
          m.data_ptr(), None if c1 is None else c1.data_ptr(), None if c2 is None else c2.data_ptr(),
          work.data_ptr(), g.data_ptr(), None if dx1 is None else dx1.data_ptr(),
          None if dx1 is None else _strides4(dx1), None if dx2 is None else dx2.data_ptr(),
          None if dx2 is None else _strides4(dx2), B, C, H, W)
    return dx1, dx2


def flow_mask_resize(flow: torch.Tensor, mask: torch.Tensor, size):
    """``mhada_flow_mask_resize`` (lossfn.py:71-80): flow [B,2,H,W], mask [B,H,W] -> (the flow resized
    bilinearly to ``size`` = (Hf, Wf) and scaled to that grid, (the resized mask > 0) as floats)."""
    _need_gpu(flow, mask)
    flow, mask = _f32c(flow, "flow"), _f32c(mask, "mask")
    if flow.dim() != 4 or flow.shape[1] != 2 or tuple(mask.shape) != (flow.shape[0],) + tuple(flow.shape[2:]):
        raise ValueError("flow_mask_resize: flow [B,2,H,W], mask [B,H,W]")
    B, _, H, W = flow.shape
    Hf, Wf = int(size[0]), int(size[1])
    fflow = torch.empty(B, 2, Hf, Wf, device=flow.device, dtype=torch.float32)
    fmask = torch.empty(B, Hf, Wf, device=flow.device, dtype=torch.float32)
    _call("mhada_flow_mask_resize", flow, flow.data_ptr(), mask.data_ptr(), fflow.data_ptr(), fmask.data_ptr(),
          B, H, W, Hf, Wf)
    return fflow, fmask


def frame_ingest(frames: torch.Tensor, out_hw=None, bgr: bool = True) -> torch.Tensor:
    """``mhada_frame_ingest``: u8 frames [B][H][W][3] (or one [H][W][3]; rows may be padded) ->
    fp32 [B][3][Ho][Wo] (BGR->RGB, INTER_AREA to out_hw = (Ho, Wo), toTensor255)."""
    _need_gpu(frames)
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 (H, W, 3) images")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3:
        raise ValueError(f"frames must be [B][H][W][3] with packed pixels, got {tuple(frames.shape)}")
    B, H, W, _ = frames.shape
    if B > 1 and frames.stride(0) != H * frames.stride(1):
        frames = frames.contiguous()
    Ho, Wo = (H, W) if out_hw is None else out_hw
    out = torch.empty(B, 3, Ho, Wo, device=frames.device, dtype=torch.float32)
    _call("mhada_frame_ingest", frames, frames.data_ptr(), B, H, W, frames.stride(1), int(bgr), out.data_ptr(), Ho, Wo)
    return out


def _u8_frames(out: Optional[torch.Tensor], B: int, H: int, W: int, device) -> torch.Tensor:
    """The u8 [B][H][W][3] output of frame_emit / conv3x3_out3_u8: a new packed tensor, or the caller's
    ``out`` checked under the stride rules frame_ingest accepts on input (packed pixels, rows of any
    stride >= 3W, images H rows apart)."""
    if out is None:
        return torch.empty(B, H, W, 3, device=device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or out.device != device:
        raise ValueError("out must be a uint8 tensor on the input's device")
    if tuple(out.shape) != (B, H, W, 3) or out.stride(3) != 1 or out.stride(2) != 3:
        raise ValueError(f"out must be [{B}][{H}][{W}][3] with packed pixels, got {tuple(out.shape)} "
                         f"strides {tuple(out.stride())}")
    if out.stride(1) < 3 * W or (B > 1 and out.stride(0) != H * out.stride(1)):
        raise ValueError("out rows must be >= 3*W bytes apart and its images H rows apart")
    return out


def frame_emit(x: torch.Tensor, bgr: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_frame_emit``, the inverse of frame_ingest: fp32 [B][3][H][W] (any range, R,G,B planes) ->
    u8 frames [B][H][W][3], clamp(0, 255) then truncation (numpy ``astype(uint8)``; NaN -> 0), B,G,R
    for ``bgr`` else R,G,B.  ``out``: a u8 [B][H][W][3] tensor to write in place; its rows may be
    padded (a view of a wider buffer), and the padding bytes are not touched."""
    _need_gpu(x, out)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"frame_emit expects a float32 [B][3][H][W] tensor, got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    B, _, H, W = x.shape
    out = _u8_frames(out, B, H, W, x.device)
    _call("mhada_frame_emit", x, x.data_ptr(), B, H, W, out.data_ptr(), out.stride(1), int(bgr))
    return out


# ---- image-quality metrics on u8 frames (csrc/metrics.hip) -------------------------------
def _u8_input(frames: torch.Tensor, what: str) -> torch.Tensor:
    """u8 frames [B][H][W][3] (or one [H][W][3]) on the device, checked under frame_ingest's stride
    rules (packed pixels, rows >= 3W bytes apart); images not H rows apart are copied."""
    _need_gpu(frames)
    if frames.dtype != torch.uint8:
        raise ValueError(f"{what}: frames must be uint8, got {frames.dtype}")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3 or frames.numel() == 0:
        raise ValueError(f"{what}: frames must be [B][H][W][3] with packed pixels, got {tuple(frames.shape)}")
    B, H, W, _ = frames.shape
    if frames.stride(1) < 3 * W:
        raise ValueError(f"{what}: rows must be >= 3*W bytes apart (row_bytes {frames.stride(1)} < {3 * W})")
    if B > 1 and frames.stride(0) != H * frames.stride(1):
        frames = frames.contiguous()
    return frames


# ---- image ingest: PIL's BILINEAR resize (csrc/image_ingest.hip) --------------------------
@functools.lru_cache(maxsize=None)
def pil_bilinear_tables(n_in: int, n_out: int):
    """The coefficient tables of PIL's 8-bit BILINEAR resample of one axis, ``n_in -> n_out`` (Resample.c:
    precompute_coeffs then normalize_coeffs_8bpc), built in IEEE double with every operation in PIL's order:
    ``(coef, bounds)``, read-only CPU int32 arrays [n_out][ksize] and [n_out][2] = (xmin, count).  Row ``i`` of
    ``coef`` holds ``int(0.5 + w * 2^22)`` of the normalised triangle weights of output index ``i`` (zeros past
    ``count``).  Cached per size pair; needs no GPU."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"pil_bilinear_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * inv)) for x in range(xmax)]
        ww = 0.0
        for v in w:  # a running sum in index order, as the C loop adds (not numpy's pairwise sum)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[xx, :xmax] = [int(0.5 + v * 4194304.0) for v in w]
        bounds[xx] = (xmin, xmax)
    coef.setflags(write=False)
    bounds.setflags(write=False)
    return coef, bounds


_RESIZE_TABLES = {}


def _resize_tables(n_in: int, n_out: int, device):
    """pil_bilinear_tables(n_in, n_out) as device tensors, uploaded once per (n_in, n_out, device)."""
    key = (int(n_in), int(n_out), torch.device(device))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        coef, bounds = pil_bilinear_tables(key[0], key[1])
        t = _RESIZE_TABLES[key] = (torch.from_numpy(coef.copy()).to(device), torch.from_numpy(bounds.copy()).to(device))
    return t


def image_resize(frames: torch.Tensor, out_hw, bgr: bool = False, want_u8: bool = True, want_f32: bool = True,
                 out_u8: Optional[torch.Tensor] = None):
    """``mhada_image_resize``: u8 images [B][H][W][3] (or one [H][W][3]; rows may be padded) resized to
    ``out_hw`` = (Ho, Wo) bit for bit as ``PIL.Image.resize(..., Image.BILINEAR)`` does -> ``(u8, f32)``: the
    resized u8 R,G,B images [B][Ho][Wo][3] (``want_u8``; what metrics.score consumes) and the fp32
    [B][3][Ho][Wo] model input toTensor255 makes of them (``want_f32``); an output not wanted is None.
    ``bgr`` swaps channels 0 and 2 on the way in (PIL images are R,G,B).  ``out_u8``: a u8 [B][Ho][Wo][3]
    tensor to write in place; its rows may be padded (a view of a wider buffer), the padding bytes are not
    touched."""
    frames = _u8_input(frames, "image_resize")
    _need_gpu(frames, out_u8)
    B, H, W, _ = frames.shape
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"image_resize: out_hw must be positive, got {(Ho, Wo)}")
    if not (want_u8 or want_f32 or out_u8 is not None):
        raise ValueError("image_resize: want_u8 or want_f32 (or both)")
    dev = frames.device
    u8 = _u8_frames(out_u8, B, Ho, Wo, dev) if (want_u8 or out_u8 is not None) else None
    f32 = torch.empty(B, 3, Ho, Wo, device=dev, dtype=torch.float32) if want_f32 else None
    cx, bx = _resize_tables(W, Wo, dev) if Wo != W else (None, None)
    cy, by = _resize_tables(H, Ho, dev) if Ho != H else (None, None)
    nwork = int(_lib.load().mhada_image_resize_work(B, H, W, Ho, Wo))
    work = torch.empty(nwork, device=dev, dtype=torch.uint8) if nwork else None
    _call("mhada_image_resize", frames, frames.data_ptr(), B, H, W, frames.stride(1), int(bgr),
          _ptr(cx), _ptr(bx), 0 if cx is None else cx.shape[1], _ptr(cy), _ptr(by), 0 if cy is None else cy.shape[1],
          _ptr(u8), 0 if u8 is None else u8.stride(1), _ptr(f32), Ho, Wo, _ptr(work), nwork)
    return u8, f32


_SSIM_WINDOW = None


def ssim_window() -> torch.Tensor:
    """The [11][11] fp32 window of SSIMMetric (eval.py:180-184), built as the reference builds it:
    linspace, exp, normalise and the outer product, each an fp32 torch operation on the CPU."""
    global _SSIM_WINDOW
    if _SSIM_WINDOW is None:
        x = torch.linspace(-5, 5, 11)
        g = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
        g = g / g.sum()
        _SSIM_WINDOW = (g[:, None] @ g[None, :]).contiguous()
    return _SSIM_WINDOW


def ssim_u8(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``mhada_ssim_u8``: per-image SSIM (eval.py:167-223, reduction "none") of two u8 frame batches
    [B][H][W][3] (rows may be padded) -> fp32 [B]; fp64 inside, deterministic."""
    a, b = _u8_input(a, "ssim_u8"), _u8_input(b, "ssim_u8")
    _need_gpu(a, b)
    if a.shape != b.shape:
        raise ValueError(f"ssim_u8: shapes differ, {tuple(a.shape)} and {tuple(b.shape)}")
    B, H, W, _ = a.shape
    nwork = int(_lib.load().mhada_ssim_u8_work(B, H, W))
    work = torch.empty(max(1, nwork), device=a.device, dtype=torch.float64)
    out = torch.empty(B, device=a.device, dtype=torch.float32)
    _call("mhada_ssim_u8", a, a.data_ptr(), a.stride(1), b.data_ptr(), b.stride(1), B, H, W, ssim_window().data_ptr(),
          work.data_ptr(), nwork, out.data_ptr())
    return out


def hist_u8(frames: torch.Tensor, bgr: bool = True) -> torch.Tensor:
    """``mhada_hist_u8``: exact counts int32 [B][4][256] of u8 frames [B][H][W][3] (rows may be
    padded): the three stored channels, then the gray image of cv2's BGR2GRAY (RGB2GRAY without
    ``bgr``).  (The library counts in uint32; below 2^31 pixels the int32 view holds the same values.)"""
    frames = _u8_input(frames, "hist_u8")
    B, H, W, _ = frames.shape
    if H * W >= 1 << 31:
        raise ValueError("hist_u8: 2^31 pixels or more per frame")
    out = torch.empty(B, 4, 256, device=frames.device, dtype=torch.int32)
    _call("mhada_hist_u8", frames, frames.data_ptr(), B, H, W, frames.stride(1), int(bgr), out.data_ptr())
    return out


def gram(feat: torch.Tensor) -> torch.Tensor:
    """gram_matrix (eval.py:70-75) of fp32 features held NHWC, [B][H][W][C] or [B][P][C]: per image
    X^T X / P with X = [P][C], on ``mhada_gemm_tn`` (A = B = X: fp32, deterministic split-K) -> [B][C][C]."""
    _need_gpu(feat)
    if feat.dtype != torch.float32 or feat.dim() not in (3, 4) or not feat.is_contiguous() or feat.numel() == 0:
        raise ValueError("gram: contiguous fp32 NHWC features [B][H][W][C] (or [B][P][C])")
    B, C = feat.shape[0], feat.shape[-1]
    P = feat.numel() // (B * C)
    if C % 4:
        raise ValueError("gram: C must be a multiple of 4")
    x = feat.view(B, P, C)
    out = torch.stack([gemm_tn(x[i], x[i], M=C, N=C, K=P, lda=C, ldb=C) for i in range(B)])
    return out.div_(P)


def lpips_layer(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``mhada_lpips_layer``: the LPIPS distance of one layer (lpips.py:139-147) of two fp32 feature maps
    held NHWC, [B][H][W][C] or [B][P][C], with the linear weights w [C] -> float64 [B]: per pixel
    unit-normalise both vectors over C (eps 1e-10 added to the norm), sum_c w_c (a^_c - b^_c)^2 in fp32,
    then the fp64 mean over the pixels.  One pass over each map, deterministic.  C % 64 == 0, C <= 512."""
    _need_gpu(fa, fb, w)
    if any(t.dtype != torch.float32 for t in (fa, fb, w)):
        raise ValueError(f"lpips_layer: fp32 features and weights, got {fa.dtype}, {fb.dtype}, {w.dtype}")
    if fa.dim() not in (3, 4) or fa.shape != fb.shape or fa.numel() == 0:
        raise ValueError(f"lpips_layer: two NHWC feature maps [B][H][W][C] (or [B][P][C]) of one shape, got "
                         f"{tuple(fa.shape)} and {tuple(fb.shape)}")
    if not (fa.is_contiguous() and fb.is_contiguous() and w.is_contiguous()):
        raise ValueError("lpips_layer: contiguous NHWC storage (an NCHW view is not; permute(0, 2, 3, 1) first)")
    B, C = fa.shape[0], fa.shape[-1]
    if C % 64 or C > 512:
        raise ValueError(f"lpips_layer: C must be a multiple of 64 and at most 512, got {C}")
    if tuple(w.shape) != (C,):
        raise ValueError(f"lpips_layer: w must be [{C}], got {tuple(w.shape)}")
    if (fa.data_ptr() | fb.data_ptr() | w.data_ptr()) & 15:
        raise ValueError("lpips_layer: the tensors must start on 16-byte boundaries")
    P = fa.numel() // (B * C)
    nwork = int(_lib.load().mhada_lpips_layer_work(B, P, C))
    work = torch.empty(max(1, nwork), device=fa.device, dtype=torch.float64)
    out = torch.empty(B, device=fa.device, dtype=torch.float64)
    _call("mhada_lpips_layer", fa, fa.data_ptr(), fb.data_ptr(), w.data_ptr(), B, P, C, work.data_ptr(), nwork,
          out.data_ptr())
    return out


# ---- InceptionV3 trunk of SIFID (csrc/conv2d.hip) and its moments (csrc/sifid.hip) ---------------
_CONV2D_KERNELS = ((1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1))


def _nhwc_f32(x: torch.Tensor, what: str) -> torch.Tensor:
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"{what}: contiguous fp32 NHWC [B][H][W][C], got {x.dtype} {tuple(x.shape)}")
    return x


def conv2d_pack_weight(w: torch.Tensor) -> torch.Tensor:
    """An OIHW filter as ``mhada_conv2d`` reads it: fp32 [Cout][KH][KW][Cin'] with Cin' = Cin rounded up
    to a multiple of 4, the added channels zero (they meet the zero channel of ``inception_input``)."""
    if w.dim() != 4:
        raise ValueError(f"conv2d_pack_weight: OIHW filter, got {tuple(w.shape)}")
    w = w.detach().to(torch.float32).permute(0, 2, 3, 1)
    pad = -w.shape[3] % 4
    if pad:
        w = torch.nn.functional.pad(w, (0, pad))
    return w.contiguous()


def conv2d_out_hw(H: int, W: int, kernel, stride: int, padding):
    return (H + 2 * padding[0] - kernel[0]) // stride + 1, (W + 2 * padding[1] - kernel[1]) // stride + 1


def conv2d(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int = 1,
           padding=(0, 0), relu: bool = True, out: Optional[torch.Tensor] = None, c_off: int = 0) -> torch.Tensor:
    """``mhada_conv2d``: act(scale * conv(x, w) + shift) of fp32 NHWC x [B][H][W][Cin] with a packed filter
    w [Cout][KH][KW][Cin] (``conv2d_pack_weight``), zero padding (ph, pw), stride 1 | 2.  ``out``
    [B][Ho][Wo][ldc] with ``c_off``: the result goes into channels c_off .. c_off + Cout of that buffer
    (the concat buffer of a Mixed block); without it a new [B][Ho][Wo][Cout] tensor."""
    x = _nhwc_f32(x, "conv2d")
    _need_gpu(x, w, scale, shift, out)
    B, H, W, Cin = x.shape
    if w.dtype != torch.float32 or w.dim() != 4 or not w.is_contiguous() or w.shape[3] != Cin:
        raise ValueError(f"conv2d: packed fp32 filter [Cout][KH][KW][{Cin}] (conv2d_pack_weight), got {tuple(w.shape)}")
    Cout, KH, KW, _ = w.shape
    if (KH, KW) not in _CONV2D_KERNELS:
        raise ValueError(f"conv2d: kernel {KH}x{KW} is not one of {_CONV2D_KERNELS}")
    for v, name in ((scale, "scale"), (shift, "shift")):
        if v.dtype != torch.float32 or tuple(v.shape) != (Cout,) or not v.is_contiguous():
            raise ValueError(f"conv2d: {name} must be contiguous fp32 [{Cout}]")
    ph, pw = padding
    Ho, Wo = conv2d_out_hw(H, W, (KH, KW), stride, (ph, pw))
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"conv2d: a {H}x{W} input is smaller than the {KH}x{KW} kernel")
    if out is None:
        if c_off:
            raise ValueError("conv2d: c_off needs out=")
        out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[:3]) != (B, Ho, Wo):
        raise ValueError(f"conv2d: out must be contiguous fp32 [{B}][{Ho}][{Wo}][ldc], got {tuple(out.shape)}")
    ldc = out.shape[3]
    if c_off < 0 or c_off + Cout > ldc:
        raise ValueError(f"conv2d: channels {c_off}..{c_off + Cout} do not fit ldc {ldc}")
    _call("mhada_conv2d", x, x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), B, H, W, Cin,
          Cout, KH, KW, int(stride), int(ph), int(pw), ldc, int(c_off), int(bool(relu)))
    return out


def conv2d_stem(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int = 1,
                padding=(0, 0), relu: bool = True, normalize: bool = True, out: Optional[torch.Tensor] = None,
                c_off: int = 0) -> torch.Tensor:
    """``mhada_conv2d_stem``: the trunk's first conv, direct and in fp64, rounded to fp32 once: x the NCHW fp32
    image [B][3][H][W] (2 x - 1 applied in fp64 when ``normalize``), w the packed filter [Cout][KH][KW][4]
    (``conv2d_pack_weight`` of a 3-channel filter), scale / shift fp64 [Cout] -> NHWC [B][Ho][Wo][Cout], or into
    ``out`` at ``c_off`` as ``conv2d``."""
    _need_gpu(x, w, scale, shift, out)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f"conv2d_stem: fp32 NCHW [B][3][H][W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    B, _, H, W = x.shape
    if w.dtype != torch.float32 or w.dim() != 4 or not w.is_contiguous() or w.shape[3] != 4:
        raise ValueError(f"conv2d_stem: packed fp32 filter [Cout][KH][KW][4] (conv2d_pack_weight), got {tuple(w.shape)}")
    Cout, KH, KW, _ = w.shape
    if (KH, KW) not in _CONV2D_KERNELS:
        raise ValueError(f"conv2d_stem: kernel {KH}x{KW} is not one of {_CONV2D_KERNELS}")
    for v, name in ((scale, "scale"), (shift, "shift")):
        if v.dtype != torch.float64 or tuple(v.shape) != (Cout,) or not v.is_contiguous():
            raise ValueError(f"conv2d_stem: {name} must be contiguous fp64 [{Cout}]")
    ph, pw = padding
    Ho, Wo = conv2d_out_hw(H, W, (KH, KW), stride, (ph, pw))
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"conv2d_stem: a {H}x{W} input is smaller than the {KH}x{KW} kernel")
    if out is None:
        if c_off:
            raise ValueError("conv2d_stem: c_off needs out=")
        out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[:3]) != (B, Ho, Wo):
        raise ValueError(f"conv2d_stem: out must be contiguous fp32 [{B}][{Ho}][{Wo}][ldc], got {tuple(out.shape)}")
    ldc = out.shape[3]
    if c_off < 0 or c_off + Cout > ldc:
        raise ValueError(f"conv2d_stem: channels {c_off}..{c_off + Cout} do not fit ldc {ldc}")
    _call("mhada_conv2d_stem", x, x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), B, H, W,
          Cout, KH, KW, int(stride), int(ph), int(pw), ldc, int(c_off), int(bool(relu)), int(bool(normalize)))
    return out


def maxpool3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None, c_off: int = 0) -> torch.Tensor:
    """``mhada_maxpool3s2``: max_pool2d(3, 2) of fp32 NHWC x; ``out`` / ``c_off`` as in ``conv2d``."""
    x = _nhwc_f32(x, "maxpool3s2")
    B, H, W, C = x.shape
    if H < 3 or W < 3:
        raise ValueError(f"maxpool3s2: a {H}x{W} input is smaller than the 3x3 window")
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    if out is None:
        if c_off:
            raise ValueError("maxpool3s2: c_off needs out=")
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[:3]) != (B, Ho, Wo):
        raise ValueError(f"maxpool3s2: out must be contiguous fp32 [{B}][{Ho}][{Wo}][ldc], got {tuple(out.shape)}")
    _need_gpu(x, out)
    _call("mhada_maxpool3s2", x, x.data_ptr(), out.data_ptr(), B, H, W, C, out.shape[3], int(c_off))
    return out


def avgpool3(x: torch.Tensor) -> torch.Tensor:
    """``mhada_avgpool3``: avg_pool2d(3, 1, 1), count_include_pad=True (/ 9 everywhere), fp32 NHWC."""
    x = _nhwc_f32(x, "avgpool3")
    out = torch.empty_like(x)
    _call("mhada_avgpool3", x, x.data_ptr(), out.data_ptr(), *x.shape)
    return out


def inception_input(x: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """``mhada_inception_input``: NCHW fp32 [B][3][H][W] -> NHWC [B][H][W][4] (channel 3 zero), 2 x - 1
    when ``normalize`` (inception.py:137-138)."""
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f"inception_input: fp32 NCHW [B][3][H][W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 4, device=x.device, dtype=torch.float32)
    _call("mhada_inception_input", x, x.data_ptr(), out.data_ptr(), B, H, W, int(bool(normalize)))
    return out


def _feature_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"{what}: contiguous fp32 feature rows [n][C], got {x.dtype} {tuple(x.shape)}")
    return x


def sifid_stats(x: torch.Tensor):
    """``mhada_sifid_stats``: (mean [C], centred sum of squares [C]) in fp64 of fp32 rows x [n][C]."""
    x = _feature_rows(x, "sifid_stats")
    n, C = x.shape
    mean = torch.empty(C, device=x.device, dtype=torch.float64)
    ssq = torch.empty(C, device=x.device, dtype=torch.float64)
    _call("mhada_sifid_stats", x, x.data_ptr(), n, C, mean.data_ptr(), ssq.data_ptr())
    return mean, ssq


def _check_mean(mean: torch.Tensor, C: int, what: str) -> None:
    if mean.dtype != torch.float64 or tuple(mean.shape) != (C,) or not mean.is_contiguous():
        raise ValueError(f"{what}: mean must be contiguous fp64 [{C}]")


def sifid_cross(x1: torch.Tensor, mean1: torch.Tensor, x2: torch.Tensor, mean2: torch.Tensor) -> torch.Tensor:
    """``mhada_sifid_cross``: the centred cross product Xc1 Xc2^T, fp64 [n1][n2]."""
    x1, x2 = _feature_rows(x1, "sifid_cross"), _feature_rows(x2, "sifid_cross")
    _need_gpu(x1, mean1, x2, mean2)
    C = x1.shape[1]
    if x2.shape[1] != C:
        raise ValueError(f"sifid_cross: the rows differ in width, {C} and {x2.shape[1]}")
    _check_mean(mean1, C, "sifid_cross")
    _check_mean(mean2, C, "sifid_cross")
    out = torch.empty(x1.shape[0], x2.shape[0], device=x1.device, dtype=torch.float64)
    _call("mhada_sifid_cross", x1, x1.data_ptr(), mean1.data_ptr(), x1.shape[0], x2.data_ptr(), mean2.data_ptr(),
          x2.shape[0], C, out.data_ptr())
    return out


def sifid_cov(x: torch.Tensor, mean: torch.Tensor) -> torch.Tensor:
    """``mhada_sifid_cov``: the centred scatter matrix Xc^T Xc, fp64 [C][C] (np.cov times n - 1)."""
    x = _feature_rows(x, "sifid_cov")
    _need_gpu(x, mean)
    n, C = x.shape
    _check_mean(mean, C, "sifid_cov")
    out = torch.empty(C, C, device=x.device, dtype=torch.float64)
    _call("mhada_sifid_cov", x, x.data_ptr(), mean.data_ptr(), n, C, out.data_ptr())
    return out


# ---- training path (fp32, NHWC): backward helpers (include/mhada_hip.h) ------------------
def gemm_tn(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, lda: int, ldb: int = 0,
            b_mode: int = A_ROWS, img=(0, 0, 0), pad: int = 0, colsum: bool = False, nb: int = 1,
            sza: int = 0, szb: int = 0):
    """``mhada_gemm_tn``: C[M][N] = sum_k A[k][m] B[k][n] (fp32), deterministic split-K.  With
    ``colsum`` also the column sums of A (sum_k A[k][m], the bias gradient) from the same pass:
    returns (C, colsum).  ``nb`` > 1: a batch of problems whose A / B start sza / szb elements
    apart (ROWS mode); C is [nb][M][N] and the column sums [nb][M]."""
    _need_gpu(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("gemm_tn is fp32")
    lib = _lib.load()
    splits = lib.mhada_gemm_tn_splits(M, N, K)
    work = torch.empty(max(1, splits) * (M * N + (M if colsum else 0)) if nb == 1 else
                       max(1, splits // nb) * nb * (M * N + (M if colsum else 0)), device=a.device, dtype=torch.float32)
    c = torch.empty(*((nb,) if nb > 1 else ()), M, N, device=a.device, dtype=torch.float32)
    cs = torch.empty(*((nb,) if nb > 1 else ()), M, device=a.device, dtype=torch.float32) if colsum else None
    args = GemmTnArgs()
    args.M, args.N, args.K = M, N, K
    args.a, args.lda, args.b, args.ldb, args.b_mode = a.data_ptr(), lda, b.data_ptr(), ldb, b_mode
    args.img_c, args.img_h, args.img_w = img
    args.pad = pad
    args.c, args.ldc = c.data_ptr(), N
    args.colsum = cs.data_ptr() if colsum else None
    args.nb, args.sza, args.szb = nb, sza, szb
    _call("mhada_gemm_tn", a, ctypes.byref(args), work.data_ptr(), work.numel())
    return (c, cs) if colsum else c


def colsum(x: torch.Tensor) -> torch.Tensor:
    """``mhada_colsum`` over the rows of a contiguous [..., C] fp32 tensor -> [C]."""
    _need_gpu(x)
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    work = torch.empty(min(128, max(1, rows // 64)) * C, device=x.device, dtype=torch.float32)
    _call("mhada_colsum", x, x.data_ptr(), out.data_ptr(), rows, C, work.data_ptr(), work.numel())
    return out


def relu_bwd(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    _need_gpu(dy, y)
    dx = torch.empty_like(y)
    _call("mhada_relu_bwd", y, dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.numel())
    return dx


def feat_stats(x: torch.Tensor, t: Optional[torch.Tensor] = None, stats: bool = True):
    """``mhada_feat_stats`` on NHWC storage x [B][H][W][C] fp32 (t the same shape, or None):
    (mean [B][C], unbiased std [B][C]) or (None, None) without ``stats``, and mean((x - t)^2) as a
    0-dim fp32 device tensor (None without t)."""
    _need_gpu(x, t)
    B, H, W, C = x.shape
    for u in (x, t):
        if u is not None and (u.dtype != torch.float32 or not u.is_contiguous()):
            raise ValueError("feat_stats: contiguous fp32 NHWC operands")
    if t is not None and t.shape != x.shape:
        raise ValueError("feat_stats: target shape")
    if not stats and t is None:
        raise ValueError("feat_stats: nothing to compute")
    P = H * W
    nwork = int(_lib.load().mhada_feat_stats_work(B, P, C))
    work = torch.empty(max(1, nwork), device=x.device, dtype=torch.float64)
    mu = torch.empty(B, C, device=x.device, dtype=torch.float32) if stats else None
    sd = torch.empty(B, C, device=x.device, dtype=torch.float32) if stats else None
    mse = torch.empty((), device=x.device, dtype=torch.float32) if t is not None else None
    ptr = lambda u: None if u is None else u.data_ptr()  # noqa: E731
    _call("mhada_feat_stats", x, x.data_ptr(), ptr(t), ptr(mu), ptr(sd), ptr(mse), work.data_ptr(), nwork, B, P, C)
    return mu, sd, mse


def feat_loss_bwd(x: torch.Tensor, mu: Optional[torch.Tensor], alpha: Optional[torch.Tensor],
                  beta: Optional[torch.Tensor], t: Optional[torch.Tensor], ks: float,
                  kp: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """``mhada_feat_loss_bwd`` on NHWC storage x [B][H][W][C] fp32 (t the same shape, or None;
    mu / alpha / beta [B][C] fp32, or all None; kp a one-element fp32 device tensor or None):
    alpha + beta (x - mu) + ks * kp (x - t), times (x > 0) with ``relu`` (x a ReLU output)."""
    _need_gpu(x)
    B, H, W, C = x.shape
    for u in (x, t, mu, alpha, beta, kp):
        if u is not None and (u.dtype != torch.float32 or not u.is_contiguous()):
            raise ValueError("feat_loss_bwd: contiguous fp32 operands")
    if kp is not None and kp.numel() != 1:
        raise ValueError("feat_loss_bwd: kp is one element")
    if t is not None and t.shape != x.shape:
        raise ValueError("feat_loss_bwd: target shape")
    if alpha is not None and not (alpha.shape == beta.shape == mu.shape == (B, C)):
        raise ValueError("feat_loss_bwd: statistics [B][C]")
    g = torch.empty_like(x)
    ptr = lambda u: None if u is None else u.data_ptr()  # noqa: E731
    _call("mhada_feat_loss_bwd", x, x.data_ptr(), ptr(t), ptr(mu), ptr(alpha), ptr(beta), ptr(kp), float(ks),
          g.data_ptr(), B, H * W, C, int(relu))
    return g


def reflect_fold(dxp: torch.Tensor, relu_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_reflect_fold``; ``relu_mask`` (shaped like the result): zero where relu_mask <= 0."""
    _need_gpu(dxp, relu_mask)
    B, Hp, Wp, C = dxp.shape
    dx = torch.empty(B, Hp - 2, Wp - 2, C, device=dxp.device, dtype=torch.float32)
    if relu_mask is not None and (relu_mask.shape != dx.shape or relu_mask.dtype != torch.float32
                                  or not relu_mask.is_contiguous()):
        raise ValueError("reflect_fold: relu_mask must be a contiguous fp32 tensor shaped like the result")
    _call("mhada_reflect_fold", dxp, dxp.data_ptr(), dx.data_ptr(), B, Hp - 2, Wp - 2, C, _ptr(relu_mask))
    return dx


def maxpool2(x: torch.Tensor) -> torch.Tensor:
    _need_gpu(x)
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=torch.float32)
    _call("mhada_maxpool2", x, x.data_ptr(), y.data_ptr(), B, H, W, C)
    return y


def maxpool2_bwd(x: torch.Tensor, dy: torch.Tensor, relu_mask: bool = False) -> torch.Tensor:
    """MaxPool2d(2, 2) adjoint; relu_mask also applies the ReLU adjoint (x > 0) of a ReLU output x."""
    _need_gpu(x, dy)
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    _call("mhada_maxpool2_bwd", x, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, C, int(relu_mask))
    return dx


def upsample2x_bwd(dy: torch.Tensor, relu_x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of the NHWC bilinear x2; with relu_x (the upsample input, a ReLU output) also the
    producing ReLU's adjoint."""
    _need_gpu(dy, relu_x)
    B, Ho, Wo, C = dy.shape
    dx = torch.empty(B, Ho // 2, Wo // 2, C, device=dy.device, dtype=torch.float32)
    if relu_x is not None and (relu_x.shape != dx.shape or relu_x.dtype != torch.float32 or not relu_x.is_contiguous()):
        raise ValueError("upsample2x_bwd: relu_x must be the contiguous fp32 upsample input")
    _call("mhada_upsample2x_bwd", dy, dy.data_ptr(), _ptr(relu_x), dx.data_ptr(), B, Ho // 2, Wo // 2, C)
    return dx


def vgg_input(img: torch.Tensor, cp: int = 32) -> torch.Tensor:
    _need_gpu(img)
    B, _, H, W = img.shape
    out = torch.empty(B, H, W, cp, device=img.device, dtype=torch.float32)
    _call("mhada_vgg_input", img, img.data_ptr(), out.data_ptr(), B, H, W, cp)
    return out


def vgg_input_bwd(dout: torch.Tensor) -> torch.Tensor:
    _need_gpu(dout)
    B, H, W, cp = dout.shape
    dimg = torch.empty(B, 3, H, W, device=dout.device, dtype=torch.float32)
    _call("mhada_vgg_input_bwd", dout, dout.data_ptr(), dimg.data_ptr(), B, H, W, cp)
    return dimg


def _f32_contig(*ts: torch.Tensor, what: str) -> None:
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: contiguous fp32 tensors expected")


def vgg_stem_dgrad(dy: torch.Tensor, y: torch.Tensor, wd: torch.Tensor) -> torch.Tensor:
    """``mhada_vgg_stem_dgrad``: image gradient [B][3][H][W] of normalise -> conv3x3(3 -> 64, zero
    pad) -> ReLU from dy, y NHWC [B][H][W][64] and the flipped weights wd [9][64][3]."""
    _need_gpu(dy, y, wd)
    _f32_contig(dy, y, wd, what="vgg_stem_dgrad")
    B, H, W, C = y.shape
    if C != 64 or dy.shape != y.shape or wd.shape != (9, 64, 3):
        raise ValueError("vgg_stem_dgrad: dy, y [B][H][W][64], wd [9][64][3]")
    dimg = torch.empty(B, 3, H, W, device=y.device, dtype=torch.float32)
    _call("mhada_vgg_stem_dgrad", y, dy.data_ptr(), y.data_ptr(), wd.data_ptr(), dimg.data_ptr(), B, H, W)
    return dimg


def out3_dgrad(dy: torch.Tensor, y: torch.Tensor, wd: torch.Tensor, relu_x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mhada_out3_dgrad``: input gradient NHWC [B][H][W][64] of ReflectionPad2d(1) -> conv3x3(64 -> 3)
    -> ReLU from dy and the output y (NCHW [B][3][H][W]) and wd [9][3][64] (W[co][ci][tap]); with
    relu_x (the layer input, a ReLU output) also the producing ReLU's adjoint."""
    _need_gpu(dy, y, wd, relu_x)
    _f32_contig(dy, y, wd, *(() if relu_x is None else (relu_x,)), what="out3_dgrad")
    B, C, H, W = y.shape
    if C != 3 or dy.shape != y.shape or wd.shape != (9, 3, 64):
        raise ValueError("out3_dgrad: dy, y [B][3][H][W], wd [9][3][64]")
    dx = torch.empty(B, H, W, 64, device=y.device, dtype=torch.float32)
    if relu_x is not None and relu_x.shape != dx.shape:
        raise ValueError("out3_dgrad: relu_x must be the [B][H][W][64] layer input")
    _call("mhada_out3_dgrad", y, dy.data_ptr(), y.data_ptr(), wd.data_ptr(), _ptr(relu_x), dx.data_ptr(), B, H, W)
    return dx


def out3_wgrad(x: torch.Tensor, dy: torch.Tensor, y: torch.Tensor, bias: bool = True):
    """``mhada_out3_wgrad``: (dw [3][64][3][3], db [3] or None) of the same layer from its input x
    NHWC [B][H][W][64], dy and y NCHW [B][3][H][W]."""
    _need_gpu(x, dy, y)
    _f32_contig(x, dy, y, what="out3_wgrad")
    B, H, W, C = x.shape
    if C != 64 or y.shape != (B, 3, H, W) or dy.shape != y.shape:
        raise ValueError("out3_wgrad: x [B][H][W][64], dy, y [B][3][H][W]")
    lib = _lib.load()
    n = lib.mhada_out3_wgrad_work(B, H, W)
    if n <= 0:
        raise ValueError("out3_wgrad: bad shape")
    work = torch.empty(n, device=x.device, dtype=torch.float32)
    dw = torch.empty(3, 64, 3, 3, device=x.device, dtype=torch.float32)
    db = torch.empty(3, device=x.device, dtype=torch.float32) if bias else None
    _call("mhada_out3_wgrad", x, x.data_ptr(), dy.data_ptr(), y.data_ptr(), dw.data_ptr(), _ptr(db),
          work.data_ptr(), n, B, H, W)
    return dw, db


def rows_normalize(x: torch.Tensor, mu: torch.Tensor, rs: torch.Tensor, unit: bool = False) -> torch.Tensor:
    """``mhada_rows_normalize``: (x - mu) * rs on token rows [B][N][C] (and / |row| if unit)."""
    _need_gpu(x, mu, rs)
    for t in (x, mu, rs):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("rows_normalize needs contiguous float32 rows and statistics")
    B, N, C = x.shape
    if mu.shape != (B, C) or rs.shape != (B, C):
        raise ValueError(f"rows_normalize: statistics {tuple(mu.shape)} do not match rows {tuple(x.shape)}")
    out = torch.empty_like(x)
    _call("mhada_rows_normalize", x, x.data_ptr(), mu.data_ptr(), rs.data_ptr(), out.data_ptr(), int(unit), B, N, C)
    return out


def loss_attn(qn: torch.Tensor, kn: torch.Tensor, v: torch.Tensor, x: torch.Tensor, x_mu: torch.Tensor,
              x_rs: torch.Tensor, activation: int) -> torch.Tensor:
    """``mhada_loss_attn``: AdaAttnForLoss on token rows; returns [B][Nq][Dv] fp32."""
    _need_gpu(qn, kn, v, x, x_mu, x_rs)
    for t in (qn, kn, v, x):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("loss_attn operands must be contiguous float32 token rows")
    B, Nq, Dqk = qn.shape
    Ns, Dv = v.shape[1], v.shape[2]
    if kn.shape != (B, Ns, Dqk) or x.shape != (B, Nq, Dv):
        raise ValueError(f"loss_attn: bad shapes q{tuple(qn.shape)} k{tuple(kn.shape)} v{tuple(v.shape)} "
                         f"x{tuple(x.shape)}")
    out = torch.empty(B, Nq, Dv, device=qn.device, dtype=torch.float32)
    _call("mhada_loss_attn", qn, qn.data_ptr(), kn.data_ptr(), v.data_ptr(), x.data_ptr(), x_mu.data_ptr(),
          x_rs.data_ptr(), out.data_ptr(), B, Nq, Ns, Dqk, Dv, activation)
    return out


def vit_batch_attn_bwd(qkv: torch.Tensor, dout: torch.Tensor, L: int, ntok: int, heads: int,
                       groups: int = 1, planes: bool = False):
    """``mhada_vit_batch_attn_bwd``: fp32 qkv [L][ntok][3C], dout [L][ntok][C] -> dqkv (``groups``
    as in vit_batch_attn); ``planes``: also dqkv's three bf16 planes [3][L * ntok][3C]
    (``mhada_vit_batch_attn_bwd_split3``) -> (dqkv, planes)."""
    _need_gpu(qkv, dout)
    C = qkv.shape[-1] // 3
    if L % groups:
        raise ValueError("vit_batch_attn_bwd: L must be a multiple of groups")
    dqkv = torch.empty_like(qkv)
    pl = torch.empty(3, L * ntok, 3 * C, device=qkv.device, dtype=torch.bfloat16) if planes else None
    Lg = L // groups
    for g in range(groups):
        o3, o1 = g * Lg * ntok * 3 * C * 4, g * Lg * ntok * C * 4
        if planes:
            _call("mhada_vit_batch_attn_bwd_split3", qkv, qkv.data_ptr() + o3, dout.data_ptr() + o1,
                  dqkv.data_ptr() + o3, pl.data_ptr() + o3 // 2, L * ntok * 3 * C, Lg, ntok, heads, C // heads)
        else:
            _call("mhada_vit_batch_attn_bwd", qkv, qkv.data_ptr() + o3, dout.data_ptr() + o1, dqkv.data_ptr() + o3,
                  Lg, ntok, heads, C // heads)
    return (dqkv, pl) if planes else dqkv
