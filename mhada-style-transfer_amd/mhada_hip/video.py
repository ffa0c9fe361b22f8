"""Video-path helpers with the reference's signatures.

* ``warp(x, flo, padding_mode)`` — ``utilities.warp`` (utilities.py:100-118);
* ``flow_warp_mask(flo01, flo10, padding_mode, threshold)`` — utilities.py:121-151;
* ``cv2_to_tensor(img, resize)`` — utilities.py:43-52 (BGR->RGB, INTER_AREA, toTensor255) as one
  HIP pass over the u8 frame in device memory (csrc/ingest.hip);
* ``tensor_to_cv2(cs, bgr)`` — its counterpart, the output conversion of infer_video.py:94,110-112
  (clamp(0,255) -> HWC -> uint8 -> RGB2BGR) as one HIP pass (mhada_frame_emit, csrc/ingest.hip);
* ``warping_error(cs1, cs2, flow, mask)`` — the per-frame optical-flow metric of
  exps_sintel.py:101-109 (sum(mask * |cs2 - warp(cs1, flow)|) / (C*H*W));
* ``VideoStylizer`` — the infer_video.py:58-92 loop: the style is encoded once and, through the
  AdaFormer's per-style cache (engine.style_cache), its K/V projections are reused per frame;
  ``stylize_u8`` returns the cv2-ready u8 frame (mhada_frame_emit, or the decoder's last layer
  writing it itself: mhada_conv3x3_out3_u8); ``stylize_clip`` stylises the T frames of a clip in one
  call, each as if alone, against the one cached style.

The inference forms run the HIP kernels (csrc/warp.hip); the gradient through the warp w.r.t. the
image (train_video.py temporal losses) runs its HIP adjoint (WarpFn / mhada_warp_bwd).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import engine, losses, ops


class WarpFn(torch.autograd.Function):
    """utilities.warp under autograd w.r.t. the image (train_video.py:147-151): forward mhada_warp,
    backward its adjoint mhada_warp_bwd.  The flow is data there (no gradient)."""

    @staticmethod
    def forward(ctx, x, flo, padding_mode):
        ctx.save_for_backward(flo)
        ctx.padding_mode = padding_mode
        return ops.warp(x, flo, padding_mode)

    @staticmethod
    def backward(ctx, gy):
        (flo,) = ctx.saved_tensors
        return ops.warp_bwd(gy, flo, ctx.padding_mode), None, None


def warp(x: torch.Tensor, flo: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    """utilities.warp: bilinear backward warp of x [B,C,H,W] by flow flo [B,2,H,W].  On the device:
    the HIP kernel, with its HIP adjoint when x takes a gradient.  A flow that takes a gradient
    (no reference script differentiates through the flow) evaluates the reference expression with
    differentiable device ops (mhada_hip.losses.warp)."""
    if torch.is_grad_enabled() and flo.requires_grad:
        return losses.warp(x, flo, padding_mode)
    if torch.is_grad_enabled() and x.requires_grad:
        return WarpFn.apply(x, flo, padding_mode)
    return ops.warp(x, flo, padding_mode)


class TemporalLossFn(torch.autograd.Function):
    """One masked, warped MSE of train_video.py's temporal losses (lossfn.py:50-86),
    sum(m (x2 - warp(x1, flow) - t)^2) / (C #{m != 0}), as two HIP launches forward
    (mhada_temporal_loss_fwd: the sum and the count reduced on the device, no host synchronisation)
    and one backward (mhada_temporal_loss_bwd).  t is the luminance of c2 - warp(c1, flow) when
    c1 / c2 are given, else 0.  Saves its inputs and the kernel's small workspace only; flow, m, c1
    and c2 are data (no gradient)."""

    @staticmethod
    def forward(ctx, x1, x2, flow, m, c1, c2):
        out, work = ops.temporal_loss_fwd(x1, x2, flow, m, c1, c2)
        ctx.save_for_backward(x1, x2, flow, m, c1, c2, work)
        return out

    @staticmethod
    def backward(ctx, g):
        x1, x2, flow, m, c1, c2, work = ctx.saved_tensors
        dx1, dx2 = ops.temporal_loss_bwd(x1, x2, flow, m, c1, c2, work, g, need_dx1=ctx.needs_input_grad[0],
                                         need_dx2=ctx.needs_input_grad[1])
        return dx1, dx2, None, None, None, None


def _temporal_fused(images, data) -> bool:
    """The fused route takes float32 device tensors whose data operands (flow, mask, frames) take no
    gradient; everything else evaluates the expressions of mhada_hip.losses."""
    if not all(t.is_cuda and t.dtype == torch.float32 for t in tuple(images) + tuple(data)):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in data))


def output_level_temporal_loss_hip(c1, c2, cs1, cs2, flow, mask) -> torch.Tensor:
    """lossfn.output_level_temporal_loss (lossfn.py:50-66) with nn.MSELoss(reduction="none") as its
    loss matrix, as a 0-d device tensor computed by TemporalLossFn without a host synchronisation
    (the reference's, and mhada_hip.losses', torch.nonzero(m).shape[0] is one).  An all-zero mask gives
    NaN where the reference raises ZeroDivisionError.  CPU tensors, or a flow / mask / c1 / c2 that
    takes a gradient, evaluate mhada_hip.losses.output_level_temporal_loss."""
    if not _temporal_fused((cs1, cs2), (c1, c2, flow, mask)):
        return losses.output_level_temporal_loss(c1, c2, cs1, cs2, flow, mask, torch.nn.MSELoss(reduction="none"))
    if c2.shape[1] > 3:  # the luminance reads channels 0..2 (lossfn.py:53)
        c1, c2 = c1[:, :3], c2[:, :3]
    return TemporalLossFn.apply(cs1, cs2, flow, mask, c1, c2)


def feature_level_temporal_loss_hip(f1, f2, flow, mask) -> torch.Tensor:
    """lossfn.feature_level_temporal_loss (lossfn.py:69-86) with nn.MSELoss(reduction="none"): the flow
    and the mask resized to the feature grid by one launch (mhada_flow_mask_resize), then
    TemporalLossFn on f1 / f2 in their own layout (channels_last views are not copied).  Same
    conventions as output_level_temporal_loss_hip."""
    if not _temporal_fused((f1, f2), (flow, mask)):
        return losses.feature_level_temporal_loss(f1, f2, flow, mask, torch.nn.MSELoss(reduction="none"))
    fflow, fmask = ops.flow_mask_resize(flow, mask, f1.shape[2:])
    return TemporalLossFn.apply(f1, f2, fflow, fmask, None, None)


def cv2_to_tensor(img, resize: Optional[tuple] = None, device: Optional[torch.device] = None) -> torch.Tensor:
    """utilities.cv2_to_tensor: ``img`` is a cv2 BGR u8 frame (H, W, 3) — a numpy array (uploaded
    through pinned memory to ``device``, default the current ROCm device) or a uint8 device
    tensor; ``resize`` = (width, height) as cv2.resize takes it.  Returns the fp32 (3, h, w)
    tensor in [0, 255] on the device (the reference returns it on the CPU and moves it with
    .to(device) at infer_video.py:81).

    Shrinking uses INTER_AREA's box average; enlarging (any axis) OpenCV's area-mode 2-tap
    interpolation (csrc/ingest.hip), as cv2.resize(INTER_AREA) does — so a low-resolution video
    resized to a fixed IMAGE_SIZE (exps_video.py:84, infer_video.py:80) works as in the reference.
    cv2 is not installed here: parity with cv2's bits is unpinned."""
    if not isinstance(img, torch.Tensor):
        t = torch.from_numpy(img)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("cv2_to_tensor expects a uint8 (H, W, 3) BGR frame")
        img = t.pin_memory().to(device or torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    out_hw = None if resize is None else (int(resize[1]), int(resize[0]))
    return ops.frame_ingest(img, out_hw, bgr=True)[0]


# VideoStylizer.stylize_u8's default route to the u8 frame.  False: the decoder ends in mhada_conv3x3_out3
# and mhada_frame_emit converts its fp32 frame (two kernels); True: the fused mhada_conv3x3_out3_u8 (no fp32
# frame in HBM).  Both give the same bits.  The fused kernel had to stay within the same-run A-against-A
# spread of the mhada_conv3x3_out3 kernel time to become the default and did not in three of four cases
# (tools/frame_emit_ab.py, profiles/r21_frame_emit_ab.log: +7.6 / +14.4 / +5.6 / -1.5 us against spreads
# of 4.5 / 2.9 / 4.3 / 1.6 us; DESIGN.md §3a "Frame emit").
STYLIZE_U8_FUSED = False


# VideoStylizer.stylize_clip: the most frames one chunk holds when the caller sets no ``max_frames`` (the
# largest measured, DESIGN.md §3a "Clips")
CLIP_MAX_FRAMES = 16


def tensor_to_cv2(cs: torch.Tensor, bgr: bool = True):
    """The output conversion of infer_video.py:94,110-112 (and exps_video.py / exps_sintel.py), the
    counterpart of cv2_to_tensor: ``cs`` fp32 [3][H][W] or [B][3][H][W] in any range ->
    ``cs.clamp(0, 255)``, channels last, ``astype(np.uint8)`` (truncation), and RGB->BGR when ``bgr``.

    A device tensor takes the HIP pass (ops.frame_emit) and returns the uint8 device tensor
    [H][W][3] / [B][H][W][3] (download it with ``.cpu().numpy()``, a quarter of the fp32 bytes).  A CPU
    tensor evaluates the reference expression and returns the numpy array.  NaN gives 0 on the device
    (numpy leaves it undefined)."""
    if not isinstance(cs, torch.Tensor) or cs.dim() not in (3, 4):
        raise ValueError("tensor_to_cv2 expects a [3][H][W] or [B][3][H][W] tensor")
    if cs.shape[-3] != 3:
        raise ValueError(f"tensor_to_cv2 expects 3 channels, got {cs.shape[-3]}")
    if not cs.is_floating_point():
        raise ValueError(f"tensor_to_cv2 expects a floating-point tensor, got {cs.dtype}")
    single = cs.dim() == 3
    x = cs.detach().unsqueeze(0) if single else cs.detach()
    if x.is_cuda:
        out = ops.frame_emit(x.float(), bgr=bgr)
        return out[0] if single else out
    out = x.float().clamp(0, 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    if bgr:
        out = np.ascontiguousarray(out[..., ::-1])
    return out[0] if single else out


def _frames01(t: torch.Tensor) -> torch.Tensor:
    """A warping_error operand as fp32 NCHW in [0, 1]: fp32 NCHW passes through; a uint8 frame
    [B][H][W][3] (stylize_u8 / tensor_to_cv2) becomes its values / 255, channels first."""
    if t.dtype == torch.uint8:
        return (t.permute(0, 3, 1, 2).float() / 255.0).contiguous()
    return t


def flow_warp_mask(flo01: torch.Tensor, flo10: torch.Tensor, padding_mode: str = "zeros",
                   threshold: float = 2) -> torch.Tensor:
    """utilities.flow_warp_mask: forward/backward flow consistency mask [H,W] (1.0 = valid)."""
    return ops.flow_warp_mask(flo01, flo10, padding_mode, threshold)


def warping_error(cs1: torch.Tensor, cs2: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """exps_sintel.py:101-109 per image: sum(mask * |cs2 - warp(cs1, flow)|) / (C*H*W).
    mask is [B,H,W] (or [H,W] for B == 1).  cs1 / cs2: fp32 NCHW in [0, 1], or uint8 frames
    [B][H][W][3] (both in one channel order), scored as their values / 255 — the quantised frames, as
    exps_sintel.py scores them after its own round trip through uint8 images."""
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    return ops.warp_l1(_frames01(cs1), _frames01(cs2), flow, mask)


class VideoStylizer:
    """infer_video.py:58-92 on the drop-in modules: ``set_style(s)`` encodes the style once,
    ``__call__(frame)`` stylises one content frame [B,3,H,W] (0..255) against it and returns the
    clamped output; ``warping_error(flow, mask)`` scores the last two outputs (exps_sintel).
    ``stylize_u8(frame)`` returns the frame as cv2 wants it (uint8, HWC, BGR), converted on the
    device; it keeps the last two uint8 frames, so after it ``warping_error`` scores
    the quantised frames (values / 255), as exps_sintel.py does after writing and re-reading images."""

    def __init__(self, vit_c, vit_s, ada):
        self.vit_c, self.vit_s, self.ada = vit_c, vit_s, ada
        self.fs = None
        self.prev: Optional[torch.Tensor] = None
        self.cur: Optional[torch.Tensor] = None
        self._host = [None, None]  # stylize_u8(to_host=True): two pinned buffers, used alternately
        self._host_ev = [None, None]
        self._host_i = 0

    @torch.no_grad()
    def set_style(self, s: torch.Tensor) -> None:
        self.fs = self.vit_s(s)

    @torch.no_grad()
    def __call__(self, frame: torch.Tensor) -> torch.Tensor:
        if self.fs is None:
            raise RuntimeError("VideoStylizer: call set_style(style_image) first")
        _, cs = self.ada(self.vit_c(frame), self.fs)
        cs = cs.clamp(0, 255)
        self.prev, self.cur = self.cur, cs
        return cs

    @torch.no_grad()
    def stylize_u8(self, frame: torch.Tensor, bgr: bool = True, to_host: bool = False,
                   fused: Optional[bool] = None):
        """Stylise one content frame [B,3,H,W] (0..255) and return it as uint8 [B][H][W][3], B,G,R
        (``bgr``) or R,G,B: bit for bit the reference's clamp(0,255) -> HWC -> astype(uint8) (->
        RGB2BGR) of what ``__call__`` returns.  ``fused`` (default STYLIZE_U8_FUSED): True — written by the
        decoder's last kernel itself (mhada_conv3x3_out3_u8; the fp32 frame is never stored); False — the
        decoder's fp32 frame converted by mhada_frame_emit.  The same bits either way.  Takes the
        multi-head model or the single-head AdaAttnTransformer.

        Returns the device tensor, or with ``to_host`` a numpy array (B, H, W, 3) — (H, W, 3) for a
        [3,H,W] frame.  The download goes through two pinned host buffers used alternately: a
        non-blocking copy on the current stream, then a wait on that copy's event only (not a device
        synchronize).  The returned array is a COPY of the pinned buffer: it owns its memory, and later
        calls never change it."""
        if self.fs is None:
            raise RuntimeError("VideoStylizer: call set_style(style_image) first")
        single = frame.dim() == 3
        if single:
            frame = frame.unsqueeze(0)
        fused = STYLIZE_U8_FUSED if fused is None else fused
        emit = ("bgr" if bgr else "rgb") if fused else None
        fc = self.vit_c(frame)
        if hasattr(self.ada, "adaAttnHead"):
            _, u8 = engine.adaformer_forward(self.ada, list(fc), list(self.fs), emit_u8=emit)
        else:
            u8 = engine.adaformer1_forward(self.ada, list(fc), list(self.fs), emit_u8=emit)
        if not fused:
            u8 = ops.frame_emit(u8, bgr=bgr)  # clamps: the bits of mhada_conv3x3_out3(clamp255 = 1) cast
        self.prev, self.cur = self.cur, u8
        if not to_host:
            return u8[0] if single else u8
        i = self._host_i
        self._host_i ^= 1
        if self._host[i] is None or self._host[i].shape != u8.shape:
            self._host[i] = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            self._host_ev[i] = torch.cuda.Event()
        self._host[i].copy_(u8, non_blocking=True)
        self._host_ev[i].record()
        self._host_ev[i].synchronize()
        out = self._host[i].numpy().copy()
        return out[0] if single else out

    def _clip_route(self, frames: torch.Tensor) -> bool:
        """The one-call clip route covers device modules of the multi-head model at head widths 32, 64 and 128
        (16, 8 and 4 heads) with either activation, against a style of batch 1."""
        ada = self.ada
        widths = (engine.HEAD_DIM,) + tuple(ops.HD_WIDTHS)
        return (frames.is_cuda and hasattr(ada, "adaAttnHead") and self.fs[0].is_cuda and self.fs[0].shape[0] == 1
                and all(b.head_dim in widths for b in ada.adaAttnHead))

    @staticmethod
    def _clip_chunk(T: int, H: int, W: int, device) -> int:
        """Frames per chunk when the caller sets none: what half of the free device memory holds at about
        1 KiB per output pixel (the decoder's full-resolution 64-channel maps dominate), at most CLIP_MAX_FRAMES."""
        free, _ = torch.cuda.mem_get_info(device)
        free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        return max(1, min(T, CLIP_MAX_FRAMES, int(free // 2 // (1024 * H * W))))

    @torch.no_grad()
    def stylize_clip(self, frames: torch.Tensor, bgr: bool = True, to_host: bool = False, u8: bool = True,
                     max_frames: Optional[int] = None):
        """Stylise the T frames of a clip against the one style of ``set_style``, each exactly as if it had
        been passed alone — NOT ``vit_c(frames)``: the reference ViT attends over the batch axis
        (vit.py:48,59), so a plain batch of frames mixes them with one another.

        ``frames``: fp32 [T][3][H][W] (0..255, R,G,B planes), or uint8 [T][H][W][3] B,G,R (cv2 frames; rows
        may be padded), ingested on the device (mhada_frame_ingest).  Returns uint8 [T][H][W][3] in B,G,R
        (``bgr``) or R,G,B order — ``ops.frame_emit`` of the fp32 result, bit for bit — or with ``u8=False``
        the clamped fp32 [T][3][H][W]; with ``to_host`` as a numpy array.  ``prev`` / ``cur`` become the
        last two frames, so ``warping_error`` scores them as after two single calls.

        A chunk of frames is one ``engine.vit_forward(groups=frames)``, the six MHAda blocks against the ONE
        cached style (the shared-style attention entries: K, V', the plane image and the cosine activation's
        moments exist once, whatever the number of frames) and the decoder over the chunk.  ``max_frames`` bounds the chunk; None sizes it from
        the free device memory, at most CLIP_MAX_FRAMES.  A frame's result does not depend on the other
        frames of the clip, on its place in it, or on the chunking: every chunk runs under
        ``ops.route_as(T, frames in the chunk)``, so each rule that chooses a kernel form from the rows or the
        batch of a call chooses what the whole clip of T frames would take.  The forms, and with them the last
        bits, do depend on T itself (a clip of 3 frames and one of 16 may take different GEMM forms), which is
        also why the result agrees with ``__call__`` on the frame alone to the forward's parity bound and not
        bit for bit.

        Measured at 256x512 (DESIGN.md §3a "Clips"): 1.6-1.7x the per-frame loop's frames/s at 2 frames, 3.5x
        (fp32) and 5.3x (bf16) at 16; one frame per call gains nothing (equal within the per-frame call's own
        spread), and 1080p frames gain 0-4 % at 2 frames for twice the memory.

        Covered: device modules, the multi-head model at head widths 32, 64 and 128 (16, 8 and 4 heads) with
        the softmax or the cosine activation, fp32 and bf16, a style of batch 1.  The single-head width-512
        AdaAttnTransformer, any other head width, a style of another batch and CPU modules evaluate the frames
        one by one through ``__call__`` / ``stylize_u8``: the same result, only slower."""
        if self.fs is None:
            raise RuntimeError("VideoStylizer: call set_style(style_image) first")
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise ValueError("stylize_clip expects fp32 [T][3][H][W] or uint8 [T][H][W][3] frames, got "
                             f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames).__name__}")
        if max_frames is not None and max_frames < 1:
            raise ValueError(f"max_frames must be at least 1, got {max_frames}")
        if frames.dtype == torch.uint8:
            if frames.shape[3] != 3:
                raise ValueError(f"uint8 frames must be [T][H][W][3], got {tuple(frames.shape)}")
            # CPU: the reference's BGR -> RGB, HWC -> CHW, float (utilities.cv2_to_tensor without resize)
            frames = ops.frame_ingest(frames, None, bgr=True) if frames.is_cuda else \
                frames.flip(-1).permute(0, 3, 1, 2).float().contiguous()
        elif not frames.is_floating_point() or frames.shape[1] != 3:
            raise ValueError(f"float frames must be [T][3][H][W], got {frames.dtype} {tuple(frames.shape)}")
        T, _, H, W = frames.shape
        if T == 0:
            raise ValueError("stylize_clip needs at least one frame")
        outs = []
        if self._clip_route(frames):
            step = max_frames if max_frames is not None else self._clip_chunk(T, H, W, frames.device)
            emit = ("bgr" if bgr else "rgb") if (u8 and STYLIZE_U8_FUSED) else None
            for t0 in range(0, T, step):
                x = frames[t0:t0 + step]
                with ops.route_as(T, x.shape[0]):  # the forms of the whole clip, whatever the chunk
                    fc = engine.vit_forward(self.vit_c, x, groups=x.shape[0])
                    _, cs = engine.adaformer_forward(self.ada, list(fc), list(self.fs), emit_u8=emit)
                if u8 and emit is None:
                    cs = ops.frame_emit(cs, bgr=bgr)
                outs.append(cs if u8 else cs.clamp(0, 255))
        else:
            keep = (self.prev, self.cur)
            for t in range(T):
                x = frames[t:t + 1]
                if not u8:
                    outs.append(self(x))
                elif x.is_cuda:
                    outs.append(self.stylize_u8(x, bgr=bgr))
                else:
                    outs.append(torch.from_numpy(tensor_to_cv2(self(x), bgr=bgr)))
            self.prev, self.cur = keep
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        if T > 1:
            self.prev, self.cur = out[T - 2:T - 1], out[T - 1:]
        else:
            self.prev, self.cur = self.cur, out
        return out.cpu().numpy() if to_host else out

    @torch.no_grad()
    def warping_error(self, flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """Scores the last two outputs: fp32 frames of ``__call__`` as values / 255, uint8 frames of
        ``stylize_u8`` as their quantised values / 255 (the L1 sum is the same for B,G,R and R,G,B)."""
        if self.prev is None:
            raise RuntimeError("VideoStylizer: need two frames")
        if self.prev.dtype != self.cur.dtype:
            raise RuntimeError("VideoStylizer: the last two frames come from different calls (__call__ and "
                               "stylize_u8); score two frames of one kind")
        if self.cur.dtype == torch.uint8:
            return warping_error(self.prev, self.cur, flow, mask)
        return warping_error(self.prev / 255.0, self.cur / 255.0, flow, mask)
