"""Forward-path engine: the reference modules' forward passes expressed as sequences of
HIP launches on token-major ("NHWC") device buffers.

Layout in HBM (per forward call, B images, N = (H/8)(W/8) tokens, C = 512):
  * ViT residual stream       fp32 [B][N][C]            (LayerNorm inputs / residual adds)
  * GEMM operands             compute dtype (fp32 | bf16) [B*N][K]
  * per-layer ViT outputs     fp32 [B][N][C]; handed to callers as NCHW *views*
                              (x.view(B,h,w,C).permute(0,3,1,2)) — no transpose kernel
  * MHAda per block           Q [B][H][Nc][64], KV [B][H][Ns][128] (K | V'), and
                              VT [B][H][128][ceil64(Ns)] (V'^T | V'^2^T); out [B][Nc][C]
  * decoder                   NHWC activations in the compute dtype; the module output is
                              NCHW fp32 (B,3,8h,8w), written directly by the last conv.
Weights are repacked once per (dtype, parameter version) and cached on the module.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import weakref

import torch

from . import ops
from ._lib import ACT_COSINE, ACT_SOFTMAX

HEAD_DIM = 64
DECODER_LAYERS: Tuple[Tuple[str, bool], ...] = (
    # (name, upsample x2 applied to this layer's INPUT) — conv.py:78-94: bilinear x2 follows
    # conv1.0, conv1.4 and conv2.1, so conv1.1, conv2.0 and conv3.0 read an upsampled input.
    ("conv1.0", False), ("conv1.1", True), ("conv1.2", False), ("conv1.3", False),
    ("conv1.4", False), ("conv2.0", True), ("conv2.1", False), ("conv3.0", True),
)
LAST_LAYER = "conv3.1"
# Where the decoder's bilinear x2 runs: fused into the next conv's operand gather (4 taps per
# staged chunk, no extra HBM round trip) or as a standalone NHWC upsample kernel followed by a
# plain conv (one extra write+read of the upsampled tensor, but the conv keeps its lean
# gather and large tile).  Measured (tools/opbench.py conv): the standalone form is faster
# for every decoder layer in both dtypes (e.g. bf16 256->256 @256: 464 vs 903 us).
FUSE_UPSAMPLE = {torch.float32: False, torch.bfloat16: False}


def _fuse_upsample(dt: torch.dtype, w: torch.Tensor) -> bool:
    """The bf16 64 -> 64 layer runs on the direct tile kernel (csrc/conv_tile.hip), whose fused
    upsample is bit-identical to the separate one and 13 % faster (523 vs 600 us at 1024^2 B4)."""
    return FUSE_UPSAMPLE[dt] or (dt == torch.bfloat16 and w.shape[0] == 64 and w.shape[1] == 9 * 64)


# ---------------------------------------------------------------------------------------
# optional per-kernel event timing (bench.py): HIP events recorded on the launch stream
# ---------------------------------------------------------------------------------------
_event_log = None  # dict name -> list of (start, end) torch.cuda.Event, or None (off)


def record_kernel_events(log) -> None:
    """Enable (pass a dict) or disable (None) event brackets around the named launches."""
    global _event_log
    _event_log = log


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _event_log is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if _event_log is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _event_log.setdefault(self.name, []).append((self.s, e))
        return False


# ---------------------------------------------------------------------------------------
# compute dtype & weight caches
# ---------------------------------------------------------------------------------------
def resolve_compute_dtype(module: torch.nn.Module) -> torch.dtype:
    """fp32 by default (the reference's arithmetic); bf16 when the module's
    ``compute_dtype`` says so or a CUDA autocast region asks for a 16-bit dtype (the HIP path
    has bf16 MFMA kernels only, so float16 autocast also runs bf16)."""
    explicit = getattr(module, "compute_dtype", None)
    if explicit is not None:
        if explicit not in (torch.float32, torch.bfloat16):
            raise ValueError(f"compute_dtype must be torch.float32 or torch.bfloat16, got {explicit}")
        return explicit
    if torch.is_autocast_enabled("cuda"):
        if torch.get_autocast_dtype("cuda") in (torch.bfloat16, torch.float16):
            return torch.bfloat16
    return torch.float32


def _signature(module: torch.nn.Module):
    return tuple((p.data_ptr(), p._version) for p in module.parameters())


def cached_prep(module: torch.nn.Module, dtype: torch.dtype, build):
    cache: Dict = module.__dict__.setdefault("_mhada_prep", {})
    key = (dtype, _signature(module))
    hit = cache.get(dtype)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        prep = build(dtype)
    cache[dtype] = (key, prep)
    return prep


def require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the MI355X-native network runs on ROCm device tensors only; "
                           "move the module and inputs with .to('cuda')")


def to_tokens(x: torch.Tensor) -> torch.Tensor:
    """NCHW (any strides) -> contiguous fp32 [B][H][W][C] (zero-copy for this package's own
    channels-last views)."""
    t = x.permute(0, 2, 3, 1)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def tokens_to_nchw(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    B, _, C = t.shape
    return t.view(B, h, w, C).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------
# ViT (network/vit.py)
# ---------------------------------------------------------------------------------------
def vit_prep(vit, dtype):
    def build(dt):
        pe = vit.patch_embedding.conv_proj
        layers = []
        for blk in vit.encoder:
            att = blk.attention
            layers.append(dict(
                ln1_g=blk.ln1.weight.float().contiguous(), ln1_b=blk.ln1.bias.float().contiguous(),
                ln2_g=blk.ln2.weight.float().contiguous(), ln2_b=blk.ln2.bias.float().contiguous(),
                w_qkv=att.in_proj_weight.to(dt).contiguous(), b_qkv=att.in_proj_bias.float().contiguous(),
                w_o=att.out_proj.weight.to(dt).contiguous(), b_o=att.out_proj.bias.float().contiguous(),
                w1=blk.mlp[0].weight.to(dt).contiguous(), b1=blk.mlp[0].bias.float().contiguous(),
                w2=blk.mlp[2].weight.to(dt).contiguous(), b2=blk.mlp[2].bias.float().contiguous(),
                heads=att.num_heads, eps=blk.ln1.eps))
        return dict(patch_w=pe.weight.reshape(pe.weight.shape[0], -1).to(dt).contiguous(),
                    patch_b=pe.bias.float().contiguous(), layers=layers, pos={})
    return cached_prep(vit, dtype, build)


_NUM_CUS: Dict = {}


def _split3_fills(M: int, N: int, dev: torch.device) -> bool:
    """ops.F32_SPLIT and the SPLIT3 GEMM's 256x256 tiles cover >= 7/8 of the CUs (the rule the fp32
    GEMM dispatch uses for its own persistent kernel)."""
    if not ops.F32_SPLIT:
        return False
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _NUM_CUS:
        _NUM_CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return 8 * ((ops.routed(M) + 255) // 256) * ((N + 255) // 256) >= 7 * _NUM_CUS[idx]


def _w6(L: dict, key: str) -> torch.Tensor:
    """The SPLIT3 form of an fp32 ViT weight (ops.split3_weight), built once per prepared layer."""
    k6 = key + "_split3"
    if k6 not in L:
        with torch.no_grad():
            L[k6] = ops.split3_weight(L[key])
    return L[k6]


def _h2(L: dict, ln: str, key: str) -> Optional[dict]:
    """The HALF2 form of the linear layer `key` fed by LayerNorm `ln` (ops.half2_prepare), decided and built
    once per prepared layer; None: ops.F32_HALF2 is off or the preparation refused (the layer keeps SPLIT3)."""
    if not ops.F32_HALF2:
        return None
    k2 = key + "_half2"
    if k2 not in L:
        with torch.no_grad():
            L[k2] = ops.half2_prepare(L[ln + "_g"], L[ln + "_b"], L[key])
    return L[k2]


def _h2_chain(L: dict, key: str) -> Optional[dict]:
    """The HALF2 chain form (ops.half2_chain_prepare) of MLP2 (`key` "w2": fed by relu(MLP1(ln2)), and only
    where MLP1 itself is HALF2) or of the attention out-projection ("w_o": fed by a convex combination of V
    rows, V the last third of QKV(ln1)), decided and built once per prepared layer; None: a switch is off
    (ops.F32_HALF2, F32_HALF2_CHAIN; for "w_o" also F32_HALF2_CHAIN_OUTPROJ) or the preparation refused (the
    layer keeps SPLIT3)."""
    if not (ops.F32_HALF2 and ops.F32_HALF2_CHAIN) or (key == "w_o" and not ops.F32_HALF2_CHAIN_OUTPROJ):
        return None
    k2 = key + "_half2"
    if k2 not in L:
        with torch.no_grad():
            if key == "w2":
                L[k2] = None if _h2(L, "ln2", "w1") is None else \
                    ops.half2_chain_prepare(L["ln2_g"], L["ln2_b"], L["w1"], L["b1"], L["w2"])
            else:
                C = L["w_o"].shape[1]
                L[k2] = ops.half2_chain_prepare(L["ln1_g"], L["ln1_b"], L["w_qkv"][2 * C:], L["b_qkv"][2 * C:],
                                                L["w_o"])
    return L[k2]


def vit_forward(vit, x: torch.Tensor, groups: int = 1) -> List[torch.Tensor]:
    """VisionTransformer.forward (vit.py:148-169) on the HIP path.

    ``groups`` > 1: x is that many calls' batches concatenated, and every result equals that call's own.
    The reference attends over the batch axis (vit.py:48,59), so without it the images of one call mix;
    everything else in the ViT is per token.  Built for one image per group (the frames of a clip,
    ``VideoStylizer.stylize_clip``): the batch-axis attention is then the grouped pass-through of V
    (mhada_vit_batch_attn*_grouped, one launch).  A CPU tensor evaluates the groups one by one
    (autograd_path.vit_forward)."""
    if groups != 1:
        if groups < 1 or x.dim() != 4 or x.shape[0] % groups:
            raise ValueError(f"groups must divide the batch, got groups {groups} for {tuple(x.shape)}")
        if not x.is_cuda:
            from . import autograd_path
            with torch.no_grad():
                return autograd_path.vit_forward(vit, x, groups)
        if x.shape[0] != groups:
            raise ValueError("vit_forward(groups=) is built for one image per group on the device, got "
                             f"{x.shape[0] // groups}")
    require_device(x, "VisionTransformer")
    dt = resolve_compute_dtype(vit)
    prep = vit_prep(vit, dt)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected an image batch (B, 3, H, W), got {tuple(x.shape)}")
    img = x.float().contiguous()
    B, _, H, W = img.shape
    p = vit.patch_size
    h, w = H // p, W // p
    N = h * w
    C = prep["patch_w"].shape[0]
    pos = None
    if vit.pos_embedding is not None:
        pos = prep["pos"].get((h, w))
        if pos is None:
            pos = ops.pos_embed(vit.pos_embedding.pos_embed.detach().float().contiguous(), h, w)
            prep["pos"][(h, w)] = pos
    tok = ops.patch_embed(img, prep["patch_w"], prep["patch_b"], pos, p)  # [B][N][C] fp32
    xs = tok.view(B * N, C)
    outs = []
    for L in prep["layers"]:
        # fp32: LayerNorm -> bf16 planes -> SPLIT3 GEMM (fp32-accurate on the bf16 MFMA) where the
        # 256x256 tiles fill the chip; small batches keep the fp32 MFMA GEMMs (their 128x128 tiles
        # cover more CUs than 6x-longer SPLIT3 tiles would)
        split = dt == torch.float32 and _split3_fills(B * N, 3 * C, xs.device)
        split_mlp = dt == torch.float32 and _split3_fills(B * N, C, xs.device)
        h2q = _h2(L, "ln1", "w_qkv") if split else None
        h2m = _h2(L, "ln2", "w1") if split_mlp else None
        if h2q is not None:  # HALF2: three fp16 products where SPLIT3 takes six bf16 ones
            qkv = ops.linear_half2(ops.layernorm_half2(xs, L["ln1_g"], L["ln1_b"], L["eps"], h2q["s_a"]),
                                   h2q["w2"], h2q["cs"], L["b_qkv"], dt)
        elif split:
            qkv = ops.linear_split3(ops.layernorm_split3(xs, L["ln1_g"], L["ln1_b"], L["eps"]), _w6(L, "w_qkv"),
                                    L["b_qkv"], dt)
        else:
            hb = ops.layernorm(xs, L["ln1_g"], L["ln1_b"], dt, L["eps"])
            qkv = ops.linear(hb, L["w_qkv"], L["b_qkv"], dt)
        # the out-projection as a SPLIT3 GEMM too: the batch-axis attention writes the planes (no fp32 att)
        q3 = qkv.view(B, N, 3 * C)
        if split_mlp and ops.F32_SPLIT_OUTPROJ and C == L["heads"] * HEAD_DIM \
                and B // groups <= ops.VIT_ATTN_SPLIT3_MAX_L:
            h2o = _h2_chain(L, "w_o")
            if h2o is not None:  # the attention output is bounded by V's bound: fp16 planes, HALF2 GEMM
                att2 = ops.vit_batch_attn_half2(q3, B, N, L["heads"], h2o["u"]) if groups == 1 else \
                    ops.vit_batch_attn_half2_grouped(q3, B, N, L["heads"], h2o["u"], groups)
                xs = ops.linear_half2_planes(att2, h2o["w2"], h2o["cs"], L["b_o"], residual=xs)
            else:
                att3 = ops.vit_batch_attn_split3(q3, B, N, L["heads"]) if groups == 1 else \
                    ops.vit_batch_attn_split3_grouped(q3, B, N, L["heads"], groups)
                xs = ops.linear_split3(att3, _w6(L, "w_o"), L["b_o"], torch.float32, residual=xs)
        else:
            att = ops.vit_batch_attn(q3, B, N, L["heads"]) if groups == 1 else \
                ops.vit_batch_attn_grouped(q3, B, N, L["heads"], groups)
            xs = ops.linear(att.view(B * N, C), L["w_o"], L["b_o"], torch.float32, residual=xs)
        if split_mlp:  # MLP1 writes its ReLU output as planes, MLP2 consumes them (SPLIT3; HALF2 where prepared)
            h2c = _h2_chain(L, "w2")  # None wherever h2m is
            if h2m is not None:
                m1 = ops.linear_half2(ops.layernorm_half2(xs, L["ln2_g"], L["ln2_b"], L["eps"], h2m["s_a"]),
                                      h2m["w2"], h2m["cs"], L["b1"], dt, relu=True, out_planes=True,
                                      out_scale=h2c["u"] if h2c is not None else None)
            else:
                m1 = ops.linear_split3(ops.layernorm_split3(xs, L["ln2_g"], L["ln2_b"], L["eps"]), _w6(L, "w1"),
                                       L["b1"], dt, relu=True, out_planes=True)
            if h2c is not None:
                xs = ops.linear_half2_planes(m1, h2c["w2"], h2c["cs"], L["b2"], residual=xs)
            else:
                xs = ops.linear_split3(m1, _w6(L, "w2"), L["b2"], torch.float32, residual=xs)
        else:
            h2 = ops.layernorm(xs, L["ln2_g"], L["ln2_b"], dt, L["eps"])
            m1 = ops.linear(h2, L["w1"], L["b1"], dt, relu=True)
            xs = ops.linear(m1, L["w2"], L["b2"], torch.float32, residual=xs)
        outs.append(tokens_to_nchw(xs.view(B, N, C), h, w))
    return outs


# ---------------------------------------------------------------------------------------
# MHAda blocks (network/adaDecoder.py)
# ---------------------------------------------------------------------------------------
def block_prep(blk, dtype):
    def build(dt):
        H = blk.num_heads
        d = blk.head_dim

        def stack(lst):
            return torch.stack([m.weight.reshape(d, d) for m in lst]).float().contiguous()

        def stackb(lst):
            return torch.stack([m.bias for m in lst]).float().contiguous()
        C = H * d
        return dict(wf=stack(blk.f_list), wg=stack(blk.g_list), wh=stack(blk.h_list),
                    bf=stackb(blk.f_list), bg=stackb(blk.g_list), bh=stackb(blk.h_list),
                    w_out=blk.out_conv.weight.reshape(C, C).to(dt).contiguous(),
                    b_out=blk.out_conv.bias.float().contiguous())
    return cached_prep(blk, dtype, build)


class _Feat:
    """A token-major fp32 feature map with lazily computed InstanceNorm statistics."""

    def __init__(self, t: torch.Tensor, h: int, w: int):
        self.t, self.h, self.w = t, h, w  # t: [B][N][C]
        self._stats = None
        self.t16 = None  # optional bf16 copy of t (written by the producing GEMM)

    @classmethod
    def from_nchw(cls, x: torch.Tensor):
        _, _, h, w = x.shape
        t = to_tokens(x)
        return cls(t.view(t.shape[0], h * w, t.shape[3]), h, w)

    def stats(self):
        if self._stats is None:
            self._stats = ops.instnorm_stats(self.t)
        return self._stats


def block_forward(blk, fc: _Feat, fs: Optional[_Feat], fcs: _Feat, dt: torch.dtype,
                  side: Optional[dict] = None, want_bf16: bool = False) -> _Feat:
    """AdaAttnMultiHead.forward (adaDecoder.py:162-206) at head width D = 64 (its own kernels) or 32 | 128
    (ops.HD_WIDTHS, csrc/attn_hd.hip): the weight fold, the Q and K|V' projections on mhada_gemm (N = K = D
    and N = 2D, K = D), the attention, the out_conv GEMM.

    ``side`` carries the block's style-only tensors (IN statistics of fs and the style side of the attention,
    below): when it is filled they are reused (fs may then be None), when it is an empty dict they are
    computed and stored into it (the per-style cache of adaformer_forward).
    ``want_bf16``: the out_conv GEMM also writes a bf16 copy of the block output (``.t16``) for
    the decoder's first conv (the last block of a bf16 forward).

    The style side and the attention, per width and activation (``side`` keys in brackets):
      * 64, fp32 softmax with ops.F32_SPLIT_ATTN: kv_proj_split3 writes the bf16 plane image [img];
        attn_split3, or attn_split3_planes + a SPLIT3 out_conv (linear_split3) where its tiles fill the chip.
      * 64, other softmax: the K|V' GEMM with the vt epilogue (K rows into kv, V' into the transposed
        V'^T | V'^2^T image) [kv, vt]; mhada_attn.
      * 64, cosine: on top of that cosine_prep and cosine_moments, the linear form's style moments [mom];
        cosine_prep of q, cosine_attn.
      * 32 / 128: fold_block_hd, the K|V' GEMM without vt (the attention reads kv) [kv], cosine_prep_hd of kv
        and of q for cosine (the flash loop, not the linear form); attn_hd.

    One style for B > 1 content frames (a style batch of 1, in ``fs`` or in the cache; the clip route of
    ``VideoStylizer.stylize_clip``): the block takes the shared-style entries (fold_block_shared /
    fold_block_hd_shared, the style side at the style's batch, mhada_attn_shared / attn_split3_shared /
    attn_split3_planes_shared / cosine_attn_shared / attn_hd_shared), so the style-side tensors exist once;
    every frame gets the result of its own B = 1 call.  Other combinations of unequal batches raise."""
    H, D = blk.num_heads, blk.head_dim
    hd = D in ops.HD_WIDTHS
    if not hd and D != HEAD_DIM:
        raise ValueError("the HIP MHAda kernels implement head_dim (qkv_dim/num_heads) in {32, 64, 128}, "
                         f"got {D}")
    prep = block_prep(blk, dt)
    C = H * D
    B, Nc, Cc = fc.t.shape
    cached = bool(side)
    act = ACT_COSINE if blk.activation_name == "cosine" else ACT_SOFTMAX
    # fp32 softmax at 64: the SPLIT3 attention on bf16 planes of K and V'^T | V'^2^T (csrc/attn_split3.hip)
    split_attn = not hd and act == ACT_SOFTMAX and dt == torch.float32 and ops.F32_SPLIT_ATTN
    kv = vt = mom = img = None
    if cached:
        mu_s, rstd_s, Ns, Bs = side["mu_s"], side["rstd_s"], side["Ns"], side["B"]
        kv, vt, mom, img = side.get("kv"), side.get("vt"), side.get("mom"), side.get("img")
    else:
        if fs.t.shape[2] != C:
            raise ValueError(f"channel mismatch: block expects {C}")
        mu_s, rstd_s = fs.stats()
        Ns, Bs = fs.t.shape[1], fs.t.shape[0]
    shared = Bs == 1 and B > 1  # one style, B frames
    if Bs != B and not shared:
        raise ValueError(f"cached style batch {Bs} != content batch {B}" if cached else
                         f"style batch {Bs} != content batch {B}")
    if Cc != C or fcs.t.shape[2] != C:
        raise ValueError(f"channel mismatch: block expects {C}")
    mu_c, rstd_c = fc.stats()
    mu_o, rstd_o = fcs.stats()
    if hd:
        fold = ops.fold_block_hd_shared if shared else ops.fold_block_hd
    else:
        fold = ops.fold_block_shared if shared else ops.fold_block
    wq, wkv, bkv, v_mu = fold(prep["wf"], prep["wg"], prep["wh"], prep["bg"], prep["bh"],
                              rstd_c, mu_s, rstd_s, dt, ops.LOG2E if act == ACT_SOFTMAX else 1.0)
    dev = fc.t.device
    q = torch.empty(B, H, Nc, D, device=dev, dtype=dt)
    ops.gemm(a=fc.t, w=wq, c=q, M=Nc, N=D, K=D, compute=dt, lda=C, sa=(Nc * C, D), nb=(B, H), a_mu=mu_c,
             smu=(C, D), ldw=D, sw=(H * D * D, D * D), bias=prep["bf"], sb=(0, D), ldc=D, sc=(H * Nc * D, Nc * D))
    if not cached and split_attn:
        # K|V' projection written straight as the SPLIT3 attention's bf16 plane image (no fp32 kv / vt)
        img = ops.kv_proj_split3(fs.t, mu_s, wkv, bkv)
        built = dict(img=img)
    elif not cached:
        kv = torch.empty(Bs, H, Ns, 2 * D, device=dev, dtype=dt)
        vt_args = {}
        if not hd:
            # K rows into kv[..., :64] (the attention's K operand), V' straight into the transposed
            # V'^T | V'^2^T image vt (the GEMM's vt epilogue; kv[..., 64:] unused)
            ldt = (Ns + 63) // 64 * 64
            vt = torch.empty(Bs, H, 2 * D, ldt, device=dev, dtype=dt)
            vt_args = dict(vt=vt, ldt=ldt, svt=(H * 2 * D * ldt, 2 * D * ldt))
        ops.gemm(a=fs.t, w=wkv, c=kv, M=Ns, N=2 * D, K=D, compute=dt, lda=C, sa=(Ns * C, D), nb=(Bs, H),
                 a_mu=mu_s, smu=(C, D), ldw=D, sw=(H * 2 * D * D, 2 * D * D), bias=bkv, sb=(0, 2 * D),
                 ldc=2 * D, sc=(H * Ns * 2 * D, Ns * 2 * D), **vt_args)
        if act == ACT_COSINE and hd:
            ops.cosine_prep_hd(None, kv)
        elif act == ACT_COSINE:
            # the cosine activation's linear form: the style-side moments replace the Nc x Ns loop
            ops.cosine_prep(None, kv)
            mom = ops.cosine_moments(kv, vt)
        built = dict(kv=kv) if hd else dict(kv=kv, vt=vt, mom=mom)
    if not cached and side is not None:
        side.update(mu_s=mu_s, rstd_s=rstd_s, Ns=Ns, B=Bs, **built)
    if act == ACT_COSINE:
        (ops.cosine_prep_hd if hd else ops.cosine_prep)(q, None)
    # fp32 softmax where the tiles fill the chip: the attention writes its output as bf16 planes and out_conv
    # runs as a SPLIT3 GEMM (no fp32 att)
    planes = split_attn and ops.F32_SPLIT_OUTPROJ and _split3_fills(B * Nc, C, dev)
    with _timed("mhada_attn"):
        if hd:
            att = (ops.attn_hd_shared if shared else ops.attn_hd)(q, kv, fcs.t, mu_o, rstd_o, v_mu, act)
        elif act == ACT_COSINE:
            att = (ops.cosine_attn_shared if shared else ops.cosine_attn)(q, mom, fcs.t, mu_o, rstd_o, v_mu)
        elif planes:
            att = (ops.attn_split3_planes_shared if shared else ops.attn_split3_planes)(
                q, img, Ns, fcs.t, mu_o, rstd_o, v_mu)  # [3][B Nc][C] bf16
        elif split_attn:
            att = (ops.attn_split3_shared if shared else ops.attn_split3)(
                q, img, Ns, fcs.t, mu_o, rstd_o, v_mu)  # [B][Nc][C] fp32
        elif shared:
            att = ops.mhada_attn_shared(q, kv, vt, fcs.t, mu_o, rstd_o, v_mu)
        else:
            att = ops.mhada_attn(q, kv, vt, fcs.t, mu_o, rstd_o, v_mu, act)  # [B][Nc][C] dt
    if planes:
        if "w_out_split3" not in prep:
            with torch.no_grad():
                prep["w_out_split3"] = ops.split3_weight(prep["w_out"])
        out = ops.linear_split3(att, prep["w_out_split3"], prep["b_out"], torch.float32)
        return _Feat(out.view(B, Nc, C), fc.h, fc.w)
    out = torch.empty(B * Nc, C, device=dev, dtype=torch.float32)
    t16 = torch.empty(B * Nc, C, device=dev, dtype=torch.bfloat16) if want_bf16 else None
    ops.gemm(a=att.view(B * Nc, C), w=prep["w_out"], c=out, M=B * Nc, N=C, K=C, compute=dt, lda=C, ldw=C,
             bias=prep["b_out"], ldc=C, c2=t16, ldc2=C)
    f = _Feat(out.view(B, Nc, C), fc.h, fc.w)
    f.t16 = None if t16 is None else t16.view(B, Nc, C)
    return f


def adaattn_prep(blk, dtype):
    """Weights of the single-head AdaAttN (f, g, h: 512 x 512 1x1 convs).  bf16: f carries log2(e) in weight
    and bias (the attention's log2-unit Q contract); h also in fp32 for v_mu = W_h mu_s + b_h."""
    def build(dt):
        def w(m):
            return m.weight.reshape(m.weight.shape[0], -1).float()
        qs = ops.LOG2E if dt == torch.bfloat16 else 1.0
        return dict(wf=(w(blk.f) * qs).to(dt).contiguous(), bf=(blk.f.bias.float() * qs).contiguous(),
                    wg=w(blk.g).to(dt).contiguous(), bg=blk.g.bias.float().contiguous(),
                    wh=w(blk.h).to(dt).contiguous(), bh=blk.h.bias.float().contiguous(),
                    wh32=w(blk.h).contiguous())
    return cached_prep(blk, dtype, build)


def adaattn_forward(blk, fc: _Feat, fs: _Feat, fcs: _Feat, dt: torch.dtype, want_bf16: bool = False) -> _Feat:
    """AdaAttN.forward (adaDecoder.py:102-131), one head over all 512 channels; returns the fp32 block output
    [B][Nc][512] as a _Feat.  The projections are ordinary mhada_gemm calls (N = K = 512) fed by
    ops.rows_normalize output (Q, K: the InstanceNorm is applied to the rows, not folded into per-batch
    weights) or by fs itself (V).

    fp32 (and cosine in either dtype: there is no bf16 cosine form at this width, so a bf16 cosine block
    runs this route in fp32): V = h(fs) uncentred, ops.loss_attn at d_qk = d_v = 512 on natural-unit logits;
    cosine divides the Q and K rows by their L2 norm after the projection.
    bf16 softmax (ops.BF16_WIDE_ATTN): ops.attn_wide — Q in log2 units (adaattn_prep), V' = h(fs - mean(fs))
    without bias through the GEMM's a_mu, v_mu = W_h mu_s + b_h added in the attention's epilogue (the 64-wide
    path's centring).  ``want_bf16``: the attention also writes the bf16 copy (``.t16``) for the decoder."""
    C = ops.WIDE_WIDTH
    B, Nc, Cc = fc.t.shape
    if Cc != C or fs.t.shape[2] != C or fcs.t.shape[2] != C or blk.f.weight.shape[0] != C:
        raise ValueError(f"the HIP AdaAttN kernels implement qkv_dim {C}, got channels {Cc} / {fs.t.shape[2]} / "
                         f"{fcs.t.shape[2]} and qkv_dim {blk.f.weight.shape[0]}")
    if fs.t.shape[0] != B or fcs.t.shape[:2] != (B, Nc):
        raise ValueError(f"batch / token mismatch: fc {tuple(fc.t.shape)}, fs {tuple(fs.t.shape)}, fcs {tuple(fcs.t.shape)}")
    Ns = fs.t.shape[1]
    cosine = blk.activation_name == "cosine"
    wide = dt == torch.bfloat16 and not cosine and ops.BF16_WIDE_ATTN
    prep = adaattn_prep(blk, torch.bfloat16 if wide else torch.float32)
    pdt = torch.bfloat16 if wide else torch.float32
    mu_c, rstd_c = fc.stats()
    mu_s, rstd_s = fs.stats()
    mu_o, rstd_o = fcs.stats()
    q = ops.linear(ops.rows_normalize(fc.t, mu_c, rstd_c).view(B * Nc, C), prep["wf"], prep["bf"], pdt).view(B, Nc, C)
    k = ops.linear(ops.rows_normalize(fs.t, mu_s, rstd_s).view(B * Ns, C), prep["wg"], prep["bg"], pdt).view(B, Ns, C)
    if wide:
        v = torch.empty(B, Ns, C, device=fs.t.device, dtype=torch.bfloat16)
        ops.gemm(a=fs.t, w=prep["wh"], c=v, M=Ns, N=C, K=C, compute=torch.bfloat16, lda=C, sa=(Ns * C, 0), nb=(B, 1),
                 a_mu=mu_s, smu=(C, 0), ldw=C, ldc=C, sc=(Ns * C, 0))
        v_mu = ops.linear(mu_s, prep["wh32"], prep["bh"], torch.float32)
        with _timed("mhada_attn"):
            res = ops.attn_wide(q, k, v, fcs.t, mu_o, rstd_o, v_mu, want_bf16=want_bf16)
        out, t16 = res if want_bf16 else (res, None)
    else:
        v = ops.linear(fs.t.view(B * Ns, C), prep["wh"], prep["bh"], torch.float32).view(B, Ns, C)
        if cosine:
            q = q / q.norm(dim=-1, keepdim=True)
            k = k / k.norm(dim=-1, keepdim=True)
        with _timed("mhada_attn"):
            out = ops.loss_attn(q, k, v, fcs.t, mu_o, rstd_o, ACT_COSINE if cosine else ACT_SOFTMAX)
        t16 = None
    f = _Feat(out, fc.h, fc.w)
    f.t16 = t16
    return f


def adaformer1_forward(ada, fc: Sequence[torch.Tensor], fs: Sequence[torch.Tensor],
                       emit_u8: Optional[str] = None) -> torch.Tensor:
    """AdaAttnTransformer.forward (adaDecoder.py:226-232): num_layers single-head AdaAttN blocks and the
    Decoder; returns cs.  No per-style cache (multi-head only).  ``emit_u8``: as in
    decoder_forward_tokens (cs is then the u8 frame)."""
    require_device(fc[0], "AdaAttnTransformer")
    dt = resolve_compute_dtype(ada)
    L = ada.num_layers
    fcf = [_Feat.from_nchw(t) for t in fc[:L]]
    fsf = [_Feat.from_nchw(t) for t in fs[:L]]
    fcs = fcf[0]
    for i in range(L):
        fcs = adaattn_forward(ada.adaAttNs[i], fcf[i], fsf[i], fcs, dt,
                              want_bf16=(dt == torch.bfloat16 and i == L - 1))
    B, N, C = fcs.t.shape
    x16 = None if fcs.t16 is None else fcs.t16.view(B, fcs.h, fcs.w, C)
    return decoder_forward_tokens(ada.decoder, fcs.t.view(B, fcs.h, fcs.w, C), dt, x16=x16, emit_u8=emit_u8)


def style_cache(ada, fs: Sequence[torch.Tensor], dt: torch.dtype):
    """Per-style cache of the blocks' style-side tensors (the video path of
    infer_video.py:58-92: fs = vit_s(style) once, adaFormer(fc, fs) per frame).

    A hit needs the SAME fs tensor objects (held by weak reference, so a freed and reallocated
    buffer can never alias), unchanged in place (tensor._version), the same compute dtype and
    unchanged block parameters.  Returns (per-block dicts, hit).  ``ada.cache_style = False``
    turns the cache off."""
    if not getattr(ada, "cache_style", True):
        return [None] * len(ada.adaAttnHead), False
    sig = tuple(_signature(b) for b in ada.adaAttnHead)
    vers = tuple(t._version for t in fs)
    mode = (dt, ops.F32_SPLIT_ATTN)  # the cached side tensors depend on the attention form
    c = ada.__dict__.get("_mhada_style")
    if (c is not None and c["mode"] == mode and c["sig"] == sig and c["vers"] == vers
            and len(c["refs"]) == len(fs) and all(r() is t for r, t in zip(c["refs"], fs))):
        return c["sides"], True
    sides = [dict() for _ in ada.adaAttnHead]
    ada.__dict__["_mhada_style"] = dict(mode=mode, sig=sig, vers=vers, refs=[weakref.ref(t) for t in fs], sides=sides)
    return sides, False


# ---------------------------------------------------------------------------------------
# Decoder (network/conv.py)
# ---------------------------------------------------------------------------------------
def decoder_prep(dec, dtype):
    def build(dt):
        mods = dict(dec.named_modules())
        layers = []
        for name, up in DECODER_LAYERS:
            conv = mods[name].conv.conv
            w = conv.weight.permute(0, 2, 3, 1).reshape(conv.weight.shape[0], -1).to(dt).contiguous()
            # fp32: the Winograd-transformed filters (ops.conv3x3 runs F(2x2,3x3) when eligible)
            u = ops.wino_weights(w) if dt == torch.float32 and w.shape[0] % 64 == 0 and (w.shape[1] // 9) % 8 == 0 \
                else None
            layers.append((w, conv.bias.float().contiguous(), up, u))
        last = mods[LAST_LAYER].conv.conv
        # [out][cin][ky][kx] -> [ky*3+kx][cin][out]
        return dict(layers=layers, w_last=last.weight.permute(2, 3, 1, 0).float().contiguous(),
                    b_last=last.bias.float().contiguous())
    return cached_prep(dec, dtype, build)


def decoder_forward_tokens(dec, x_nhwc: torch.Tensor, dt: torch.dtype, clamp255: bool = False,
                           x16: Optional[torch.Tensor] = None, emit_u8: Optional[str] = None) -> torch.Tensor:
    """Decoder.forward (conv.py:96-100) on NHWC input; returns NCHW fp32 (B,3,8h,8w).  ``x16``: a
    bf16 copy of the input (bf16 compute: the first conv then runs on the bf16 ping-pong GEMM
    instead of converting fp32 rows on load).  ``emit_u8`` = "bgr" | "rgb": the last layer writes
    the clamped u8 frame (B,8h,8w,3) in that channel order instead (ops.conv3x3_out3_u8)."""
    if emit_u8 not in (None, "bgr", "rgb"):
        raise ValueError(f'emit_u8 must be None, "bgr" or "rgb", got {emit_u8!r}')
    prep = decoder_prep(dec, dt)
    x = x16 if (x16 is not None and dt == torch.bfloat16) else x_nhwc
    for w, b, up, u in prep["layers"]:
        if up and not _fuse_upsample(dt, w):
            x = ops.upsample2x(x)
            up = False
        x = ops.conv3x3(x, w, b, dt, upsample=up, relu=True, wino_u=u)
    if emit_u8 is not None:
        return ops.conv3x3_out3_u8(x, prep["w_last"], prep["b_last"], bgr=(emit_u8 == "bgr"))
    return ops.conv3x3_out3(x, prep["w_last"], prep["b_last"], clamp255=clamp255)


def adaformer_forward(ada, fc: Sequence[torch.Tensor], fs: Sequence[torch.Tensor], emit_u8: Optional[str] = None):
    """AdaAttnTransformerMultiHead.forward (adaDecoder.py:253-268): returns (fcs, cs).  ``emit_u8``: as in
    decoder_forward_tokens (cs is then the u8 frame)."""
    require_device(fc[0], "AdaAttnTransformerMultiHead")
    dt = resolve_compute_dtype(ada)
    L = ada.num_layers
    fcf = [_Feat.from_nchw(t) for t in fc[:L]]
    sides, hit = style_cache(ada, fs[:L], dt)
    fsf = [None] * L if hit else [_Feat.from_nchw(t) for t in fs[:L]]
    fcs = fcf[0]
    for i in range(L):
        fcs = block_forward(ada.adaAttnHead[2 * i], fcf[i], fsf[i], fcs, dt, sides[2 * i])
        fcs = block_forward(ada.adaAttnHead[2 * i + 1], fcs, fsf[i], fcs, dt, sides[2 * i + 1],
                            want_bf16=(dt == torch.bfloat16 and i == L - 1))
    B, N, C = fcs.t.shape
    x16 = None if fcs.t16 is None else fcs.t16.view(B, fcs.h, fcs.w, C)
    cs = decoder_forward_tokens(ada.decoder, fcs.t.view(B, fcs.h, fcs.w, C), dt, x16=x16, emit_u8=emit_u8)
    return tokens_to_nchw(fcs.t, fcs.h, fcs.w), cs
