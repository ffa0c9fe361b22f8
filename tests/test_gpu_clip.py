"""The clip route: T frames per call, each stylised as if alone, against one cached style
(VideoStylizer.stylize_clip; DESIGN.md §3a "Clips").

1. the shared-style attention entries give, per frame, the bits of the per-batch entries called with the
   style operands repeated B times (mhada_attn fp32 / bf16, attn_split3, attn_split3_planes);
2. the grouped batch-axis ViT attention gives the bits of the ungrouped entry on each group's slice (the
   forms built: one image per group);
3. a frame's clip result does not depend on the other frames, on its place, or on the chunking;
4. both the clip route and the per-frame route meet tests/test_gpu_parity.py's bound (pixel MSE on
   clamp(cs, 0, 255) / 255 < 1e-4, fp32 also raw MSE < 1e-4) against the numpy oracle's evaluation of each
   single frame — the two routes may take different GEMM forms (the engine routes on frames x tokens), so
   they are not compared bit for bit;
5. the u8 forms;
6. the style-side tensors exist once, and the call's peak memory is below the replicated-style call's;
7. the default paths return the same bits before and after a clip call on the same modules.

Operands of 1. are Gaussian: q of unit scale, K in log2 units of unit scale (logits of standard deviation 8:
a sharp softmax, as a trained block's), V' of unit scale; the per-frame fcs statistics differ between frames.
"""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
H = 8


def _parity_bound():
    """The bound tests/test_gpu_parity.py applies to the full forward against the goldens and the oracle, read
    from that file: every `assert mse01(...) < X` and `assert mse_raw(...) < X` there states one X."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py")).read()
    found = set(re.findall(r"assert mse(?:01|_raw)\(.*\) < ([0-9.e+-]+)", src))
    assert len(found) == 1, found
    return float(found.pop())


PARITY_MSE = _parity_bound()  # mse01 for both dtypes, mse_raw for fp32


def models(dtype, act="softmax"):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(activation=act), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = dtype
    return vc, vs, ada


def stylizer(dtype, style_seed=2):
    from mhada_hip.video import VideoStylizer
    st = VideoStylizer(*models(dtype))
    st.set_style(seeded_image(1, 40, 56, style_seed).to(DEV))  # Ns = 35
    return st


def frames(seeds):
    return torch.cat([seeded_image(1, 64, 96, s) for s in seeds]).to(DEV)  # Nc = 96


# ---- 1. shared-style attention -------------------------------------------------------------------------
def attn_operands(B, Nc, Ns, dtype):
    from mhada_hip import ops
    g = torch.Generator(device="cpu").manual_seed(1000 * B + 10 * Nc + Ns)
    C = 64 * H
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q = r(B, H, Nc, 64).to(DEV, dtype)
    kv = r(1, H, Ns, 128).to(DEV, dtype)
    vt = ops.transpose_v(kv)
    fcs = r(B, Nc, C).to(DEV)
    mu = (r(B, C) * 0.5).to(DEV)            # differ between frames
    rstd = (r(B, C).abs() + 0.5).to(DEV)
    v_mu = r(1, C).to(DEV)
    return q, kv, vt, fcs, mu, rstd, v_mu


def rep(t, B):
    return t.expand(B, *t.shape[1:]).contiguous()


@pytest.mark.parametrize("Ns", [35, 64, 130])
@pytest.mark.parametrize("Nc", [64, 96, 200])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", ["attn_f32", "attn_bf16", "split3", "split3_planes"])
def test_shared_attention_equals_replicated(form, B, Nc, Ns):
    from mhada_hip import ops
    from mhada_hip._lib import ACT_SOFTMAX
    dtype = BF16 if form == "attn_bf16" else F32
    q, kv, vt, fcs, mu, rstd, v_mu = attn_operands(B, Nc, Ns, dtype)
    if B > 1:
        assert not torch.equal(mu[0], mu[1]) and not torch.equal(rstd[0], rstd[1])
    if form in ("attn_f32", "attn_bf16"):
        got = ops.mhada_attn_shared(q, kv, vt, fcs, mu, rstd, v_mu)
        want = ops.mhada_attn(q, rep(kv, B), rep(vt, B), fcs, mu, rstd, rep(v_mu, B), ACT_SOFTMAX)
    else:
        img = ops.split3_kv(kv, vt)
        shared, plain = (ops.attn_split3_shared, ops.attn_split3) if form == "split3" else \
            (ops.attn_split3_planes_shared, ops.attn_split3_planes)
        got = shared(q, img, Ns, fcs, mu, rstd, v_mu)
        want = plain(q, rep(img, B), Ns, fcs, mu, rstd, rep(v_mu, B))
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want)


# Every shared-style instantiation against its replicated-style model, pinned as tests/test_gpu_attn_forms.py pins
# the per-batch forms (knobs of mhada_set_tuning; Ns % 128 == 0 sends the bf16 fixed shift to the LDS-DMA kernel).
# B = 3 and Nc = 200: a 128- or 256-row query tile would straddle frames if frames were folded into rows.
PINNED = [
    # form, knobs, Ns, the kernel form reached (kAttnShared = 256 in the flagged parameter)
    ("attn_f32", dict(attn_waves=4), 130, "attn_f32_kernel<256, 4>"),
    ("attn_f32", dict(attn_waves=8), 130, "attn_f32_kernel<256, 8>"),
    ("attn_bf16", dict(attn_fixed_shift=0, attn_waves=4), 130, "attn_bf16_kernel<256, 4, 64>"),
    ("attn_bf16", dict(attn_fixed_shift=0, attn_waves=8, attn_tk=64), 130, "attn_bf16_kernel<256, 8, 64>"),
    ("attn_bf16", dict(attn_fixed_shift=0, attn_waves=8, attn_tk=128), 130, "attn_bf16_kernel<256, 8, 128>"),
    ("attn_bf16", dict(attn_fixed_shift=0, attn_waves=8, attn_tk=128), 256, "attn_bf16_kernel<256, 8, 128>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=8), 130, "attn_bf16_fs_kernel<8, 384>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=8), 35, "attn_bf16_fs_kernel<8, 384>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=4), 128, "attn_bf16_fsq_kernel<260>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=4), 256, "attn_bf16_fsq_kernel<260>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=8), 128, "attn_bf16_fsq_kernel<264>"),
    ("attn_bf16", dict(attn_fixed_shift=1, attn_waves=8), 256, "attn_bf16_fsq_kernel<264>"),
    ("split3", dict(attn_waves=4), 130, "attn_s3_kernel<4, .., 257, false>"),
    ("split3", dict(attn_waves=8), 130, "attn_s3_kernel<8, .., 257, false>"),
    ("split3", dict(attn_waves=8), 256, "attn_s3_kernel<8, .., 257, false>"),
    ("split3_planes", dict(attn_waves=4), 130, "attn_s3_kernel<4, .., 257, true>"),
    ("split3_planes", dict(attn_waves=8), 130, "attn_s3_kernel<8, .., 257, true>"),
    ("split3_planes", dict(attn_waves=8), 256, "attn_s3_kernel<8, .., 257, true>"),
]


@pytest.mark.parametrize("form,knobs,Ns,kernel", PINNED, ids=[f"{k}-Ns{n}" for _, _, n, k in PINNED])
def test_every_shared_instantiation_equals_its_model(form, knobs, Ns, kernel):
    from mhada_hip import _lib
    with _lib.tuning(**knobs):
        test_shared_attention_equals_replicated(form, 3, 200, Ns)


def test_shared_attention_refuses_cosine_and_bad_style():
    from mhada_hip import _lib, ops
    q, kv, vt, fcs, mu, rstd, v_mu = attn_operands(2, 64, 64, F32)
    with pytest.raises(ValueError):
        ops.mhada_attn_shared(q, rep(kv, 2), rep(vt, 2), fcs, mu, rstd, v_mu)
    with pytest.raises(ValueError):
        _lib.check(_lib.load().mhada_attn_shared(q.data_ptr(), kv.data_ptr(), vt.data_ptr(), fcs.data_ptr(),
                                                 mu.data_ptr(), rstd.data_ptr(), v_mu.data_ptr(), q.data_ptr(),
                                                 _lib.F32, 2, H, 64, 64, _lib.ACT_COSINE, None), "mhada_attn_shared")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_shared_fold_equals_the_per_batch_fold(dtype):
    """fold_block_shared (the existing entry with the style statistics repeated): wq as fold_block's for the B
    frames, the style side with a leading batch of 1."""
    from mhada_hip import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    B, C = 3, 64 * H
    w = [(torch.randn(H, 64, 64, generator=g) * 0.1).to(DEV) for _ in range(3)]
    bg, bh = (torch.randn(H, 64, generator=g).to(DEV) for _ in range(2))
    rstd_c = (torch.rand(B, C, generator=g) + 0.5).to(DEV)
    mu_s, rstd_s = torch.randn(1, C, generator=g).to(DEV), (torch.rand(1, C, generator=g) + 0.5).to(DEV)
    wq, wkv, bkv, v_mu = ops.fold_block_shared(*w, bg, bh, rstd_c, mu_s, rstd_s, dtype)
    wq0, wkv0, bkv0, v_mu0 = ops.fold_block(*w, bg, bh, rstd_c, rep(mu_s, B), rep(rstd_s, B), dtype)
    assert wkv.shape[0] == 1 and v_mu.shape == (1, C)
    assert torch.equal(wq, wq0) and torch.equal(bkv, bkv0)
    for b in range(B):
        assert torch.equal(wkv[0], wkv0[b]) and torch.equal(v_mu[0], v_mu0[b])


# ---- 2. grouped batch-axis attention -------------------------------------------------------------------
@pytest.mark.parametrize("ntok", [96, 200])
@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("form", ["f32", "bf16", "split3", "half2"])
def test_grouped_vit_attention_equals_slices(form, L, ntok):
    from mhada_hip import ops
    g = torch.Generator(device="cpu").manual_seed(7 * L + ntok)
    C = 64 * H
    qkv = torch.randn(L, ntok, 3 * C, generator=g).to(DEV, BF16 if form == "bf16" else F32)
    if form in ("f32", "bf16"):
        got = ops.vit_batch_attn_grouped(qkv, L, ntok, H, L)
        want = torch.cat([ops.vit_batch_attn(qkv[i:i + 1].contiguous(), 1, ntok, H) for i in range(L)])
    elif form == "split3":
        got = ops.vit_batch_attn_split3_grouped(qkv, L, ntok, H, L)
        want = torch.cat([ops.vit_batch_attn_split3(qkv[i:i + 1].contiguous(), 1, ntok, H) for i in range(L)], dim=1)
    else:
        u = torch.full((C,), 4.0, device=DEV)
        got = ops.vit_batch_attn_half2_grouped(qkv, L, ntok, H, u, L)
        want = torch.cat([ops.vit_batch_attn_half2(qkv[i:i + 1].contiguous(), 1, ntok, H, u) for i in range(L)], dim=1)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want)
    # the loop of the training path's wrapper is the same function
    if form in ("f32", "bf16"):
        assert torch.equal(got, ops.vit_batch_attn(qkv, L, ntok, H, groups=L))


def test_grouped_vit_attention_refuses_larger_groups():
    from mhada_hip import ops
    qkv = torch.zeros(4, 96, 3 * 64 * H, device=DEV)
    with pytest.raises(ValueError):
        ops.vit_batch_attn_grouped(qkv, 4, 96, H, 2)


# ---- 3. frame independence -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_clip_frames_are_independent(dtype):
    st = stylizer(dtype)
    abc = frames([11, 12, 13])
    base = st.stylize_clip(abc, u8=False)
    assert base.shape == (3, 3, 64, 96) and base.dtype == F32
    axy = frames([11, 21, 22])
    assert torch.equal(st.stylize_clip(axy, u8=False)[0], base[0])
    perm = [2, 0, 1]
    assert torch.equal(st.stylize_clip(abc[perm], u8=False), base[perm])
    for mf in (1, 2):
        assert torch.equal(st.stylize_clip(abc, u8=False, max_frames=mf), base)
    assert torch.equal(st.cur, base[2:3]) and torch.equal(st.prev, base[1:2])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_clip_chunking_across_the_routing_thresholds(dtype):
    """14 frames of 256x512 (2048 tokens each): the whole clip is past every rows-based rule (the ViT's SPLIT3 /
    HALF2 GEMMs from ~5 frames, the out-projection and the MHAda plane form from ~14, 8-wave attention blocks
    from 4, the fp32 GEMM's persistent form), chunks of 5 are past some, single frames past none.  Every chunking
    must return the same bits: the chunks take the clip's forms (ops.route_as)."""
    from mhada_hip import engine
    st = stylizer(dtype)
    T, N, C = 14, 2048, 512
    g = torch.Generator(device="cpu").manual_seed(9)
    u8 = torch.randint(0, 256, (T, 256, 512, 3), generator=g, dtype=torch.uint8).to(DEV)
    if dtype == F32:  # the shape does cross the rules: the test is not vacuous
        assert engine._split3_fills(T * N, C, u8.device) and not engine._split3_fills(5 * N, C, u8.device)
        assert engine._split3_fills(5 * N, 3 * C, u8.device) and not engine._split3_fills(N, 3 * C, u8.device)
    whole = st.stylize_clip(u8, max_frames=T)
    for mf in (5, 1):
        assert torch.equal(st.stylize_clip(u8, max_frames=mf), whole), mf
    assert torch.equal(st.stylize_clip(u8), whole)  # the chunk sized from the free memory
    # and the setting does not outlive the call
    from mhada_hip import ops
    assert ops.routed(7) == 7


# ---- 4. agreement with the per-frame route, through the oracle -------------------------------------------
def mse01(a, b):
    a = np.clip(np.asarray(a, dtype=np.float64), 0, 255) / 255.0
    b = np.clip(np.asarray(b, dtype=np.float64), 0, 255) / 255.0
    return float(((a - b) ** 2).mean())


def mse_raw(a, b):
    return float(((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).mean())


@pytest.fixture(scope="module")
def oracle_frames():
    """The numpy oracle's unclamped cs of each single frame (seeds 11, 12, 13 against style seed 2)."""
    from oracle import mhada_oracle as O
    ms = models(F32)
    p = [O.to_numpy_params(m.state_dict()) for m in ms]
    s = seeded_image(1, 40, 56, 2).numpy()
    return [O.stylize(seeded_image(1, 64, 96, seed).numpy(), s, *p)[3] for seed in (11, 12, 13)]


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_clip_and_per_frame_route_meet_the_parity_bound(dtype, oracle_frames):
    st = stylizer(dtype)
    abc = frames([11, 12, 13])
    clip = st.stylize_clip(abc, u8=False).cpu().numpy()
    for i, ref in enumerate(oracle_frames):
        one = st(abc[i:i + 1]).cpu().numpy()
        # both routes return clamp(cs, 0, 255): the oracle's cs is clamped the same way for the raw MSE
        refc = np.clip(ref, 0, 255)
        for name, got in (("clip", clip[i:i + 1]), ("frame", one)):
            m01, mr = mse01(got, ref), mse_raw(got, refc)
            print(f"{dtype} frame {i} {name}: mse01 {m01:.3e} mse_raw {mr:.3e}")
            assert m01 < PARITY_MSE
            if dtype == F32:
                assert mr < PARITY_MSE


# ---- 5. u8 forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [True, False])
def test_clip_u8_output_is_frame_emit_of_the_fp32_result(bgr):
    from mhada_hip import ops
    st = stylizer(F32)
    abc = frames([11, 12, 13])
    want = ops.frame_emit(st.stylize_clip(abc, u8=False), bgr=bgr)
    got = st.stylize_clip(abc, bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == (3, 64, 96, 3)
    assert torch.equal(got, want)
    host = st.stylize_clip(abc, bgr=bgr, to_host=True)
    assert isinstance(host, np.ndarray) and np.array_equal(host, want.cpu().numpy())
    assert torch.equal(st.cur, want[2:3]) and torch.equal(st.prev, want[1:2])


def test_clip_u8_input_equals_cv2_to_tensor_per_frame():
    from mhada_hip.video import cv2_to_tensor
    st = stylizer(F32)
    g = torch.Generator(device="cpu").manual_seed(5)
    u8 = torch.randint(0, 256, (3, 64, 96, 3), generator=g, dtype=torch.uint8).to(DEV)
    ingested = torch.stack([cv2_to_tensor(u8[i]) for i in range(3)])
    assert torch.equal(st.stylize_clip(u8), st.stylize_clip(ingested))


# ---- 6. one style in memory ----------------------------------------------------------------------------
def test_clip_keeps_one_style_and_needs_less_memory():
    abc = frames([11, 12, 13])
    style = seeded_image(1, 40, 56, 2).to(DEV)

    def peak(run):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    from mhada_hip.video import VideoStylizer
    st = VideoStylizer(*models(F32))
    st.set_style(style)
    st1 = VideoStylizer(*models(F32))
    st1.set_style(style.expand(3, -1, -1, -1).contiguous())  # the style replicated: the existing matched-batch path
    p_clip = peak(lambda: st.stylize_clip(abc, u8=False, max_frames=3))
    p_rep = peak(lambda: st1(abc))
    sides = st.ada.__dict__["_mhada_style"]["sides"]
    assert len(sides) == len(st.ada.adaAttnHead)
    for side in sides:
        assert side["B"] == 1
        for k in ("mu_s", "rstd_s", "img", "kv", "vt"):
            if side.get(k) is not None:
                assert side[k].shape[0] == 1
    for side in st1.ada.__dict__["_mhada_style"]["sides"]:
        assert side["B"] == 3
    print(f"peak bytes: clip {p_clip}, replicated style {p_rep}")
    assert p_clip < p_rep


# ---- 7. the default paths are untouched ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_default_paths_unchanged_by_a_clip_call(dtype):
    from mhada_hip.graphs import GraphedStylizer
    from mhada_hip.video import VideoStylizer
    vc, vs, ada = models(dtype)
    c = seeded_image(2, 64, 96, 31).to(DEV)
    s = seeded_image(2, 64, 96, 32).to(DEV)
    g = GraphedStylizer(vc, vs, ada, (2, 3, 64, 96))
    with torch.no_grad():
        before = [t.clone() for t in ada(vc(c), vs(s))]
        gbefore = g(c, s).clone()
        st = VideoStylizer(vc, vs, ada)
        st.set_style(seeded_image(1, 40, 56, 2).to(DEV))
        one_before = st(c[:1]).clone()
        st.stylize_clip(frames([11, 12, 13]), u8=False)
        one_after = st(c[:1])
        after = ada(vc(c), vs(s))
        gafter = g(c, s)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(gbefore, gafter) and torch.equal(gbefore, before[1].clamp(0, 255))
    assert torch.equal(one_before, one_after)
