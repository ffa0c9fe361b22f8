"""The clip route for the cosine activation and for 4- / 16-head models (head widths 128 / 32):
VideoStylizer.stylize_clip against one cached style through mhada_cosine_attn_shared and
mhada_attn_hd_shared (DESIGN.md §3a "Clips").  Beside tests/test_gpu_clip.py, which covers softmax at 64.

1. the two shared-style entries give, per frame, the bits of the per-batch entries called with the style
   operands repeated B times;
2. fold_block_hd_shared equals the per-batch fold_block_hd;
3. the raw entries and the wrappers refuse bad arguments;
4. clip level, for cosine at 8 heads, softmax at 4 and 16 heads and cosine at 16 heads: the route is taken
   (call counts, one style in every cached side), a frame's result does not depend on the other frames, its
   place or the chunking, the u8 form, both routes meet the full forward's parity bound against the numpy
   oracle's evaluation of each single frame, the clip needs less memory than the replicated-style call, and
   the matched-batch paths return the same bits before and after a clip call.

Operands of 1. are Gaussian, as in test_gpu_clip.py: q of unit scale, K of unit scale in log2 units (softmax
logits of standard deviation sqrt(D): a sharp softmax), V' of unit scale; the cosine operands pass through
cosine_prep / cosine_prep_hd first, as in the engine.  The per-frame fcs statistics differ between frames.
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


def _parity_bound():
    """The bound tests/test_gpu_parity.py and tests/test_gpu_heads.py apply to the full forward, read from
    those files: every `assert mse01(...) < X`, `assert mse_raw(...) < X` and raw-MSE `... .mean()) < X` there
    states one X."""
    here = os.path.dirname(os.path.abspath(__file__))
    found = set()
    for name, pat in (("test_gpu_parity.py", r"assert mse(?:01|_raw)\(.*\) < ([0-9.e+-]+)"),
                      ("test_gpu_heads.py", r"assert (?:mse01\(cs, g\[\"cs\"\]\)|float\(\(\(cs\.astype.*\.mean\(\)\)) "
                                            r"< ([0-9.e+-]+)")):
        got = re.findall(pat, open(os.path.join(here, name)).read())
        assert got, name
        found |= set(got)
    assert len(found) == 1, found
    return float(found.pop())


PARITY_MSE = _parity_bound()  # mse01 for both dtypes, mse_raw for fp32

# (heads, activation): cosine at head width 64 (the linear form), softmax at 128 and 32, cosine at 32
MODELS = [(8, "cosine"), (4, "softmax"), (16, "softmax"), (16, "cosine")]
MODEL_IDS = [f"h{h}-{a}" for h, a in MODELS]


def models(heads, act, dtype):
    vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads, activation=act), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = dtype
    return vc, vs, ada


def stylizer(heads, act, dtype, style_seed=2):
    from mhada_hip.video import VideoStylizer
    st = VideoStylizer(*models(heads, act, dtype))
    st.set_style(seeded_image(1, 40, 56, style_seed).to(DEV))  # Ns = 35
    return st


def frames(seeds):
    return torch.cat([seeded_image(1, 64, 96, s) for s in seeds]).to(DEV)  # Nc = 96


def rep(t, B):
    return t.expand(B, *t.shape[1:]).contiguous()


# ---- 1. shared-style entries ---------------------------------------------------------------------------
def frame_operands(g, B, H, D, Nc, dtype):
    C = H * D
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q = r(B, H, Nc, D).to(DEV, dtype)
    fcs = r(B, Nc, C).to(DEV)
    mu = (r(B, C) * 0.5).to(DEV)            # differ between frames
    rstd = (r(B, C).abs() + 0.5).to(DEV)
    v_mu = r(1, C).to(DEV)
    return q, fcs, mu, rstd, v_mu


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Nc", [64, 96, 200])
@pytest.mark.parametrize("B", [1, 3])
def test_shared_cosine_attention_equals_replicated(B, Nc, dtype):
    from mhada_hip import ops
    H, Ns = 8, 35
    g = torch.Generator(device="cpu").manual_seed(1000 * B + 10 * Nc + Ns)
    q, fcs, mu, rstd, v_mu = frame_operands(g, B, H, 64, Nc, dtype)
    kv = torch.randn(1, H, Ns, 128, generator=g).to(DEV, dtype)
    ops.cosine_prep(q, None)   # separately, as the engine does: q is per frame, kv the one style's
    ops.cosine_prep(None, kv)
    mom = ops.cosine_moments(kv, ops.transpose_v(kv))
    assert mom.shape == (1, H, 65, 132)
    if B > 1:
        assert not torch.equal(mu[0], mu[1]) and not torch.equal(rstd[0], rstd[1])
    got = ops.cosine_attn_shared(q, mom, fcs, mu, rstd, v_mu)
    want = ops.cosine_attn(q, rep(mom, B), fcs, mu, rstd, rep(v_mu, B))
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize("Ns", [35, 64, 130])
@pytest.mark.parametrize("Nc", [64, 200])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", ["softmax", "cosine"])
@pytest.mark.parametrize("D", [32, 128])
def test_shared_hd_attention_equals_replicated(D, act, dtype, B, Nc, Ns):
    from mhada_hip import _lib, ops
    H = 512 // D
    g = torch.Generator(device="cpu").manual_seed(100000 * D + 1000 * B + 10 * Nc + Ns)
    q, fcs, mu, rstd, v_mu = frame_operands(g, B, H, D, Nc, dtype)
    kv = torch.randn(1, H, Ns, 2 * D, generator=g).to(DEV, dtype)
    code = _lib.ACT_COSINE if act == "cosine" else _lib.ACT_SOFTMAX
    if act == "cosine":
        ops.cosine_prep_hd(q, None)   # separately, as the engine does: q is per frame, kv the one style's
        ops.cosine_prep_hd(None, kv)
    if B > 1:
        assert not torch.equal(mu[0], mu[1]) and not torch.equal(rstd[0], rstd[1])
    got = ops.attn_hd_shared(q, kv, fcs, mu, rstd, v_mu, code)
    want = ops.attn_hd(q, rep(kv, B), fcs, mu, rstd, rep(v_mu, B), code)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want)


# ---- 2. the fold -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [32, 128])
def test_shared_hd_fold_equals_the_per_batch_fold(D, dtype):
    """fold_block_hd_shared (the existing entry with the style statistics repeated): wq as fold_block_hd's for
    the B frames, the style side with a leading batch of 1."""
    from mhada_hip import ops
    g = torch.Generator(device="cpu").manual_seed(3 + D)
    H = 512 // D
    B, C = 3, 512
    w = [(torch.randn(H, D, D, generator=g) * 0.1).to(DEV) for _ in range(3)]
    bg, bh = (torch.randn(H, D, generator=g).to(DEV) for _ in range(2))
    rstd_c = (torch.rand(B, C, generator=g) + 0.5).to(DEV)
    mu_s, rstd_s = torch.randn(1, C, generator=g).to(DEV), (torch.rand(1, C, generator=g) + 0.5).to(DEV)
    wq, wkv, bkv, v_mu = ops.fold_block_hd_shared(*w, bg, bh, rstd_c, mu_s, rstd_s, dtype)
    wq0, wkv0, bkv0, v_mu0 = ops.fold_block_hd(*w, bg, bh, rstd_c, rep(mu_s, B), rep(rstd_s, B), dtype)
    assert wkv.shape == (1, H, 2 * D, D) and v_mu.shape == (1, C) and wq.shape == (B, H, D, D)
    assert torch.isfinite(wq0.float()).all() and torch.isfinite(wkv0.float()).all()
    assert torch.equal(wq, wq0) and torch.equal(bkv, bkv0)
    for b in range(B):
        assert torch.equal(wkv[0], wkv0[b]) and torch.equal(v_mu[0], v_mu0[b])


# ---- 3. refusals -------------------------------------------------------------------------------------------
def test_shared_entries_refuse_bad_arguments():
    from mhada_hip import _lib, ops
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(5)
    # cosine at 64
    q, fcs, mu, rstd, v_mu = frame_operands(g, 2, 8, 64, 64, F32)
    mom = torch.zeros(1, 8, 65, 132, device=DEV)
    out = torch.empty(2, 64, 512, device=DEV)
    ptrs = [t.data_ptr() for t in (q, mom, fcs, mu, rstd, v_mu, out)]
    for i in (0, 1, 5, 6):  # q, mom, v_mu, out
        a = list(ptrs)
        a[i] = None
        with pytest.raises(ValueError, match="mhada_cosine_attn_shared"):
            _lib.check(lib.mhada_cosine_attn_shared(*a, _lib.F32, 2, 8, 64, None), "mhada_cosine_attn_shared")
    with pytest.raises(ValueError):
        _lib.check(lib.mhada_cosine_attn_shared(*ptrs, _lib.F32, 0, 8, 64, None), "mhada_cosine_attn_shared")
    with pytest.raises(ValueError):
        ops.cosine_attn_shared(q, rep(mom, 2), fcs, mu, rstd, v_mu)
    with pytest.raises(ValueError):
        ops.cosine_attn_shared(q, mom, fcs, mu, rstd, rep(v_mu, 2))
    # widths 32 / 128
    q, fcs, mu, rstd, v_mu = frame_operands(g, 2, 16, 32, 64, F32)
    kv = torch.zeros(1, 16, 64, 64, device=DEV)
    ptrs = [t.data_ptr() for t in (q, kv, fcs, mu, rstd, v_mu, out)]
    for i in (0, 1, 5, 6):  # q, kv, v_mu, out
        a = list(ptrs)
        a[i] = None
        with pytest.raises(ValueError, match="mhada_attn_hd_shared"):
            _lib.check(lib.mhada_attn_hd_shared(*a, _lib.F32, 2, 16, 32, 64, 64, _lib.ACT_SOFTMAX, None),
                       "mhada_attn_hd_shared")
    for D in (64, 48):
        with pytest.raises(ValueError, match="32 or 128"):
            _lib.check(lib.mhada_attn_hd_shared(*ptrs, _lib.F32, 2, 512 // 64, D, 64, 64, _lib.ACT_SOFTMAX, None),
                       "mhada_attn_hd_shared")
    with pytest.raises(ValueError):
        _lib.check(lib.mhada_attn_hd_shared(*ptrs, _lib.F32, 2, 16, 32, 64, 0, _lib.ACT_SOFTMAX, None),
                   "mhada_attn_hd_shared")
    a = list(ptrs)
    a[1] += 4  # a misaligned kv
    with pytest.raises(ValueError, match="aligned"):
        _lib.check(lib.mhada_attn_hd_shared(*a, _lib.F32, 2, 16, 32, 64, 63, _lib.ACT_SOFTMAX, None),
                   "mhada_attn_hd_shared")
    with pytest.raises(ValueError):
        ops.attn_hd_shared(q, rep(kv, 2), fcs, mu, rstd, v_mu, _lib.ACT_SOFTMAX)
    with pytest.raises(ValueError):
        ops.attn_hd_shared(q, kv, fcs, mu, rstd, rep(v_mu, 2), _lib.ACT_SOFTMAX)
    w = [torch.zeros(16, 32, 32, device=DEV) for _ in range(3)]
    b2 = [torch.zeros(16, 32, device=DEV) for _ in range(2)]
    st1, st2 = torch.ones(1, 512, device=DEV), torch.ones(2, 512, device=DEV)
    with pytest.raises(ValueError):
        ops.fold_block_hd_shared(*w, *b2, st2, st2, st2, F32)
    with pytest.raises(ValueError):
        ops.fold_block_hd_shared(*w, *b2, st2, st1, st2, F32)


# ---- 4. clip level -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("heads,act", MODELS, ids=MODEL_IDS)
def test_clip_takes_the_shared_route(heads, act, dtype, monkeypatch):
    from mhada_hip import ops
    st = stylizer(heads, act, dtype)
    abc = frames([11, 12, 13])
    assert st._clip_route(abc)
    calls = dict(cosine_attn_shared=0, attn_hd_shared=0, cosine_attn=0, attn_hd=0, mhada_attn=0,
                 mhada_attn_shared=0, attn_split3=0, attn_split3_planes=0)

    def counted(name):
        real = getattr(ops, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn

    for name in calls:
        monkeypatch.setattr(ops, name, counted(name))
    st.stylize_clip(abc, u8=False, max_frames=3)
    nblk = len(st.ada.adaAttnHead)
    shared = "cosine_attn_shared" if heads == 8 else "attn_hd_shared"
    assert calls.pop(shared) == nblk
    assert all(v == 0 for v in calls.values()), calls
    sides = st.ada.__dict__["_mhada_style"]["sides"]
    assert len(sides) == nblk
    for side in sides:
        assert side["B"] == 1
        assert side["kv"].shape[0] == 1
        if heads == 8:
            assert side["mom"].shape == (1, heads, 65, 132)
        for k in ("kv", "vt", "mom", "mu_s", "rstd_s"):
            if side.get(k) is not None:
                assert side[k].shape[0] == 1, k


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("heads,act", MODELS, ids=MODEL_IDS)
def test_clip_frames_are_independent(heads, act, dtype):
    st = stylizer(heads, act, dtype)
    abc = frames([11, 12, 13])
    base = st.stylize_clip(abc, u8=False)
    assert base.shape == (3, 3, 64, 96) and base.dtype == F32
    assert torch.isfinite(base).all() and not torch.equal(base[0], base[1])
    axy = frames([11, 21, 22])
    assert torch.equal(st.stylize_clip(axy, u8=False)[0], base[0])
    perm = [2, 0, 1]
    assert torch.equal(st.stylize_clip(abc[perm], u8=False), base[perm])
    for mf in (1, 2):
        assert torch.equal(st.stylize_clip(abc, u8=False, max_frames=mf), base)
    assert torch.equal(st.cur, base[2:3]) and torch.equal(st.prev, base[1:2])


def test_clip_u8_output_is_frame_emit_of_the_fp32_result():
    from mhada_hip import ops
    st = stylizer(16, "cosine", F32)
    abc = frames([11, 12, 13])
    for bgr in (True, False):
        want = ops.frame_emit(st.stylize_clip(abc, u8=False), bgr=bgr)
        got = st.stylize_clip(abc, bgr=bgr, u8=True)
        assert got.dtype == torch.uint8 and got.shape == (3, 64, 96, 3)
        assert torch.equal(got, want)


def mse01(a, b):
    a = np.clip(np.asarray(a, dtype=np.float64), 0, 255) / 255.0
    b = np.clip(np.asarray(b, dtype=np.float64), 0, 255) / 255.0
    return float(((a - b) ** 2).mean())


def mse_raw(a, b):
    return float(((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).mean())


_ORACLE = {}


def oracle_frames(heads, act):
    """The numpy oracle's unclamped cs of each single frame (seeds 11, 12, 13 against style seed 2), computed
    once per model and shared by both dtypes.  8 heads: oracle.mhada_oracle.stylize.  That function does not
    thread the head count, so 4 and 16 heads make its call sequence with it (as tests/test_heads_cpu.py does,
    which pins the oracle to the reference's head-count goldens)."""
    if (heads, act) not in _ORACLE:
        from oracle import mhada_oracle as O
        p_vc, p_vs, p_ada = [O.to_numpy_params(m.state_dict()) for m in models(heads, act, F32)]
        s = seeded_image(1, 40, 56, 2).numpy()
        out = []
        for seed in (11, 12, 13):
            c = seeded_image(1, 64, 96, seed).numpy()
            if heads == 8:
                out.append(O.stylize(c, s, p_vc, p_vs, p_ada, activation=act)[3])
            else:
                fc, fs = O.vit_forward(c, p_vc, heads=heads), O.vit_forward(s, p_vs, heads=heads)
                out.append(O.adaformer_forward(fc, fs, p_ada, heads=heads, activation=act)[1])
        _ORACLE[(heads, act)] = out
    return _ORACLE[(heads, act)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("heads,act", MODELS, ids=MODEL_IDS)
def test_clip_and_per_frame_route_meet_the_parity_bound(heads, act, dtype):
    refs = oracle_frames(heads, act)
    st = stylizer(heads, act, dtype)
    abc = frames([11, 12, 13])
    clip = st.stylize_clip(abc, u8=False).cpu().numpy()
    for i, ref in enumerate(refs):
        one = st(abc[i:i + 1]).cpu().numpy()
        # both routes return clamp(cs, 0, 255): the oracle's cs is clamped the same way for the raw MSE
        refc = np.clip(ref, 0, 255)
        for name, got in (("clip", clip[i:i + 1]), ("frame", one)):
            m01, mr = mse01(got, ref), mse_raw(got, refc)
            print(f"h{heads} {act} {dtype} frame {i} {name}: mse01 {m01:.3e} mse_raw {mr:.3e}")
            assert m01 < PARITY_MSE
            if dtype == F32:
                assert mr < PARITY_MSE


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
    st = VideoStylizer(*models(16, "cosine", F32))
    st.set_style(style)
    st1 = VideoStylizer(*models(16, "cosine", F32))
    st1.set_style(style.expand(3, -1, -1, -1).contiguous())  # the style replicated: the matched-batch path
    p_clip = peak(lambda: st.stylize_clip(abc, u8=False, max_frames=3))
    p_rep = peak(lambda: st1(abc))
    for side in st.ada.__dict__["_mhada_style"]["sides"]:
        assert side["B"] == 1 and side["kv"].shape[0] == 1
    for side in st1.ada.__dict__["_mhada_style"]["sides"]:
        assert side["B"] == 3 and side["kv"].shape[0] == 3
    print(f"peak bytes: clip {p_clip}, replicated style {p_rep}")
    assert p_clip < p_rep


@pytest.mark.parametrize("heads,act", [(4, "softmax"), (8, "cosine")], ids=["h4-softmax", "h8-cosine"])
def test_default_paths_unchanged_by_a_clip_call(heads, act):
    from mhada_hip.video import VideoStylizer
    vc, vs, ada = models(heads, act, F32)
    c = seeded_image(2, 64, 96, 31).to(DEV)
    s = seeded_image(2, 64, 96, 32).to(DEV)
    with torch.no_grad():
        before = [t.clone() for t in ada(vc(c), vs(s))]
        st = VideoStylizer(vc, vs, ada)
        st.set_style(seeded_image(1, 40, 56, 2).to(DEV))
        one_before = st(c[:1]).clone()
        st.stylize_clip(frames([11, 12, 13]), u8=False)
        one_after = st(c[:1])
        after = ada(vc(c), vs(s))
    assert all(torch.isfinite(t).all() for t in before)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(one_before, one_after)
