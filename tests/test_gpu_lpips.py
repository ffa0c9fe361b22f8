"""LPIPS on the device (csrc/lpips.hip, network.VGG16, mhada_hip.metrics) against the fp64 restatements of
tests/lpips_ref.py: the fused distance head on synthetic features within its a-priori fp32 bound, the HIP
VGG16 trunk against fp64 aten, metrics.lpips end to end on the golden frames, and metrics.score with the
two LPIPS columns on the output of VideoStylizer.stylize_u8."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lpips_ref as L
import network
from conftest import load_golden
from mhada_hip import _lib, metrics, ops, video
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"
# (64,1,1) one pixel; (64,5,7) 35 pixels, odd; (512,2,2) widest rows, fewer pixels than waves in a workgroup;
# (512,3,33) 99 pixels; (192,4,5) a C that is no power of two; (512,40,40) 1600 pixels, many workgroups' partials
HEAD_SHAPES = [(64, 1, 1), (64, 5, 7), (128, 3, 3), (256, 8, 8), (512, 2, 2), (512, 3, 33), (192, 4, 5), (512, 40, 40)]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def to_dev(frames: np.ndarray, pad: int = 0, fill: int = 0xFF, guard_rows: int = 0):
    """The frames on the device: packed, or as a view with rows of 3W + pad bytes inside a buffer whose
    other bytes (row padding, `guard_rows` rows after the last image) hold `fill`."""
    t = torch.from_numpy(np.ascontiguousarray(frames))
    if not pad and not guard_rows:
        return t.to(DEV)
    B, H, W, _ = frames.shape
    rb = 3 * W + pad
    buf = torch.full(((B * H + guard_rows) * rb,), fill, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((B, H, W, 3), (H * rb, rb, 3, 1))
    view.copy_(t.to(DEV))
    return view


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("lpips_vgg16_48_b2")


@functools.lru_cache(maxsize=None)
def gold_lins():
    return tuple(torch.from_numpy(gold()[f"lin{k}"]) for k in range(5))


@functools.lru_cache(maxsize=None)
def head_case(shape):
    """(fa, fb, w) fp32 CPU tensors, B = 2 with different images: rand with about half the entries zero, as
    after a ReLU, and planted pixels: 0 all zero in a only, 1 all zero in both, 2 equal in a and b, 3 with
    values in [1e-11, 1e-10] in both, so that the + 1e-10 decides the result.  Plant j sits at pixel j P / 4;
    a single-pixel map holds plant 3 in image 0 and plant 0 in image 1."""
    C, H, W = shape
    B, P = 2, H * W
    g = torch.Generator().manual_seed(1000 * C + P)

    def feat():
        x = torch.rand(B, P, C, generator=g)
        return x * (torch.rand(B, P, C, generator=g) < 0.5)

    fa, fb = feat(), feat()
    for n in range(B):
        for j in range(4):
            if P < 4 and j != (3, 0)[n]:
                continue
            p = j * P // 4 if P >= 4 else 0
            if j == 0:
                fa[n, p] = 0.0
            elif j == 1:
                fa[n, p] = 0.0
                fb[n, p] = 0.0
            elif j == 2:
                fb[n, p] = fa[n, p]
            else:
                fa[n, p] = 1e-11 + 9e-11 * torch.rand(C, generator=g)
                fb[n, p] = 1e-11 + 9e-11 * torch.rand(C, generator=g)
    lin = {64: 0, 128: 1, 256: 2, 512: 3 if P != 99 else 4}.get(C)
    w = gold_lins()[lin] if lin is not None else 1.3 * torch.rand(C, generator=g)
    return fa.view(B, H, W, C).contiguous(), fb.view(B, H, W, C).contiguous(), w.contiguous()


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=ids)
def test_head_is_within_the_fp32_bound_of_the_fp64_value(shape):
    fa, fb, w = head_case(shape)
    want = L.lpips_layer64(fa.numpy(), fb.numpy(), w.numpy())
    bound = L.bound_layer(fa.numpy(), fb.numpy(), w.numpy())
    assert np.isfinite(want).all() and (bound > 0).all()
    da, db, dw = fa.to(DEV), fb.to(DEV), w.to(DEV)
    got = ops.lpips_layer(da, db, dw)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
    g = got.cpu().numpy()
    print(shape, "value", want, "max |err| / bound", (np.abs(g - want) / bound).max())
    assert (np.abs(g - want) <= bound).all(), (g, want, bound)
    ba = ops.lpips_layer(db, da, dw)
    assert (np.abs(ba.cpu().numpy() - want) <= bound).all() and (np.abs((ba - got).cpu().numpy()) <= bound).all()
    assert torch.equal(got, ops.lpips_layer(da, db, dw))  # repeatable
    B, H, W, C = fa.shape
    assert torch.equal(got, ops.lpips_layer(da.view(B, H * W, C), db.view(B, H * W, C), dw))  # the [B][P][C] form


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=ids)
def test_head_of_identical_maps_is_exactly_zero(shape):
    fa, fb, w = head_case(shape)
    for x in (fa.to(DEV), fb.to(DEV)):
        assert ops.lpips_layer(x, x, w.to(DEV)).tolist() == [0.0, 0.0]
        assert ops.lpips_layer(x, x.clone(), w.to(DEV)).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("shape", [(64, 5, 7), (512, 5, 7)], ids=ids)
@pytest.mark.parametrize("where", ["middle", "end"])
def test_head_reads_nothing_outside_its_maps(shape, where):
    """The maps as views into buffers whose other floats are NaN: 35 pixels (the last wave pass is partly
    past the map), C = 64 (four pixels per wave) and C = 512, in the middle and at the very end of the buffer."""
    fa, fb, w = head_case((shape[0], 5, 7))
    n = fa.numel()
    head, tail = 256, (256 if where == "middle" else 0)  # floats; 16-byte aligned starts
    views = []
    for f in (fa, fb):
        buf = torch.full((head + n + tail,), float("nan"), device=DEV)
        v = buf[head:head + n].view(fa.shape)
        v.copy_(f)
        views.append(v)
    wbuf = torch.full((64 + w.numel(),), float("nan"), device=DEV)
    wbuf[64:].copy_(w)
    got = ops.lpips_layer(views[0], views[1], wbuf[64:])
    assert torch.isfinite(got).all()
    assert torch.equal(got, ops.lpips_layer(fa.to(DEV), fb.to(DEV), w.to(DEV)))


# ---- trunk -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vgg16():
    return L.vgg16_kaiming().to(DEV)


def test_vgg16_trunk_against_fp64_aten():
    """48 x 40, B = 2 (the size of test_vgg19_and_decoder_modules_against_aten_autograd, with its tolerance):
    the device taps against fp64 aten on scaling64 of the u8 frame, through frame_ingest in both channel orders."""
    rgb = np.random.default_rng(48).integers(0, 256, (2, 48, 40, 3), dtype=np.uint8)
    truth = L.vgg16_taps(L.vgg16_kaiming(), L.scaling64(rgb))
    for bgr in (True, False):
        stored = np.ascontiguousarray(rgb[..., ::-1]) if bgr else rgb
        with torch.no_grad():
            feats = vgg16()(ops.frame_ingest(to_dev(stored, 5 if bgr else 0), bgr=bgr))
        assert tuple(feats) == L.TAPS
        for s, (name, c) in enumerate(zip(L.TAPS, L.CHNS)):
            assert tuple(feats[name].shape) == (2, c, 48 >> s, 40 >> s), name
            assert feats[name].permute(0, 2, 3, 1).is_contiguous(), name  # an NCHW view of NHWC storage
            e = rel(feats[name].cpu(), truth[s])
            print("bgr", bgr, name, "rel", e)
            assert e < 1e-5, (name, e)
    a = to_dev(gold()["a"])
    assert [tuple(f.shape[1:]) for f in metrics.vgg16_features(a, vgg16(), bgr=False)] == \
        [(48, 48, 64), (24, 24, 128), (12, 12, 256), (6, 6, 512), (3, 3, 512)]
    x = ops.frame_ingest(a, bgr=False).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        vgg16()(x)


# ---- end to end --------------------------------------------------------------------------------------
def test_lpips_end_to_end_on_the_golden():
    """The golden frames are R,G,B (bgr=False).  Against lpips64 on the SAME device taps, downloaded, so trunk
    parity (which has its own test) is not in the bound; the difference to the reference's forward is printed."""
    g = gold()
    da, db = to_dev(g["a"]), to_dev(g["b"], 5)
    lins = list(gold_lins())
    fa, fb = metrics.vgg16_features(da, vgg16(), bgr=False), metrics.vgg16_features(db, vgg16(), bgr=False)
    na, nb = [f.cpu().numpy() for f in fa], [f.cpu().numpy() for f in fb]
    want = L.lpips64(na, nb, [w.numpy() for w in lins])
    bound = np.stack([L.bound_layer(x, y, w.numpy()) for x, y, w in zip(na, nb, lins)])
    got = metrics.lpips(da, db, vgg16(), lins, bgr=False, per_layer=True)
    assert got.shape == (5, 2) and got.dtype == np.float64
    print("max |err| / bound per layer", (np.abs(got - want) / bound).max(axis=1))
    assert (np.abs(got - want) <= bound).all()
    total = metrics.lpips(da, db, vgg16(), lins, bgr=False)
    acc = np.zeros(2)
    for layer in got:
        acc = acc + layer
    assert total.shape == (2,) and total.dtype == np.float64 and np.array_equal(total, acc)
    assert metrics.lpips(da, da, vgg16(), lins, bgr=False).tolist() == [0.0, 0.0]
    assert np.array_equal(metrics.lpips_from_features(fa, fb, lins, per_layer=True), got)
    print("device vs reference, per layer, relative:", np.abs(got - g["ref_layers"]) / g["ref_layers"])
    print("device vs reference, total, relative:", np.abs(total - g["ref_total"]) / g["ref_total"])


@functools.lru_cache(maxsize=None)
def vgg19():
    return load_recipe(network.VGG19(), "vgg").to(DEV).eval()


def test_score_with_the_lpips_columns():
    """The stylised output of the full_64_b2 recipe, built as test_gpu_metrics.test_score_on_stylize_u8_output
    builds it."""
    gd = load_golden("full_64_b2")
    c = seeded_image(*map(int, gd["content_shape"]), int(gd["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, gd["style_shape"]), int(gd["seeds"][1])).to(DEV)
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = torch.bfloat16
    st = video.VideoStylizer(vc, vs, ada)
    st.set_style(s)
    cs = st.stylize_u8(c)  # u8 [2][64][64][3] B,G,R on the device
    cu, su = ops.frame_emit(c, bgr=True), ops.frame_emit(s, bgr=True)
    lins = list(gold_lins())
    old = metrics.score(cs, cu, su, bgr=True, vgg=vgg19())
    assert tuple(old) == metrics.SCORE_KEYS and len(old) == 8
    sc = metrics.score(cs, cu, su, bgr=True, vgg=vgg19(), lpips=(vgg16(), lins))
    assert tuple(sc) == metrics.SCORE_KEYS_LPIPS and len(sc) == 10
    for k, v in sc.items():
        print(k, v)
        assert v.shape == (2,) and v.dtype == np.float64 and not np.isnan(v).any(), k
    for k in metrics.SCORE_KEYS:
        np.testing.assert_array_equal(sc[k], old[k], err_msg=k)
    np.testing.assert_array_equal(sc["lpips_content"], metrics.lpips(cs, cu, vgg16(), lins))
    np.testing.assert_array_equal(sc["lpips_style"], metrics.lpips(cs, su, vgg16(), lins))
    assert (sc["lpips_content"] > 0).all() and (sc["lpips_style"] > 0).all()


# ---- error paths -------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    f = torch.zeros(1, 2, 2, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    nchw = torch.zeros(1, 2, 2, 64, device=DEV).permute(0, 3, 1, 2)  # an NCHW view of NHWC storage
    a = to_dev(gold()["a"])
    bad = [lambda: ops.lpips_layer(f.cpu(), f.cpu(), w.cpu()), lambda: ops.lpips_layer(f, f, w.cpu()),
           lambda: ops.lpips_layer(torch.zeros(1, 2, 2, 96, device=DEV), torch.zeros(1, 2, 2, 96, device=DEV),
                                   torch.ones(96, device=DEV)),
           lambda: ops.lpips_layer(torch.zeros(1, 2, 2, 576, device=DEV), torch.zeros(1, 2, 2, 576, device=DEV),
                                   torch.ones(576, device=DEV)),
           lambda: ops.lpips_layer(f, torch.zeros(1, 2, 3, 64, device=DEV), w),
           lambda: ops.lpips_layer(f, torch.zeros(2, 2, 2, 64, device=DEV), w),
           lambda: ops.lpips_layer(f.half(), f.half(), w.half()), lambda: ops.lpips_layer(f, f, w.double()),
           lambda: ops.lpips_layer(nchw, nchw, torch.ones(2, device=DEV)),
           lambda: ops.lpips_layer(f, f, torch.ones(128, device=DEV)), lambda: ops.lpips_layer(f, f, w.view(1, 64)),
           lambda: ops.lpips_layer(f.view(-1)[:128].view(2, 64), f.view(-1)[:128].view(2, 64), w),
           lambda: metrics.lpips(a, a, vgg16(), list(gold_lins())[:4]),
           lambda: metrics.lpips(a, a), lambda: metrics.lpips(a.cpu(), a.cpu(), vgg16(), list(gold_lins()))]
    for i, call in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError)):
            call()
            pytest.fail(f"call {i} did not raise")
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    work = torch.zeros(8, dtype=torch.float64, device=DEV)
    res = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    assert lib.mhada_lpips_layer_work(1, 4, 64) == 1 and lib.mhada_lpips_layer_work(2, 1600, 512) == 2 * 100
    assert lib.mhada_lpips_layer_work(1, 4, 96) == 0
    args = lambda fa=f.data_ptr(), wp=w.data_ptr(), C=64, nwork=8: (  # noqa: E731
        fa, f.data_ptr(), wp, 1, 4, C, work.data_ptr(), nwork, res.data_ptr(), st)
    assert lib.mhada_lpips_layer(*args(fa=None)) != 0
    assert "mhada_lpips_layer" in lib.mhada_last_error().decode()
    assert lib.mhada_lpips_layer(*args(wp=None)) != 0
    for C in (96, 576, 0):
        assert lib.mhada_lpips_layer(*args(C=C)) != 0
        assert "multiple of 64" in lib.mhada_last_error().decode()
    assert lib.mhada_lpips_layer(*args(fa=f.data_ptr() + 4)) != 0
    assert "aligned" in lib.mhada_last_error().decode()
    assert lib.mhada_lpips_layer(*args(nwork=0)) != 0
    assert "workspace" in lib.mhada_last_error().decode()
    assert res.item() == -1.0  # nothing was launched
    assert lib.mhada_lpips_layer(*args()) == 0 and res.item() == 0.0
