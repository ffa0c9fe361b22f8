"""The device metrics (csrc/metrics.hip, mhada_hip.metrics) against the fp64 restatements of
tests/metrics_ref.py: mhada_ssim_u8 to the fp64 truth of the reference's definition, mhada_hist_u8
exactly, the histogram metrics through the public module, the Gram distance on the HIP VGG19's
features, and metrics.score on the output of VideoStylizer.stylize_u8."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as R
import network
from conftest import load_golden
from mhada_hip import _lib, metrics, ops, video
from mhada_hip.recipe import load_recipe, seeded_image

DEV = "cuda"
# (1,1,1) minimal; (1,3,7) smaller than the window in both axes; (1,11,11) one window; (2,33,45) one past
# a 32-tile in each axis, two images; (1,70,37) three tile rows with halos crossing; (3,16,130) wide, 3W % 4 != 0
SHAPES = [(1, 1, 1), (1, 3, 7), (1, 11, 11), (2, 33, 45), (1, 70, 37), (3, 16, 130)]
SSIM_BOUND = 2.0 ** -22  # fp64 inside; the one fp32 rounding of a value in [-1, 1] is 2^-24
ids = lambda s: "x".join(map(str, s))  # noqa: E731


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
def ssim_pairs(shape):
    """name -> (a, b) u8 [B][H][W][3]: noise, noise against itself with a few values moved by one, flat
    200 against a 200 / 201 step, a column ramp against itself + 1 (images after the first shifted, so the
    images of a batch differ), flat 255 against 0."""
    B, H, W = shape
    g = np.random.default_rng(100 * H + W)
    noise = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    near = noise.copy()
    flip = g.random((B, H, W, 3)) < 0.1
    near[flip] = np.where(near[flip] < 255, near[flip] + 1, 254)
    flat = np.full((B, H, W, 3), 200, np.uint8)
    step = flat.copy()
    step[:, :, W // 2:] = 201
    for n in range(1, B):
        step[n, H // 2:] = 199
    col = np.round(np.linspace(100, 140, W)).astype(np.uint8)
    ramp = np.stack([np.broadcast_to((col + 7 * n)[None, :, None], (H, W, 3)) for n in range(B)]).astype(np.uint8)
    return {"noise": (noise, g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)), "near": (noise, near),
            "flat_step": (flat, step), "ramp": (ramp, (ramp + 1).astype(np.uint8)),
            "white_black": (np.full((B, H, W, 3), 255, np.uint8), np.zeros((B, H, W, 3), np.uint8))}


@functools.lru_cache(maxsize=None)
def ssim_truth(shape, name):
    return R.ssim64(*ssim_pairs(shape)[name])


@pytest.mark.parametrize("pad", [0, 5], ids=["tight", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_ssim_is_the_fp64_value_of_the_definition(shape, pad):
    for name, (a, b) in ssim_pairs(shape).items():
        got = ops.ssim_u8(to_dev(a, pad), to_dev(b, pad))
        assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0],)
        got = got.cpu().numpy().astype(np.float64)
        truth = ssim_truth(shape, name)
        print(shape, pad, name, "truth", truth, "|got - truth|", np.abs(got - truth))
        assert np.abs(got - truth).max() <= SSIM_BOUND, (name, got, truth)
        if pad:  # the 0xFF padding bytes are never read: the bits of the packed call
            assert np.array_equal(got, ops.ssim_u8(to_dev(a), to_dev(b)).cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_ssim_identity_symmetry_and_repeatability(shape):
    pairs = ssim_pairs(shape)
    for name in ("noise", "flat_step", "ramp"):
        x = to_dev(pairs[name][0])
        assert ops.ssim_u8(x, x).cpu().tolist() == [1.0] * shape[0], name
    for name, (a, b) in pairs.items():
        a, b = to_dev(a), to_dev(b, 5)
        ab = ops.ssim_u8(a, b)
        assert torch.equal(ab, ops.ssim_u8(b, a)), name
        assert torch.equal(ab, ops.ssim_u8(a, b)), name


def test_ssim_reductions():
    a, b = (to_dev(t) for t in ssim_pairs((3, 16, 130))["noise"])
    none = metrics.ssim(a, b, reduction="none")
    assert tuple(none.shape) == (3,) and torch.equal(none, ops.ssim_u8(a, b))
    mean = metrics.ssim(a, b)
    assert mean.dim() == 0 and mean.dtype == torch.float32 and torch.equal(mean, none.mean())
    one = metrics.ssim(a[0], b[0], reduction="none")  # a single [H][W][3] frame
    assert tuple(one.shape) == (1,) and one[0] == none[0]


# ---- histograms ----------------------------------------------------------------------------------
def check_hist(frames: np.ndarray, dev: torch.Tensor):
    B, H, W, _ = frames.shape
    planes = None
    for bgr in (True, False):
        got = ops.hist_u8(dev, bgr=bgr)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, 4, 256)
        got = got.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(got, R.hist_counts(frames, bgr))
        assert (got.sum(axis=2) == H * W).all()
        if planes is not None:  # the flag moves only the gray plane
            np.testing.assert_array_equal(got[:, :3], planes)
        planes = got[:, :3]


@pytest.mark.parametrize("pad", [0, 5], ids=["tight", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_hist_is_bincount_and_the_integer_gray_formula(shape, pad):
    pairs = ssim_pairs(shape)
    for frames in (pairs["noise"][0], pairs["ramp"][0]):
        check_hist(frames, to_dev(frames, pad, fill=0xA5))
    if shape == (2, 33, 45):  # R and B weighted differently: the flag must change the gray plane
        dev = to_dev(pairs["noise"][0])
        assert not torch.equal(ops.hist_u8(dev, bgr=True)[:, 3], ops.hist_u8(dev, bgr=False)[:, 3])


def test_hist_counts_are_full_width():
    frames = np.full((1, 300, 300, 3), 7, np.uint8)  # 90 000 in one bin: above 2^16
    check_hist(frames, to_dev(frames))
    assert int(ops.hist_u8(to_dev(frames))[0, 0, 7]) == 90000


def test_hist_reads_no_padding_and_no_guard_row():
    g = np.random.default_rng(4)
    frames = g.integers(0, 0xA5, (2, 5, 3, 3), dtype=np.uint8)  # no 0xA5 of its own
    dev = to_dev(frames, pad=16 - 9, fill=0xA5, guard_rows=1)
    assert dev.stride(1) == 16
    check_hist(frames, dev)
    assert int(ops.hist_u8(dev)[:, :, 0xA5].sum()) == 0


def test_hist_output_is_zeroed_by_every_call():
    frames = ssim_pairs((2, 33, 45))["noise"][0]
    dev = to_dev(frames)
    out = torch.full((2, 4, 256), 12345, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    for _ in range(2):
        rc = lib.mhada_hist_u8(dev.data_ptr(), 2, 33, 45, dev.stride(1), 1, out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        np.testing.assert_array_equal(out.cpu().numpy(), R.hist_counts(frames, True))


@pytest.mark.parametrize("shape", [(2, 33, 45), (3, 16, 130)], ids=ids)
def test_histogram_metrics_equal_the_host_restatements(shape):
    a, b = ssim_pairs(shape)["noise"]
    b = b // 3 + 40  # a narrower histogram: empty bins on one side
    da, db = to_dev(a), to_dev(b, 5)
    rel = lambda got, want: np.abs(got - want).max() <= 1e-12 * np.abs(want).max()  # noqa: E731
    assert rel(metrics.kl(da, db), R.kl(a, b)) and rel(metrics.kl(db, da), R.kl(b, a))
    assert metrics.kl(da, da).tolist() == [0.0] * shape[0]
    for bgr in (True, False):
        assert rel(metrics.moment(db, bgr), R.moment(b, bgr))
        assert rel(metrics.uniformity(db, bgr), R.uniformity(b, bgr))
        assert rel(metrics.entropy(db, bgr), R.entropy(b, bgr))
    assert metrics.kl(da, db).shape == metrics.moment(da).shape == (shape[0],)


# ---- Gram ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(64, 5, 7), (512, 2, 2), (128, 32, 32)], ids=["c64_hw35", "c512_hw4", "c128_hw1024"])
def test_gram_op_on_synthetic_features(C, H, W):
    B, K = 2, H * W
    feat = torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(C + K))  # >= 0, as after a ReLU
    got = ops.gram(feat.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, C, C)
    got = got.cpu().numpy().astype(np.float64)
    want = R.gram64(feat.numpy())
    # fp32 accumulation of K non-negative terms: |err| <= K 2^-24 sum, with a factor 2 of slack
    bound = K * 2.0 ** -23 * want + 1e-30
    print(C, K, "max |G - G64| / bound", (np.abs(got - want) / bound).max())
    assert (np.abs(got - want) <= bound).all()
    assert (np.abs(got - got.transpose(0, 2, 1)) <= bound).all()
    assert torch.equal(ops.gram(feat.to(DEV)), ops.gram(feat.to(DEV).view(B, K, C)))  # repeatable; [B][P][C] form


@functools.lru_cache(maxsize=None)
def vgg19():
    return load_recipe(network.VGG19(), "vgg").to(DEV).eval()


def test_gram_distance_end_to_end():
    """64 x 64: the smallest size at which relu5_1 is still 4 x 4.  The reference expression in fp64 on the
    CPU from the SAME device VGG features, so VGG parity (which has its own tests) is not in the bound:
    every Gram entry is within K 2^-23 (K <= 4096) of fp64, hence 1e-4 relative for the distance."""
    g = np.random.default_rng(12)
    a = g.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:64, 0:64]
    b = np.stack([np.stack([(3 * xx + n * 40) % 256, (2 * yy + 4 * xx) % 256, (yy * xx // 16) % 256], -1)
                  for n in range(2)]).astype(np.uint8)
    da, db = to_dev(a), to_dev(b, 5)
    fa, fb = metrics.vgg_features(da, vgg19()), metrics.vgg_features(db, vgg19())
    assert [tuple(f.shape[1:]) for f in fa] == [(64, 64, 64), (32, 32, 128), (16, 16, 256), (8, 8, 512), (4, 4, 512)]
    want = R.gram_loss64([f.cpu().numpy() for f in fa], [f.cpu().numpy() for f in fb])
    got = metrics.gram(da, db, vgg19())
    print("gram", got, "fp64 on the same features", want, "rel", np.abs(got - want) / want)
    assert got.shape == (2,) and (want > 0).all()
    assert (np.abs(got - want) <= 1e-4 * want).all()
    assert metrics.gram(da, da, vgg19()).tolist() == [0.0, 0.0]


# ---- score -----------------------------------------------------------------------------------------
def test_score_on_stylize_u8_output():
    """The smallest recipe of the video tests (tests/test_gpu_frame_emit.py): the 64^2 B2 golden inputs."""
    gold = load_golden("full_64_b2")
    c = seeded_image(*map(int, gold["content_shape"]), int(gold["seeds"][0])).to(DEV)
    s = seeded_image(*map(int, gold["style_shape"]), int(gold["seeds"][1])).to(DEV)
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = torch.bfloat16
    st = video.VideoStylizer(vc, vs, ada)
    st.set_style(s)
    cs = st.stylize_u8(c)  # u8 [2][64][64][3] B,G,R on the device
    cu, su = ops.frame_emit(c, bgr=True), ops.frame_emit(s, bgr=True)
    sc = metrics.score(cs, cu, su, bgr=True, vgg=vgg19())
    assert tuple(sc) == metrics.SCORE_KEYS and len(sc) == 8
    want = {"ssim_content": metrics.ssim(cs, cu, "none").cpu().numpy(), "kl_c": metrics.kl(cs, cu),
            "ssim_style": metrics.ssim(cs, su, "none").cpu().numpy(), "kl_s": metrics.kl(cs, su),
            "gram": metrics.gram(cs, su, vgg19()), "moment": metrics.moment(cs), "uniformity": metrics.uniformity(cs),
            "entropy": metrics.entropy(cs)}
    for k, v in sc.items():
        print(k, v)
        assert v.shape == (2,) and v.dtype == np.float64 and not np.isnan(v).any(), k
        np.testing.assert_array_equal(v, want[k].astype(np.float64), err_msg=k)
    assert ((sc["ssim_content"] >= -1) & (sc["ssim_content"] <= 1)).all()
    # the numbers are those of the downloaded frames
    h = cs.cpu().numpy()
    assert np.abs(sc["ssim_content"] - R.ssim64(h, cu.cpu().numpy())).max() <= SSIM_BOUND
    assert np.abs(sc["entropy"] - R.entropy(h)).max() <= 1e-12 * np.abs(sc["entropy"]).max()


# ---- error paths -----------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    a = torch.zeros(1, 5, 3, 3, dtype=torch.uint8, device=DEV)
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    short = buf.as_strided((1, 5, 3, 3), (40, 8, 3, 1))  # row_bytes 8 < 3W = 9
    bad = [lambda: ops.ssim_u8(a.cpu(), a.cpu()), lambda: ops.ssim_u8(a, a.cpu()), lambda: ops.hist_u8(a.cpu()),
           lambda: ops.ssim_u8(a.float(), a.float()), lambda: ops.hist_u8(a.int()),
           lambda: ops.ssim_u8(a, torch.zeros(1, 5, 4, 3, dtype=torch.uint8, device=DEV)),
           lambda: ops.ssim_u8(a, torch.zeros(2, 5, 3, 3, dtype=torch.uint8, device=DEV)),
           lambda: ops.ssim_u8(a, short), lambda: ops.hist_u8(short), lambda: ops.hist_u8(a[..., :2]),
           lambda: ops.gram(torch.zeros(1, 2, 2, 4, device=DEV).half()), lambda: ops.gram(torch.zeros(1, 2, 2, 3, device=DEV)),
           lambda: metrics.kl(a, a.cpu()), lambda: metrics.moment(a.float())]
    for i, call in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError)):
            call()
            pytest.fail(f"call {i} did not raise")
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.zeros(4, 256, dtype=torch.int32, device=DEV)
    assert lib.mhada_hist_u8(a.data_ptr(), 1, 5, 3, 8, 1, out.data_ptr(), st) != 0
    assert "row_bytes" in lib.mhada_last_error().decode()
    assert lib.mhada_hist_u8(None, 1, 5, 3, 9, 1, out.data_ptr(), st) != 0
    work = torch.zeros(8, dtype=torch.float64, device=DEV)
    res = torch.zeros(1, device=DEV)
    win = ops.ssim_window().data_ptr()
    assert lib.mhada_ssim_u8_work(1, 5, 3) == 3 and lib.mhada_ssim_u8_work(2, 33, 45) == 2 * 3 * 2 * 2
    assert lib.mhada_ssim_u8(a.data_ptr(), 9, a.data_ptr(), 8, 1, 5, 3, win, work.data_ptr(), 8, res.data_ptr(), st) != 0
    assert "row_bytes" in lib.mhada_last_error().decode()
    assert lib.mhada_ssim_u8(a.data_ptr(), 9, a.data_ptr(), 9, 1, 5, 3, None, work.data_ptr(), 8, res.data_ptr(), st) != 0
    assert lib.mhada_ssim_u8(a.data_ptr(), 9, a.data_ptr(), 9, 1, 5, 3, win, work.data_ptr(), 2, res.data_ptr(), st) != 0
    assert "workspace" in lib.mhada_last_error().decode()
    assert res.item() == 0.0 and int(out.sum()) == 0  # nothing was launched
