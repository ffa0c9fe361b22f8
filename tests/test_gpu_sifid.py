"""SIFID on the device: the HIP InceptionV3 trunk, the fp64 moment kernels, metrics.sifid and score.

The yardstick is the fp64 restatement of tests/inception_ref.py on the recipe weights, and the golden that the
reference's own SIFID package produced on the same weights and images (tests/golden/make_sifid_goldens.py).
Every device bound is 4 x the reference's own fp32 error against fp64 recorded there (``ref_vs_fp64_*``):
the device trunk and aten are both fp32 chains of the same length and differ only in summation order.

Measured on an MI355X.  Trunk taps, norm-relative error against fp64, image a / b (the reference's own): dims 64
4.57e-7 / 4.67e-7 (5.09e-5), 192 4.74e-7 / 4.97e-7 (3.30e-5), 768 8.38e-7 / 8.18e-7 (7.95e-6), 2048 1.08e-6 / 1.09e-6
(5.92e-6).  d^2, relative error against fd64 (bound = 4 x the reference's own): reference scale dims 64 3.15e-8
(3.77e-5), 192 5.03e-8 (1.74e-6), 768 3.16e-7 (6.40e-6), 2048 1.66e-6 (3.43e-4); unit scale 2048 1.57e-6 (7.70e-5), 64
1.26e-7 (4.10e-6).  The first conv is the direct fp64 kernel (DESIGN.md 3a "SIFID", the stem); with an fp32 stem the
trunk was as far from fp64 as aten and the d^2 checks at dims 192 and 768 failed (4.78e-6, 2.49e-5).
"""
import functools
import os

import numpy as np
import pytest
import torch

import inception_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if torch.cuda.is_available():
    import network
    from mhada_hip import metrics, ops
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(os.path.join(GOLD, "sifid_inception_139x123.npz")))


@functools.lru_cache(maxsize=None)
def recipe():
    return R.recipe()


@functools.lru_cache(maxsize=None)
def inception():
    m = network.InceptionV3([0, 1, 2, 3])
    m.load_torchvision(recipe())
    return m.to(DEV)


def nchw(img_u8, levels):
    return torch.from_numpy(levels[img_u8.astype(np.int64)]).permute(2, 0, 1)[None]


@functools.lru_cache(maxsize=None)
def taps64(scale):
    """fp64 restatement taps of both images: PNG bytes at the reference's scale, decoded JPEG bytes at unit."""
    g = gold()
    net = R.build_torchvision(recipe(), torch.float64)
    keys = ("a", "b") if scale == "reference" else ("a_jpg", "b_jpg")
    return [R.trunk(net, nchw(g[k], g[f"levels_{scale}"]).double()) for k in keys]


def frames(scale, bgr=True):
    g = gold()
    keys = ("a", "b") if scale == "reference" else ("a_jpg", "b_jpg")
    return [torch.from_numpy(np.ascontiguousarray(g[k][..., ::-1] if bgr else g[k]))[None].to(DEV) for k in keys]


@functools.lru_cache(maxsize=None)
def device_taps():
    g = gold()
    x = torch.cat([nchw(g[k], g["levels_reference"]) for k in ("a", "b")]).to(DEV)  # B = 2
    with torch.no_grad():
        return [t.cpu() for t in inception()(x)]


@pytest.mark.parametrize("i", range(4), ids=[f"dims{d}" for d in R.DIMS])
def test_trunk_taps_against_fp64(i):
    g = gold()
    got = device_taps()[i]
    assert torch.isfinite(got).all()
    for b in range(2):
        ref = taps64("reference")[b][i][0]
        assert got[b].shape == ref.shape
        err = R.norm_rel(got[b].numpy(), ref.numpy())
        print(f"dims {R.DIMS[i]} image {b}: norm-relative error {err:.3e}, reference's own {g['ref_vs_fp64_feat'][i]:.3e}")
        assert err <= 4 * g["ref_vs_fp64_feat"][i]


def test_trunk_rejects_gradients_and_truncates():
    x = torch.rand(1, 3, 40, 40, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        inception()(x)
    m0 = network.InceptionV3([0])
    m0.load_torchvision(recipe())
    m0 = m0.to(DEV)
    g = gold()
    xa = nchw(g["a"], g["levels_reference"]).to(DEV)
    with torch.no_grad():
        assert torch.equal(m0(xa)[0].cpu(), device_taps()[0][:1])  # batch-invariant bits, three convs only


@pytest.mark.parametrize("i", (0, 2, 3), ids=["dims64", "dims768", "dims2048"])
def test_moment_kernels_against_numpy(i):
    f = device_taps()[i]
    x1, x2 = (f[b].permute(1, 2, 0).reshape(-1, f.shape[1]).contiguous() for b in range(2))
    d1, d2 = x1.to(DEV), x2.to(DEV)
    (m1, q1), (m2, q2) = ops.sifid_stats(d1), ops.sifid_stats(d2)
    mu1, _, c1 = R.moments64(x1.double().numpy())
    mu2, _, c2 = R.moments64(x2.double().numpy())

    def close(got, ref):
        return np.linalg.norm(got.cpu().numpy() - ref) <= 1e-12 * np.linalg.norm(ref)

    assert close(m1, mu1) and close(m2, mu2)
    assert close(q1, (c1 * c1).sum(axis=0)) and close(q2, (c2 * c2).sum(axis=0))
    cross = ops.sifid_cross(d1, m1, d2[:-3], m2)  # n1 != n2; the centring uses the mean handed in
    assert close(cross, c1 @ (x2[:-3].double().numpy() - m2.cpu().numpy()).T)
    again = [ops.sifid_stats(d1), ops.sifid_cross(d1, m1, d2[:-3], m2)]
    assert torch.equal(again[0][0], m1) and torch.equal(again[0][1], q1) and torch.equal(again[1], cross)
    if x1.shape[0] >= x1.shape[1]:
        cov = ops.sifid_cov(d1, m1)
        assert close(cov, c1.T @ c1)
        assert torch.equal(ops.sifid_cov(d1, m1), cov)


@pytest.mark.parametrize("scale,dims", [("reference", 64), ("reference", 192), ("reference", 768), ("reference", 2048),
                                        ("unit", 2048), ("unit", 64)])
def test_sifid_against_fp64_and_the_reference(scale, dims):
    g = gold()
    if scale == "reference":
        i = R.DIMS.index(dims)
        fd64, ref, own = g["fd64"][i], g["ref_d2"][i], g["ref_vs_fp64_d2"][i]
    else:
        i = (2048, 64).index(dims)
        fd64, ref, own = g["fd64_unit"][i], g["ref_d2_unit"][i], g["ref_vs_fp64_d2_unit"][i]
    a, b = frames(scale)
    got = metrics.sifid(a, b, inception(), dims=dims, input_scale=scale)
    assert got.shape == (1,) and got.dtype == np.float64
    blk = R.DIMS.index(dims)
    assert abs(R.fd64(R.rows(taps64(scale)[0][blk]), R.rows(taps64(scale)[1][blk])) - fd64) <= 1e-9 * fd64
    print(f"{scale} dims {dims}: device {got[0]:.9g} fp64 {fd64:.9g} reference {ref:.9g}; relative error "
          f"{abs(got[0] - fd64) / fd64:.3e} (vs reference {abs(got[0] - ref) / ref:.3e}), bound {4 * own:.3e}")
    assert abs(got[0] - fd64) <= 4 * own * fd64
    assert abs(got[0] - ref) <= 4 * own * ref


@pytest.mark.parametrize("dims", (64, 2048))
def test_sifid_of_identical_frames_is_zero(dims):
    a, _ = frames("reference")
    got = metrics.sifid(a, a, inception(), dims=dims)
    tr = gold()["tr_s"][R.DIMS.index(dims)][0]
    print(f"dims {dims}: sifid(a, a) = {got[0]:.3e}, tr S = {tr:.6g}")
    assert abs(got[0]) <= 1e-9 * tr


def test_sifid_layouts_batch_and_sizes():
    a, b = frames("reference")
    base = metrics.sifid(a, b, inception(), dims=768)
    a_rgb, b_rgb = frames("reference", bgr=False)
    assert np.array_equal(metrics.sifid(a_rgb, b_rgb, inception(), dims=768, bgr=False), base)
    H, W = a.shape[1:3]
    padded = torch.zeros(1, H, W + 5, 3, dtype=torch.uint8, device=DEV)
    padded[:, :, :W] = a
    assert np.array_equal(metrics.sifid(padded[:, :, :W], b, inception(), dims=768), base)
    both = metrics.sifid(torch.cat([a, b]), torch.cat([b, b]), inception(), dims=768)  # B = 2
    assert both[0] == base[0] and abs(both[1]) <= 1e-9 * gold()["tr_s"][2][1]
    small = metrics.sifid(a[:, :100, :90], b, inception(), dims=768)  # n1 != n2
    assert np.isfinite(small).all() and small[0] > 0
    with pytest.raises(ValueError):
        metrics.sifid(a[:, :75, :75], b, inception(), dims=2048)  # a 1 x 1 map: fewer than 2 positions


def test_score_full_row():
    from lpips_ref import kaiming_state_dict
    a, b = frames("reference")
    vgg = network.VGG19()
    vgg16 = network.VGG16()
    vgg16.load_state_dict(kaiming_state_dict(vgg16))
    lins = [torch.rand(c) for c in (64, 128, 256, 512, 512)]
    vgg, vgg16 = vgg.to(DEV).eval(), vgg16.to(DEV).eval()
    content = torch.flip(a, dims=(2,)).contiguous()
    plain = metrics.score(a, content, b, vgg=vgg)
    assert tuple(plain) == metrics.SCORE_KEYS
    row = metrics.score(a, content, b, vgg=vgg, lpips=(vgg16, lins), sifid=inception())
    assert tuple(row) == metrics.SCORE_KEYS_FULL
    assert all(v.shape == (1,) and v.dtype == np.float64 for v in row.values())
    assert np.array_equal(row["sifid_style"], metrics.sifid(a, b, inception()))
    assert np.array_equal(row["sifid_content"], metrics.sifid(a, content, inception()))
    assert all(np.array_equal(row[k], plain[k]) for k in metrics.SCORE_KEYS)
    only = metrics.score(a, content, b, vgg=vgg, sifid=inception())
    assert tuple(only) == tuple(k for k in metrics.SCORE_KEYS_FULL if "lpips" not in k)
    with pytest.raises(RuntimeError):
        metrics.score(a.cpu(), content.cpu(), b.cpu(), vgg=vgg, sifid=inception())
