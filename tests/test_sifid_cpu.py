"""SIFID without a GPU: the restatement of tests/inception_ref.py against the golden that the reference's own
SIFID package produced (tests/golden/make_sifid_goldens.py), network.InceptionV3's interface on the CPU
(aten), the input tables and the host finaliser ``metrics.frechet_from_moments``.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import inception_ref as R
import network
from mhada_hip import metrics

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(os.path.join(GOLD, "sifid_inception_139x123.npz")))


@functools.lru_cache(maxsize=None)
def recipe():
    return R.recipe()


def nchw(img_u8, levels):
    return torch.from_numpy(levels[img_u8.astype(np.int64)]).permute(2, 0, 1)[None]


@functools.lru_cache(maxsize=None)
def taps32():
    """fp32 restatement taps of both PNG images at the reference's scale."""
    g = gold()
    net = R.build_torchvision(recipe())
    return [R.trunk(net, nchw(g[k], g["levels_reference"])) for k in ("a", "b")]


def test_restatement_features_are_the_references():
    g = gold()
    got = np.stack([t[3][0].permute(1, 2, 0).numpy() for t in taps32()])
    # the same aten kernels on the same operands; allow thread-count summation-order differences at the
    # reference's own fp32 error against fp64
    assert R.norm_rel(got, g["ref_feat_2048"]) <= 4 * g["ref_vs_fp64_feat"][3]


def test_restatement_d2_within_the_references_own_error():
    g = gold()
    for i, dims in enumerate(R.DIMS):
        d2 = R.fd64(R.rows(taps32()[0][i]), R.rows(taps32()[1][i]))
        bound = 4 * g["ref_vs_fp64_d2"][i] + 4 * g["sqrtm_vs_nuclear"][i]
        print(f"dims {dims}: restatement {d2:.9g} reference {g['ref_d2'][i]:.9g} fp64 {g['fd64'][i]:.9g} bound {bound:.3e}")
        assert abs(d2 - g["ref_d2"][i]) <= bound * g["ref_d2"][i]
        assert abs(d2 - g["fd64"][i]) <= bound * g["fd64"][i]


def test_golden_conditions():
    g = gold()
    assert (g["ref_d2"] >= 1e-3 * g["tr_s"].sum(axis=1)).all()
    assert (g["sqrtm_imag"] <= 1e-3).all()
    assert g["ref_feat_2048"].shape == (2, 3, 2, 2048)


def test_state_dict_keys_are_the_references():
    with open(os.path.join(GOLD, "state_dict_keys_inception.json")) as f:
        want = json.load(f)
    assert sorted(network.InceptionV3().state_dict().keys()) == want
    assert len([k for k in want if k.endswith("conv.weight")]) == 94
    m0 = network.InceptionV3([0])
    assert sorted(m0.state_dict().keys()) == [k for k in want if k.startswith("blocks.0.")]
    assert len(m0.blocks) == 1  # truncation: dims 64 builds three convs


def test_load_torchvision_maps_ignores_and_rejects():
    sd = recipe()
    m = network.InceptionV3()
    extra = dict(sd)
    extra.update({"AuxLogits.conv0.conv.weight": torch.zeros(1), "fc.weight": torch.zeros(1), "fc.bias": torch.zeros(1),
                  "transform_input": torch.zeros(1)})
    m.load_torchvision(extra)
    own = m.state_dict()
    assert torch.equal(own["blocks.0.0.conv.weight"], sd["Conv2d_1a_3x3.conv.weight"])
    assert torch.equal(own["blocks.1.2.bn.running_var"], sd["Conv2d_4a_3x3.bn.running_var"])
    assert torch.equal(own["blocks.2.5.branch7x7dbl_3.conv.weight"], sd["Mixed_6b.branch7x7dbl_3.conv.weight"])
    assert torch.equal(own["blocks.3.2.branch3x3dbl_3b.bn.bias"], sd["Mixed_7c.branch3x3dbl_3b.bn.bias"])
    no_nbt = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}  # the old checkpoint's form
    network.InceptionV3().load_torchvision(no_nbt)
    network.InceptionV3([1]).load_torchvision(sd)  # layers of blocks that were not built are skipped
    missing = dict(sd)
    del missing["Mixed_6c.branch7x7_2.bn.running_mean"]
    with pytest.raises(KeyError):
        network.InceptionV3().load_torchvision(missing)
    with pytest.raises(KeyError):
        network.InceptionV3().load_torchvision(dict(sd, **{"Mixed_8a.conv.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError):
        network.InceptionV3().load_torchvision(dict(sd, **{"Mixed_5b.bogus.weight": torch.zeros(1)}))


def test_cpu_forward_is_the_restatement():
    m = network.InceptionV3([0, 1, 2, 3])
    m.load_torchvision(recipe())
    g = gold()
    x = nchw(g["b"], g["levels_reference"])
    with torch.no_grad():
        got = m(x)
    for a, b in zip(got, taps32()[1]):
        assert a.shape == b.shape and R.norm_rel(a.numpy(), b.numpy()) <= 1e-5
    assert [tuple(t.shape[1:]) for t in got] == [(64, 67, 59), (192, 31, 27), (768, 7, 6), (2048, 3, 2)]
    with torch.no_grad():
        only = network.InceptionV3([1])
        only.load_torchvision(recipe())
        assert torch.equal(only(x)[0], got[1])


def test_input_levels_are_the_references_bits():
    g = gold()
    for scale in ("reference", "unit"):
        assert np.array_equal(metrics.sifid_input_levels(scale).view(np.int32), g[f"levels_{scale}"].view(np.int32))
    assert metrics.sifid_input_levels("reference").max() < 1 / 254  # the PNG double-scale finding


def _moments(x):
    mu, _, xc = R.moments64(x)
    return mu, float((xc * xc).sum()), xc


def test_frechet_forms_agree_and_match_sqrtm():
    from scipy import linalg
    rng = np.random.default_rng(3)
    for C, n1, n2 in ((8, 40, 40), (12, 30, 57), (5, 6, 9)):
        x1 = rng.standard_normal((n1, C)) @ rng.standard_normal((C, C)) + rng.standard_normal(C)
        x2 = rng.standard_normal((n2, C)) @ rng.standard_normal((C, C))
        (m1, q1, c1), (m2, q2, c2) = _moments(x1), _moments(x2)
        cross = metrics.frechet_from_moments(m1, q1, n1, m2, q2, n2, cross=c1 @ c2.T)
        cov = metrics.frechet_from_moments(m1, q1, n1, m2, q2, n2, scatter1=c1.T @ c1, scatter2=c2.T @ c2)
        s1, s2 = np.cov(x1, rowvar=False), np.cov(x2, rowvar=False)
        ref = (m1 - m2) @ (m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(linalg.sqrtm(s1 @ s2)).real
        assert abs(cross - cov) <= 1e-10 * ref and abs(cross - ref) <= 1e-10 * ref and abs(cov - ref) <= 1e-10 * ref
        assert abs(cross - R.fd64(x1, x2)) <= 1e-12 * ref


def test_frechet_of_identical_sets_is_zero():
    rng = np.random.default_rng(4)
    for n, C in ((6, 64), (50, 7)):
        x = rng.standard_normal((n, C)) * 3 + 1
        m, q, c = _moments(x)
        tr = q / (n - 1)
        assert abs(metrics.frechet_from_moments(m, q, n, m, q, n, cross=c @ c.T)) <= 1e-9 * tr
        if n >= C:
            assert abs(metrics.frechet_from_moments(m, q, n, m, q, n, scatter1=c.T @ c, scatter2=c.T @ c)) <= 1e-9 * tr


def test_errors():
    m, q = np.zeros(4), 1.0
    with pytest.raises(ValueError):
        metrics.frechet_from_moments(m, q, 1, m, q, 5, cross=np.zeros((1, 5)))  # fewer than 2 positions
    with pytest.raises(ValueError):
        metrics.frechet_from_moments(m, q, 5, m, q, 5)
    with pytest.raises(ValueError):
        metrics.sifid_input_levels("jpeg")
    with pytest.raises(NotImplementedError):
        network.InceptionV3(resize_input=True)
    with pytest.raises(ValueError):
        network.InceptionV3([4])
    inc = network.InceptionV3([0])
    u8 = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        metrics.sifid(u8, u8, inc, dims=100)
    with pytest.raises(ValueError):
        metrics.sifid(u8, u8, inc, dims=2048)  # built up to block 0 only
    with pytest.raises(ValueError):
        metrics.sifid(u8, u8, inc, dims=64, input_scale="jpeg")
    with pytest.raises(ValueError):
        metrics.sifid(u8, u8, None)
    with pytest.raises(RuntimeError):
        metrics.sifid(u8, u8, inc, dims=64)  # CPU frames: no host fallback


def test_score_keys_without_sifid_are_unchanged():
    assert metrics.SCORE_KEYS == ("ssim_content", "kl_c", "ssim_style", "kl_s", "gram", "moment", "uniformity", "entropy")
    assert metrics.SCORE_KEYS_LPIPS == ("lpips_content", "ssim_content", "kl_c", "lpips_style", "ssim_style", "kl_s", "gram",
                                        "moment", "uniformity", "entropy")
    assert metrics.SCORE_KEYS_FULL == ("lpips_content", "ssim_content", "sifid_content", "kl_c", "lpips_style", "ssim_style",
                                       "sifid_style", "kl_s", "gram", "moment", "uniformity", "entropy")
    assert tuple(k for k in metrics.SCORE_KEYS_FULL if "sifid" not in k) == metrics.SCORE_KEYS_LPIPS
    assert tuple(k for k in metrics.SCORE_KEYS_LPIPS if "lpips" not in k) == metrics.SCORE_KEYS
