"""LPIPS without a GPU: network.VGG16's layout and loaders, the identity of LPIPS's ScalingLayer and the
ImageNet normalisation, the CPU forward, metrics.lpips_weights, and the fp64 restatement of
tests/lpips_ref.py tied to the reference's own forward through the golden (lpips_vgg16_48_b2.npz)."""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as L
import network
from conftest import load_golden
from mhada_hip import autograd_path, metrics

CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("lpips_vgg16_48_b2")


@functools.lru_cache(maxsize=None)
def golden_feats64():
    vgg = L.vgg16_kaiming()
    return tuple(tuple(L.nhwc(t) for t in L.vgg16_taps(vgg, L.scaling64(gold()[k]))) for k in ("a", "b"))


def lins():
    return [gold()[f"lin{k}"] for k in range(5)]


def test_vgg16_has_the_reference_layout():
    vgg = network.VGG16()
    want = {}
    for i, ci, co in CONVS:
        s = next(n for n, (a, b) in enumerate(SLICES, start=1) if a <= i < b)
        want[f"slice{s}.{i}.weight"] = (co, ci, 3, 3)
        want[f"slice{s}.{i}.bias"] = (co,)
    got = {k: tuple(v.shape) for k, v in vgg.state_dict().items()}
    assert len(want) == 26 and got == want
    assert all(not p.requires_grad for p in vgg.parameters())
    for s, (a, b) in enumerate(SLICES, start=1):  # pools at 4, 9, 16, 23; ReLU wherever no conv or pool is
        seq = getattr(vgg, f"slice{s}")
        assert [n for n, _ in seq.named_children()] == [str(i) for i in range(a, b)]
        for i in range(a, b):
            kind = torch.nn.Conv2d if i in {c[0] for c in CONVS} else torch.nn.MaxPool2d if i in (4, 9, 16, 23) \
                else torch.nn.ReLU
            assert isinstance(getattr(seq, str(i)), kind), i
    assert "VGG16" in network.__all__


def test_vgg16_loads_torchvision_feature_weights(tmp_path):
    vgg = network.VGG16()
    g = torch.Generator().manual_seed(3)
    tv = {}
    for name, p in vgg.named_parameters():
        s, i, t = name.split(".")
        tv[f"features.{i}.{t}"] = torch.randn(p.shape, generator=g)
    tv["classifier.0.weight"] = torch.randn(4096, 25088 // 64, generator=g)  # ignored
    torch.save(tv, tmp_path / "vgg16-397923af.pth")
    vgg.load_torchvision_features(str(tmp_path / "vgg16-397923af.pth"))
    for name, p in vgg.named_parameters():
        s, i, t = name.split(".")
        assert torch.equal(p, tv[f"features.{i}.{t}"])
        assert not p.requires_grad
    del tv["features.28.bias"]
    with pytest.raises(KeyError):
        network.VGG16().load_torchvision_features(tv)


def test_scaling_layer_is_the_imagenet_normalisation():
    """(u / 127.5 - 1 - shift) / scale == (u / 255 - mean) / std for every level and channel."""
    u = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None, None], (1, 256, 1, 3))
    want = L.scaling64(u)  # [1][3][256][1]
    x = torch.from_numpy(np.ascontiguousarray(u.transpose(0, 3, 1, 2))).double()
    # imagenet_normalize works in fp32 by design (x.float()), so the identity is checked on its expression in fp64,
    # relative to the values' scale (next to a zero crossing the two forms cancel differently) ...
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64).view(-1, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64).view(-1, 1, 1)
    expr = ((x / 255.0 - mean) / std).numpy()
    assert (np.abs(expr - want) <= 1e-15 * np.maximum(np.abs(want), 1.0)).all()
    # ... and the function the CPU forward calls is that expression in fp32 (four roundings of values up to 2.7)
    got = autograd_path.imagenet_normalize(x).numpy()
    assert np.abs(got - want).max() <= 2.0 ** -21 * np.abs(want).max()


@pytest.mark.parametrize("H,W", [(48, 48), (32, 40)])
def test_vgg16_cpu_forward_names_shapes_and_values(H, W):
    vgg = L.vgg16_kaiming()
    u = np.random.default_rng(H + W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    x = torch.from_numpy(u).permute(0, 3, 1, 2).float()  # fp32 NCHW in [0, 255], R,G,B planes
    with torch.no_grad():
        feats = vgg(x)
    assert tuple(feats) == L.TAPS
    want = L.vgg16_taps(vgg, autograd_path.imagenet_normalize(x), torch.float32)
    truth = L.vgg16_taps(vgg, L.scaling64(u))
    for s, (name, c) in enumerate(zip(L.TAPS, L.CHNS)):
        assert tuple(feats[name].shape) == (2, c, H >> s, W >> s), name
        assert torch.equal(feats[name], want[s]), name  # the same aten ops on the same input
        rel = ((feats[name].double() - truth[s]).norm() / truth[s].norm()).item()
        assert rel < 1e-5, (name, rel)  # and the ScalingLayer form in fp64


def test_lpips_weights_loader(tmp_path):
    g = torch.Generator().manual_seed(11)
    sd = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for k, c in enumerate(L.CHNS)}
    torch.save(sd, tmp_path / "vgg.pth")
    got = metrics.lpips_weights(str(tmp_path / "vgg.pth"))
    assert len(got) == 5
    for k, (w, c) in enumerate(zip(got, L.CHNS)):
        assert w.dtype == torch.float32 and tuple(w.shape) == (c,) and w.is_contiguous()
        assert torch.equal(w, sd[f"lin{k}.model.1.weight"].reshape(-1))
    missing = {k: v for k, v in sd.items() if not k.startswith("lin3")}
    with pytest.raises((KeyError, ValueError)):
        metrics.lpips_weights(missing)
    wrong = dict(sd)
    wrong["lin4.model.1.weight"] = torch.rand(1, 256, 1, 1, generator=g)
    with pytest.raises((KeyError, ValueError)):
        metrics.lpips_weights(wrong)
    flat = dict(sd)
    flat["lin0.model.1.weight"] = torch.rand(64, generator=g)
    with pytest.raises((KeyError, ValueError)):
        metrics.lpips_weights(flat)
    shipped = {f"lin{k}.model.1.weight": torch.from_numpy(w).view(1, -1, 1, 1) for k, w in enumerate(lins())}
    for w, want in zip(metrics.lpips_weights(shipped), lins()):
        assert np.array_equal(w.numpy().view(np.uint32), want.view(np.uint32))
    assert metrics.SCORE_KEYS_LPIPS == ("lpips_content", "ssim_content", "kl_c", "lpips_style", "ssim_style", "kl_s",
                                        "gram", "moment", "uniformity", "entropy")
    assert len(metrics.SCORE_KEYS) == 8 and set(metrics.SCORE_KEYS) < set(metrics.SCORE_KEYS_LPIPS)


def test_restatement_matches_the_reference_forward():
    """lpips64 on fp64 aten features against the reference's own fp32 forward, per layer and image, within 4 x
    the difference the golden maker measured between the two (the factor: aten's conv summation order
    changes with the thread count between machines)."""
    g = gold()
    assert g["a"].shape == g["b"].shape == (2, 48, 48, 3) and g["a"].dtype == np.uint8
    assert np.array_equal(g["b"], L.golden_b())
    fa, fb = golden_feats64()
    got = L.lpips64(fa, fb, lins())
    assert got.shape == g["ref_layers"].shape == (5, 2)
    rel = np.abs(got - g["ref_layers"]) / g["ref_layers"]
    print("restatement vs reference, relative:", rel.max(axis=1), "allowed", 4 * g["ref_vs_fp64"])
    assert (rel <= 4 * g["ref_vs_fp64"][:, None]).all()
    total = np.zeros(2)
    for layer in g["ref_layers"]:
        total = total + layer
    assert np.abs(total - g["ref_total"]).max() <= 2.0 ** -22 * g["ref_total"].max()  # the reference's fp32 additions


def test_bound_layer_is_positive_and_zero_only_for_zero_rows():
    fa, fb = golden_feats64()
    for a, b, w in zip(fa, fb, lins()):
        bd = L.bound_layer(a, b, w)
        assert bd.shape == (2,) and np.isfinite(bd).all() and (bd > 0).all()
        assert (bd < 0.1 * L.lpips_layer64(a, b, w)).all()  # a bound well below the value it guards
    z = np.zeros((2, 3, 3, 64))
    one = z.copy()
    one[1, 0, 0, 5] = 2.0
    w = np.abs(lins()[0])
    assert L.bound_layer(z, z, w).tolist() == [0.0, 0.0]
    bd = L.bound_layer(one, z, w)
    assert bd[0] == 0.0 and bd[1] > 0.0
    assert L.lpips_layer64(z, z, w).tolist() == [0.0, 0.0]  # 0 / (0 + 1e-10): no NaN
