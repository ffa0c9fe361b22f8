"""The metric restatements (tests/metrics_ref.py) against the reference's own expressions, the SSIM
finding (the reference's fp32 recipe is rounding noise on smooth images), and the host finalisers of
mhada_hip.metrics against the restatements.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as R
from mhada_hip import metrics, ops

CASES = {"flat_step": R.case_flat_step, "ramp": R.case_ramp, "noise": R.case_noise}


def literal_ssim(a, b, dtype):
    """SSIMMetric.__init__ + forward (eval.py:180-223, reduction "none") as written, the window built in
    fp32 and everything after it in ``dtype``."""
    window_size, channel, sigma = 11, 3, 1.5
    _1D = torch.linspace(-(window_size // 2), window_size // 2, window_size)
    gauss = torch.exp(-(_1D ** 2) / (2 * sigma ** 2))
    gauss = gauss / gauss.sum()
    _2D = gauss[:, None] @ gauss[None, :]
    kernel = _2D.expand(channel, 1, window_size, window_size).contiguous().to(dtype)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    # cv2_to_tensor's ToTensor: HWC -> CHW, contiguous
    img1 = torch.from_numpy(a).permute(0, 3, 1, 2).contiguous().to(dtype)
    img2 = torch.from_numpy(b).permute(0, 3, 1, 2).contiguous().to(dtype)
    mu1 = F.conv2d(img1, kernel, padding=window_size // 2, groups=channel)
    mu2 = F.conv2d(img2, kernel, padding=window_size // 2, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, kernel, padding=window_size // 2, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, kernel, padding=window_size // 2, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, kernel, padding=window_size // 2, groups=channel) - mu1_mu2
    num = (2 * mu1_mu2 + C1) * (2 * sigma12 + C2)
    den = (mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2)
    return (num / den).mean(dim=[2, 3]).mean(dim=1).double().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_ssim64_is_the_reference_expression_in_fp64(case):
    a, b = CASES[case]()
    got, want = R.ssim64(a, b), literal_ssim(a, b, torch.float64)
    print(case, got, want, np.abs(got - want))
    assert np.abs(got - want).max() <= 1e-12
    # the torch-free tap-by-tap sum is the same number up to the definition's conditioning: on flat
    # regions var = E[x^2] - E[x]^2 is ~1e-8 of its operands, so an fp64 summation-order difference
    # (typically sqrt(121) * 2^-53 * 4e4 ~ 5e-11 in a moment) is ~1e-8 of var + C2 there.  It is
    # held to the bound the device kernel, a third summation order, is held to.
    taps = R.ssim64(a, b, blur=R._blur_taps)
    print(case, "tap-by-tap", np.abs(taps - want))
    assert np.abs(taps - want).max() <= 2.0 ** -22


def test_window_is_the_reference_window_and_does_not_sum_to_one():
    w = R.window_f32()
    assert w.dtype == np.float32 and w.shape == (11, 11)
    assert np.array_equal(w, ops.ssim_window().numpy())
    # the normalisation error the flat-region variance is made of
    assert 1e-9 < abs(w.astype(np.float64).sum() - 1.0) < 1e-6


def test_reference_fp32_ssim_is_noise_on_smooth_images():
    """The finding DESIGN.md records: SSIMMetric feeds [0, 255] images to C2 = 0.03^2 and forms
    E[x^2] - E[x]^2 in fp32; on smooth images that difference is rounding noise larger than C2."""
    a, b = R.case_flat_step()
    t64, t32 = literal_ssim(a, b, torch.float64)[0], literal_ssim(a, b, torch.float32)[0]
    print("flat 200 vs 200/201 step 40x40: fp64", t64, "fp32", t32)
    assert abs(t32 - t64) > 0.5
    assert -1.0 <= t64 <= 1.0
    a, b = R.case_ramp()
    r64, r32 = literal_ssim(a, b, torch.float64)[0], literal_ssim(a, b, torch.float32)[0]
    print("ramp 100..140 vs +1 64x64: fp64", r64, "fp32", r32)
    assert abs(r32 - r64) > 1e-5
    a, b = R.case_noise()
    n64, n32 = literal_ssim(a, b, torch.float64)[0], literal_ssim(a, b, torch.float32)[0]
    print("u8 noise 33x45: fp64", n64, "fp32", n32)
    assert abs(n32 - n64) < 1e-6  # textured images hide it


def test_kl_is_scipy_entropy():
    scipy_stats = pytest.importorskip("scipy.stats")
    g = np.random.default_rng(3)
    for _ in range(5):
        p, q = g.integers(1, 5000, 256), g.integers(1, 5000, 256)
        want = scipy_stats.entropy(p, q)
        assert abs(R.entropy_pq(p, q) - want) <= 1e-12 * max(1.0, abs(want))
    ca, cb = g.integers(0, 900, (3, 256)), g.integers(0, 900, (3, 256))
    want = sum(scipy_stats.entropy(ca[i] + 1, cb[i] + 1) for i in range(3)).item() / 3.0
    assert abs(R.kl_counts(ca, cb) - want) <= 1e-12 * abs(want)
    assert abs(metrics.kl_from_counts(ca, cb) - want) <= 1e-12 * abs(want)


def eval_py_gray_metrics(img_gray):
    """nth_order_moment, uniformity, average_entropy (eval.py:111-164) from the gray image on."""
    hist = np.bincount(img_gray.flatten(), minlength=256) + 1
    hist_p = hist / np.sum(hist)
    uniformity = 0.0
    entropy = 0.0
    for i in range(256):
        uniformity += hist_p[i] ** 2
        if hist_p[i] > 0:
            entropy -= hist_p[i] * np.log2(hist_p[i])
    hist = hist / 255.0
    hist_mean = np.mean(hist)
    nth_moment = 0.0
    for i in range(256):
        nth_moment += ((hist[i] - hist_mean) ** 2) * hist_p[i]
    return nth_moment, uniformity, entropy


def test_gray_metrics_are_the_reference_loops():
    g = np.random.default_rng(5)
    frames = g.integers(0, 256, (2, 19, 23, 3), dtype=np.uint8)
    frames[1, :, :12] = 40  # a peaked histogram
    for bgr in (True, False):
        gray = R.gray_u8(frames, bgr)
        counts = R.hist_counts(frames, bgr)
        for n in range(2):
            m, u, e = eval_py_gray_metrics(gray[n])
            for got, want in ((R.moment(frames, bgr)[n], m), (R.uniformity(frames, bgr)[n], u),
                              (R.entropy(frames, bgr)[n], e),
                              (metrics.moment_from_counts(counts[n, 3]), m),
                              (metrics.uniformity_from_counts(counts[n, 3]), u),
                              (metrics.entropy_from_counts(counts[n, 3]), e)):
                assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    # the gray formula: pure R, G, B and white
    px = np.array([[[[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255]]]], np.uint8)
    assert R.gray_u8(px, bgr=True)[0, 0].tolist() == [76, 150, 29, 255]
    assert R.gray_u8(px, bgr=False)[0, 0].tolist() == [29, 150, 76, 255]


def test_host_finalisers_match_restatements_on_synthetic_counts():
    g = np.random.default_rng(9)
    ca = g.integers(0, 3000, (3, 4, 256)).astype(np.uint32)  # a batch of 3, as hist_u8 returns it
    cb = g.integers(0, 3000, (3, 4, 256)).astype(np.uint32)
    ca[1, :, 7:] = 0  # nearly everything in a few bins: empty bins go through the + 1
    cb[2] = 0
    ca[0, 3, 0] = 3_000_000_000  # a count above 2^31
    kl = metrics.kl_from_counts(ca, cb)
    mo, un, en = (f(ca[:, 3]) for f in (metrics.moment_from_counts, metrics.uniformity_from_counts,
                                        metrics.entropy_from_counts))
    assert kl.shape == mo.shape == un.shape == en.shape == (3,)
    for n in range(3):
        for got, want in ((kl[n], R.kl_counts(ca[n].astype(np.int64), cb[n].astype(np.int64))),
                          (mo[n], R.moment_counts(ca[n, 3])), (un[n], R.uniformity_counts(ca[n, 3])),
                          (en[n], R.entropy_counts(ca[n, 3]))):
            assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want), (n, got, want)
    assert metrics.kl_from_counts(ca, ca).tolist() == [0.0, 0.0, 0.0]


def test_metrics_refuse_cpu_tensors_and_bad_arguments():
    a = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    for call in (lambda: metrics.ssim(a, a), lambda: metrics.kl(a, a), lambda: metrics.moment(a),
                 lambda: metrics.uniformity(a), lambda: metrics.entropy(a), lambda: ops.hist_u8(a),
                 lambda: ops.gram(torch.zeros(1, 2, 2, 4))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    with pytest.raises(ValueError):
        metrics.ssim(a, a, reduction="sum")
    with pytest.raises(ValueError):
        metrics.gram(a, a)  # no VGG19 given
    assert metrics.SCORE_KEYS == ("ssim_content", "kl_c", "ssim_style", "kl_s", "gram", "moment", "uniformity",
                                  "entropy")
