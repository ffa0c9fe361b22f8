"""fp64 restatements of the reference's weight-free image metrics (eval.py:38-67, 111-223), for the
metric tests: plain numpy loops over what the reference writes with cv2 / scipy / conv2d, on u8
frames [B][H][W][3] (or one [H][W][3]) already in host memory.  No device code, no scipy.

ssim64 is the truth the device SSIM is held to: SSIMMetric's definition (11 x 11 Gaussian, sigma
1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2 on [0, 255] values, mean over H x W then over the
channels) with the window the reference builds in fp32 and every other operation in fp64.
"""
import numpy as np
import torch

WIN, PAD = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_f32() -> np.ndarray:
    """The [11][11] fp32 window of SSIMMetric.__init__ (eval.py:180-184): linspace, exp, normalise and
    the outer product, every step an fp32 torch operation on the CPU, as the reference runs them."""
    x = torch.linspace(-(WIN // 2), WIN // 2, WIN)
    g = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).numpy()


def _frames(a) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim == 3:
        a = a[None]
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3, (a.dtype, a.shape)
    return a


def _blur(p: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Zero-padded 11 x 11 depthwise correlation of the planes p [B][3][H][W] (fp64) by the primitive
    the reference calls, F.conv2d(padding=5, groups=3) on a contiguous NCHW tensor (what ToTensor
    hands it), so that the sums are formed in its order.  That matters on flat regions, where
    E[x^2] - E[x]^2 cancels to about 1e-8 of its operands and C2 is 9e-4: feeding the same conv2d a
    channels-last view changes one moment by an ulp (7e-12) and the flat-vs-step SSIM by 4e-10, which
    is the conditioning of the definition itself."""
    k = torch.from_numpy(w).expand(p.shape[1], 1, WIN, WIN).contiguous()
    return torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(p)), k, padding=PAD,
                                      groups=p.shape[1]).numpy()


def _blur_taps(p: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The same correlation tap by tap in numpy (no torch): the independent form."""
    H, W = p.shape[-2:]
    q = np.zeros(p.shape[:-2] + (H + 2 * PAD, W + 2 * PAD), np.float64)
    q[..., PAD:PAD + H, PAD:PAD + W] = p
    out = np.zeros(p.shape, np.float64)
    for i in range(WIN):
        for j in range(WIN):
            out += w[i, j] * q[..., i:i + H, j:j + W]
    return out


def ssim_map64(a, b, blur=_blur) -> np.ndarray:
    """The SSIM map [B][3][H][W] of eval.py:199-214 in fp64."""
    w = window_f32().astype(np.float64)
    x = _frames(a).transpose(0, 3, 1, 2).astype(np.float64)
    y = _frames(b).transpose(0, 3, 1, 2).astype(np.float64)
    assert x.shape == y.shape
    mu1, mu2 = blur(x, w), blur(y, w)
    s1 = blur(x * x, w) - mu1 * mu1
    s2 = blur(y * y, w) - mu2 * mu2
    s12 = blur(x * y, w) - mu1 * mu2
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2)
    return num / den


def ssim64(a, b, blur=_blur) -> np.ndarray:
    """Per-image SSIM [B] (reduction="none"): mean over H x W, then over the channels."""
    return ssim_map64(a, b, blur).mean(axis=(2, 3)).mean(axis=1)


def gray_u8(frames, bgr: bool = True) -> np.ndarray:
    """cv2.cvtColor(BGR2GRAY) (RGB2GRAY for bgr = False) as OpenCV 4 computes it for u8:
    (R * 9798 + G * 19235 + B * 3735 + 2^14) >> 15."""
    f = _frames(frames).astype(np.int64)
    r, g, b = (f[..., 2], f[..., 1], f[..., 0]) if bgr else (f[..., 0], f[..., 1], f[..., 2])
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def hist_counts(frames, bgr: bool = True) -> np.ndarray:
    """[B][4][256] int64: np.bincount of the three stored channels and of the gray image (without
    compute_histogram's + 1)."""
    f = _frames(frames)
    gray = gray_u8(f, bgr)
    out = np.zeros((f.shape[0], 4, 256), np.int64)
    for n in range(f.shape[0]):
        for ch in range(3):
            out[n, ch] = np.bincount(f[n, :, :, ch].flatten(), minlength=256)
        out[n, 3] = np.bincount(gray[n].flatten(), minlength=256)
    return out


def entropy_pq(pk, qk) -> float:
    """scipy.stats.entropy(pk, qk): both normalised to sum 1, then sum pk ln(pk / qk) (a term with
    pk = 0 is 0)."""
    pk = np.asarray(pk, np.float64)
    qk = np.asarray(qk, np.float64)
    pk = pk / pk.sum()
    qk = qk / qk.sum()
    s = 0.0
    for p, q in zip(pk, qk):
        if p > 0:
            s += p * np.log(p / q)
    return float(s)


def kl_counts(ca, cb) -> float:
    """kl_loss (eval.py:49-67) from the [>=3][256] channel counts of the two images."""
    return sum(entropy_pq(ca[ch] + 1, cb[ch] + 1) for ch in range(3)) / 3.0


def kl(a, b) -> np.ndarray:
    ca, cb = hist_counts(a), hist_counts(b)
    return np.array([kl_counts(ca[n], cb[n]) for n in range(ca.shape[0])])


def moment_counts(gray_counts) -> float:
    """nth_order_moment (eval.py:111-129) from the gray counts: `hist / 255` of the counts, as written."""
    hist = np.asarray(gray_counts, np.int64) + 1
    hist_p = hist / np.sum(hist)
    hist = hist / 255.0
    hist_mean = np.mean(hist)
    m = 0.0
    for i in range(256):
        m += ((hist[i] - hist_mean) ** 2) * hist_p[i]
    return float(m)


def uniformity_counts(gray_counts) -> float:
    """uniformity (eval.py:132-146)."""
    hist = np.asarray(gray_counts, np.int64) + 1
    hist_p = hist / np.sum(hist)
    u = 0.0
    for i in range(256):
        u += hist_p[i] ** 2
    return float(u)


def entropy_counts(gray_counts) -> float:
    """average_entropy (eval.py:149-164)."""
    hist = np.asarray(gray_counts, np.int64) + 1
    hist_p = hist / np.sum(hist)
    e = 0.0
    for i in range(256):
        if hist_p[i] > 0:
            e -= hist_p[i] * np.log2(hist_p[i])
    return float(e)


def moment(a, bgr: bool = True) -> np.ndarray:
    return np.array([moment_counts(c[3]) for c in hist_counts(a, bgr)])


def uniformity(a, bgr: bool = True) -> np.ndarray:
    return np.array([uniformity_counts(c[3]) for c in hist_counts(a, bgr)])


def entropy(a, bgr: bool = True) -> np.ndarray:
    return np.array([entropy_counts(c[3]) for c in hist_counts(a, bgr)])


def gram64(feat) -> np.ndarray:
    """gram_matrix (eval.py:70-75) of NHWC features [B][H][W][C] in fp64: X^T X / (H W) per image."""
    f = np.asarray(feat, np.float64)
    B, H, W, C = f.shape
    x = f.reshape(B, H * W, C)
    return np.einsum("bpi,bpj->bij", x, x) / (H * W)


def gram_loss64(feats_a, feats_b) -> np.ndarray:
    """gram_loss (eval.py:78-108) per image from two lists of NHWC feature maps (relu1_1 .. relu5_1):
    the sum of the Gram MSEs, divided by 5."""
    tot = 0.0
    for fa, fb in zip(feats_a, feats_b):
        d = gram64(fa) - gram64(fb)
        tot = tot + (d * d).mean(axis=(1, 2))
    return tot / 5.0


# ---- the contents the SSIM tests use ---------------------------------------------------------------
def case_flat_step(H=40, W=40):
    """flat 200 against 200 with the right half 201 (the case the fp32 recipe gets wrong by ~1)."""
    a = np.full((1, H, W, 3), 200, np.uint8)
    b = a.copy()
    b[:, :, W // 2:] = 201
    return a, b


def case_ramp(H=64, W=64):
    """a column ramp 100..140 against the same + 1."""
    col = np.round(np.linspace(100, 140, W)).astype(np.uint8)
    a = np.broadcast_to(col[None, None, :, None], (1, H, W, 3)).copy()
    return a, (a + 1).astype(np.uint8)


def case_noise(H=33, W=45, B=1, seed=0):
    g = np.random.default_rng(seed)
    return (g.integers(0, 256, (B, H, W, 3), dtype=np.uint8), g.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
