"""A pure-numpy restatement of PIL's ``Image.resize(size, Image.BILINEAR)`` for 8-bit three-channel images
(Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc), the
yardstick of the image-ingest tests where PIL cannot be assumed to exist.  test_image_ingest_cpu.py holds it to
PIL's own outputs (tests/golden/pil_resize.npz, and PIL itself where it is installed), byte for byte.

Per axis, n_in -> n_out, all in IEEE double:
    scale = n_in / n_out, fs = max(scale, 1), support = 1.0 * fs, ksize = ceil(support) * 2 + 1;
    for output index xx: center = (xx + 0.5) * scale,
        xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), n_in) - xmin,
        w[x] = tri((x + xmin - center + 0.5) * (1 / fs)), tri(t) = max(0, 1 - |t|), x < xmax,
        each divided by their running sum when it is non-zero; k = int(0.5 + w * 2^22).
One pass: per channel ss = 2^21 + sum_x in[xmin + x] * k[x] in int32, out = clamp(ss >> 22, 0, 255) as u8.
The horizontal pass runs first (only if Wo != W) and rounds to u8; the vertical pass (only if Ho != H) runs on
that u8 image; the same size on both axes is a copy."""
import math

import numpy as np

PRECISION_BITS = 22

# (H, W) -> (Ho, Wo): the smallest shapes that reach each way the kernels can go wrong
CASES = [
    ((37, 53), (16, 24)),    # non-integer shrink on both axes, ragged edges
    ((16, 24), (37, 53)),    # enlarge, ksize 3, edge clipping
    ((40, 40), (40, 40)),    # copy
    ((64, 48), (64, 16)),    # horizontal pass only
    ((17, 90), (33, 8)),     # enlarge on one axis, shrink > 11x on the other
    ((9, 9), (8, 8)),        # ratios next to 1
    ((8, 8), (9, 9)),
    ((1, 5), (4, 4)),        # one-pixel axis
    ((400, 12), (3, 12)),    # vertical only, ~267 taps
    ((64, 64), (63, 65)),    # both passes
    ((96, 200), (70, 131)),  # outputs cross the kernels' workgroup tile edges on both axes
]
# further axis pairs whose tables are compared (the sizes of real photographs)
EXTRA_AXES = [(4000, 512), (3000, 512), (1080, 512)]
KINDS = ("rand", "bin")


def case_name(case, kind):
    (H, W), (Ho, Wo) = case
    return f"{H}x{W}_to_{Ho}x{Wo}_{kind}"


def make_input(case, kind):
    """The seeded test image of a case: uniform random u8, or random 0 / 255 (every rounding tie and clamp
    reachable)."""
    (H, W), _ = case
    rng = np.random.default_rng(1000 * H + W + (0 if kind == "rand" else 500000))
    if kind == "rand":
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return (rng.integers(0, 2, size=(H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)


def tables(n_in, n_out):
    """(coef int32 [n_out][ksize], bounds int32 [n_out][2] = (xmin, count))"""
    scale = float(n_in) / float(n_out)
    fs = scale if scale > 1.0 else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        xmax -= xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        for x in range(ksize):
            coef[xx, x] = int(0.5 + k[x] * (1 << PRECISION_BITS)) if x < xmax else 0
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def resample_axis0(img, n_out):
    """One pass along axis 0 of a u8 array [n_in][...] -> u8 [n_out][...]"""
    coef, bounds = tables(img.shape[0], n_out)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i in range(n_out):
        xmin, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        k = coef[i, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (img.ndim - 1))
        ss = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + cnt] * k).sum(axis=0)
        assert ss.max(initial=0) < 2 ** 31  # the C code accumulates in a 32-bit int
        out[i] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, Ho, Wo):
    """img u8 [H][W][3] -> u8 [Ho][Wo][3], as Image.fromarray(img).resize((Wo, Ho), Image.BILINEAR)"""
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    out = img
    if Wo != W:
        out = resample_axis0(out.transpose(1, 0, 2), Wo).transpose(1, 0, 2)
    if Ho != H:
        out = resample_axis0(out, Ho)
    return np.ascontiguousarray(out).copy()
