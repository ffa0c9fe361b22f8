"""Image ingest without a GPU: the numpy restatement of PIL's BILINEAR resize (tests/pil_resize_ref.py) against
PIL's recorded outputs (tests/golden/pil_resize.npz, make_pil_resize_goldens.py) and against PIL itself where it
is installed, ``ops.pil_bilinear_tables`` against the restatement's tables, and the host-side argument checks of
``mhada_image_resize``.  Everything is integer arithmetic: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import pil_resize_ref as R
from conftest import load_golden
from mhada_hip import _lib, ops

IDS = [R.case_name(c, k) for c in R.CASES for k in R.KINDS]
PAIRS = [(c, k) for c in R.CASES for k in R.KINDS]


@pytest.fixture(scope="module")
def gold():
    return load_golden("pil_resize")


def test_golden_file_holds_every_case(gold):
    assert str(gold["pil_version"])
    assert set(gold) == {"pil_version"} | {p + n for n in IDS for p in ("in_", "out_")}
    for case, kind in PAIRS:
        n = R.case_name(case, kind)
        assert gold["in_" + n].shape == case[0] + (3,) and gold["out_" + n].shape == case[1] + (3,)
        assert gold["in_" + n].dtype == np.uint8 and gold["out_" + n].dtype == np.uint8
        np.testing.assert_array_equal(gold["in_" + n], R.make_input(case, kind))
    assert set(np.unique(gold["in_" + R.case_name(R.CASES[0], "bin")])) == {0, 255}


@pytest.mark.parametrize("case,kind", PAIRS, ids=IDS)
def test_restatement_equals_pil_goldens(gold, case, kind):
    n = R.case_name(case, kind)
    got = R.resize(gold["in_" + n], *case[1])
    assert got.dtype == np.uint8 and got.shape == gold["out_" + n].shape
    assert int((got != gold["out_" + n]).sum()) == 0


@pytest.mark.parametrize("case,kind", PAIRS, ids=IDS)
def test_restatement_equals_pil_itself(case, kind):
    Image = pytest.importorskip("PIL.Image")
    x = R.make_input(case, kind)
    (Ho, Wo) = case[1]
    want = np.asarray(Image.fromarray(x).resize((Wo, Ho), Image.BILINEAR))
    assert int((R.resize(x, Ho, Wo) != want).sum()) == 0


def _axis_pairs():
    pairs = []
    for (H, W), (Ho, Wo) in R.CASES:
        pairs += [(H, Ho), (W, Wo)]
    return sorted(set(pairs + R.EXTRA_AXES))


@pytest.mark.parametrize("n_in,n_out", _axis_pairs())
def test_ops_tables_equal_the_restatement(n_in, n_out):
    coef, bounds = ops.pil_bilinear_tables(n_in, n_out)
    rc, rb = R.tables(n_in, n_out)
    assert coef.dtype == np.int32 and bounds.dtype == np.int32
    assert coef.shape == rc.shape and bounds.shape == (n_out, 2)
    np.testing.assert_array_equal(coef, rc)
    np.testing.assert_array_equal(bounds, rb)
    # what the kernels rely on: taps inside the axis and the table row, no negative weight, int32 sums
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= coef.shape[1]).all()
    assert (bounds.sum(axis=1) <= n_in).all() and (coef >= 0).all()
    assert 255 * int(coef.sum(axis=1).max()) + (1 << 21) < 2 ** 31
    assert ops.pil_bilinear_tables(n_in, n_out)[0] is coef  # cached
    assert not coef.flags.writeable and not bounds.flags.writeable


def test_tables_reject_bad_sizes_and_cpu_tensors_raise():
    import torch
    with pytest.raises(ValueError):
        ops.pil_bilinear_tables(0, 4)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.image_resize(torch.zeros(4, 4, 3, dtype=torch.uint8), (2, 2))


def test_image_module_imports_without_pil(monkeypatch):
    import importlib
    import sys

    import mhada_hip.image as image
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)  # any "import PIL" now raises ImportError
    image = importlib.reload(image)
    assert all(hasattr(image, n) for n in ("pil_to_tensor", "resize_u8", "prepare"))
    with pytest.raises(ValueError, match="uint8"):
        image.prepare(np.zeros((4, 4, 3), dtype=np.float32), (2, 2))


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built")
    return _lib.load()


def test_image_resize_is_an_additive_entry_of_abi_18():
    lib = _lib_or_skip()
    for name in ("mhada_image_resize", "mhada_image_resize_work"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["mhada_image_resize"][1]) == 20
    assert _lib.ABI_VERSION == 18 and lib.mhada_abi_version() == 18
    # workspace: the horizontally resampled u8 image [B][H][Wo][3], only when both axes change size
    assert lib.mhada_image_resize_work(2, 37, 53, 16, 24) == 2 * 37 * 24 * 3
    assert lib.mhada_image_resize_work(1, 64, 48, 64, 16) == 0
    assert lib.mhada_image_resize_work(1, 400, 12, 3, 12) == 0
    assert lib.mhada_image_resize_work(1, 40, 40, 40, 40) == 0
    assert lib.mhada_image_resize_work(0, 40, 40, 20, 20) == 0


def test_image_resize_rejects_bad_arguments_without_a_launch():
    """Every bad-argument case returns MHADA_ERR_ARG on the host (no GPU here: a launch would fail differently).
    The pointers are host addresses that are never dereferenced."""
    lib = _lib_or_skip()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    big = (2 ** 31 - 1) // 3 + 1

    def rs(frames=p, B=1, H=37, W=53, row_bytes=None, cx=p, bx=p, kx=7, cy=p, by=p, ky=7, u8=p, out_row=None, f32=p,
           Ho=16, Wo=24, work=p, nwork=1 << 40):
        return lib.mhada_image_resize(frames, B, H, W, 3 * W if row_bytes is None else row_bytes, 0, cx, bx, kx, cy,
                                      by, ky, u8, 3 * Wo if out_row is None else out_row, f32, Ho, Wo, work, nwork,
                                      None)

    bad = [dict(frames=None), dict(u8=None, f32=None), dict(B=0), dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=-3),
           dict(row_bytes=3 * 53 - 1), dict(out_row=3 * 24 - 1), dict(f32=p + 2), dict(cx=None), dict(bx=None),
           dict(cy=None), dict(by=None), dict(cx=p + 1), dict(by=p + 2), dict(kx=0), dict(ky=-1), dict(work=None),
           dict(nwork=37 * 24 * 3 - 1), dict(B=65536), dict(W=big, row_bytes=3 * big), dict(Wo=big, out_row=3 * big),
           dict(H=16 * 65535 + 1), dict(Ho=4 * 65535 + 1),
           # a one-axis resize still needs that axis's tables
           dict(Wo=53, cy=None, work=None), dict(Ho=37, bx=None, work=None)]
    for kw in bad:
        assert rs(**kw) == 1, kw
        assert b"mhada_image_resize" in lib.mhada_last_error(), kw
