"""Records tests/golden/pil_resize.npz: for every case of tests/pil_resize_ref.py and both image kinds, the
seeded input and what ``PIL.Image.resize((Wo, Ho), Image.BILINEAR)`` makes of it, with ``PIL.__version__``.
Needs Pillow; the file holds only pixel arrays and the version string.

    python tests/golden/make_pil_resize_goldens.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pil_resize_ref as R  # noqa: E402


def main():
    out = {"pil_version": np.array(PIL.__version__)}
    for case in R.CASES:
        (_, _), (Ho, Wo) = case
        for kind in R.KINDS:
            x = R.make_input(case, kind)
            y = np.asarray(Image.fromarray(x).resize((Wo, Ho), Image.BILINEAR))
            assert y.shape == (Ho, Wo, 3) and y.dtype == np.uint8
            out["in_" + R.case_name(case, kind)] = x
            out["out_" + R.case_name(case, kind)] = y
    path = os.path.join(HERE, "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
