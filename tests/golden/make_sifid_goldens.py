"""SIFID golden, produced by the reference's own SIFID package.

Runs in the build container only.  SIFID/inception.py and SIFID/sifid_score.py import torchvision at module
level, which is not installed, and inception.py:60 asks it for ImageNet weights (a remote download this
environment cannot make).  This script puts a stand-in into sys.modules before importing the package:
  * torchvision.models.inception_v3(weights=...) -> tests/inception_ref.py's restated modules under
    torchvision's names, holding the seeded recipe weights of inception_ref.recipe();
  * tqdm gets an inert stand-in if it is missing.
Then the reference's own InceptionV3, calculate_activation_statistics and calculate_frechet_distance run in
fp32 on the CPU on image FILES this script writes into a temporary directory — the body of
eval.calculate_sifid_given_paths (eval.py itself needs cv2 and is not imported).  This script holds none
of the package's text.

Inputs, u8 RGB 139 x 123 (H x W): a = seeded noise, b = an arithmetic pattern.  The feature maps are
69x61 -> 67x59 (dims 64), 31x27 (192), 7x6 (768) and 3x2 (2048): every stride-2 layer meets an odd size at
least once, and the deepest map has 6 samples of 2048 channels (the rank-deficient case).  PNG files give
the reference's table scale (imread returns [0, 1], sifid_score.py:104 divides by 255 again); for the
"unit" scale (what a JPEG file gets) one JPEG per image is written and the DECODED bytes are the stored image.

Stored: a, b (PNG), a_jpg, b_jpg (decoded JPEG); levels_reference, levels_unit [256] fp32 (the trunk input of
each byte value as the reference produced it); ref_d2 [4] (dims 64, 192, 768, 2048) and ref_d2_unit [2] (dims
2048, 64); fd64 / fd64_unit (inception_ref.fd64 on the fp64 restatement's features); tr_s [4][2], mu_dist [4]
(|mu1 - mu2|) of the reference; ref_feat_2048 [2][3][2][2048] (the reference's final NHWC features);
ref_vs_fp64_feat [4], ref_vs_fp64_feat_unit [2] (norm-relative error of the reference's fp32 features
against fp64, the larger of the two images) and ref_vs_fp64_d2 [4], ref_vs_fp64_d2_unit [2] (relative):
the reference's own fp32 error, which every device bound is scaled by; sqrtm_imag [4] (max |imag| of
scipy's sqrtm diagonal) and sqrtm_vs_nuclear [4] (relative difference in d^2 between scipy's sqrtm and the
nuclear-norm form on the reference's own fp32 features).

Usage:  python tests/golden/make_sifid_goldens.py <path to the reference's MHAdaSTr directory>
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import inception_ref as R  # noqa: E402

H, W = 139, 123


def images():
    a = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    b = np.stack([(3 * x + 5 * y) % 256, (7 * x * y + 11 * y) % 256, 255 - ((x * x + 2 * y) % 200)], axis=-1).astype(np.uint8)
    return a, b


def load_reference_sifid(ref_dir, sd):
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.inception_v3 = lambda weights=None, **kw: R.build_torchvision(sd)
    tv.models = models
    sys.modules.update({"torchvision": tv, "torchvision.models": models})
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = tq
    sys.path.insert(0, ref_dir)
    from SIFID import sifid_score
    from SIFID.inception import InceptionV3
    return sifid_score, InceptionV3


def main():
    torch.set_num_threads(8)
    from matplotlib.pyplot import imread
    from PIL import Image
    from scipy import linalg
    sd = R.recipe()
    S, InceptionV3 = load_reference_sifid(sys.argv[1], sd)
    net64 = R.build_torchvision(sd, torch.float64)
    a, b = images()
    out = {"a": a, "b": b}
    tmp = tempfile.mkdtemp()
    files = {}
    for name, img in (("a", a), ("b", b)):
        files[name, "png"] = os.path.join(tmp, f"{name}.png")
        Image.fromarray(img).save(files[name, "png"])
        files[name, "jpg"] = os.path.join(tmp, f"{name}.jpg")
        Image.fromarray(img).save(files[name, "jpg"], quality=95)
        out[f"{name}_jpg"] = np.asarray(Image.open(files[name, "jpg"]).convert("RGB"))
        assert np.array_equal((imread(files[name, "png"])[..., :3] * 255).round().astype(np.uint8), img)
        assert np.array_equal(imread(files[name, "jpg"])[..., :3], out[f"{name}_jpg"])

    # the trunk input of each byte value, produced as sifid_score.py:97-104 produces it from a file
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ramp = np.stack([ramp] * 3, axis=-1)
    Image.fromarray(ramp).save(os.path.join(tmp, "ramp.png"))
    lv = imread(os.path.join(tmp, "ramp.png")).astype(np.float32)[..., 0].reshape(-1)
    lv /= 255
    out["levels_reference"] = lv
    lu = ramp[..., 0].reshape(-1).astype(np.float32)  # imread of a JPEG returns the u8 array
    lu /= 255
    out["levels_unit"] = lu

    def one_scale(ext, dims_list, imgs):
        res = {k: [] for k in ("d2", "fd64", "tr", "mud", "feat_err", "d2_err", "imag", "sq_vs_nuc")}
        x64 = [torch.from_numpy(out[f"levels_{'reference' if ext == 'png' else 'unit'}"][im.astype(np.int64)])
               .permute(2, 0, 1)[None].double() for im in imgs]
        # fp64 of the reference's own fp32 INPUT: the input's rounding is not an error of the trunk
        taps64 = [R.trunk(net64, x) for x in x64]
        for dims in dims_list:
            blk = InceptionV3.BLOCK_INDEX_BY_DIM[dims]
            model = InceptionV3([blk])
            acts = [S.get_activations([files[n, ext]], model, 1, dims, False) for n in ("a", "b")]
            stats = [S.calculate_activation_statistics([files[n, ext]], model, 1, dims, False) for n in ("a", "b")]
            (m1, s1), (m2, s2) = stats
            covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
            assert np.isfinite(covmean).all()
            imag = float(np.abs(np.diagonal(covmean).imag).max()) if np.iscomplexobj(covmean) else 0.0
            assert imag <= 1e-3, imag  # the reference's own acceptance, sifid_score.py:173-177
            d2 = float(S.calculate_frechet_distance(m1, s1, m2, s2))
            r64 = [R.rows(t[blk]) for t in taps64]
            for r in r64:
                assert (np.abs(r).sum(axis=1) > 0).all(), "no position may have an all-zero channel vector"
            f64 = R.fd64(*r64)
            nuc = R.fd64(acts[0].astype(np.float64), acts[1].astype(np.float64))
            tr = [float(np.trace(s1)), float(np.trace(s2))]
            assert d2 >= 1e-3 * (tr[0] + tr[1]) and f64 >= 1e-3 * (tr[0] + tr[1]), (dims, d2, f64, tr)
            res["d2"].append(d2)
            res["fd64"].append(f64)
            res["tr"].append(tr)
            res["mud"].append(float(np.linalg.norm(m1 - m2)))
            res["feat_err"].append(max(R.norm_rel(x, r) for x, r in zip(acts, r64)))
            res["d2_err"].append(abs(d2 - f64) / f64)
            res["imag"].append(imag)
            res["sq_vs_nuc"].append(abs(d2 - nuc) / nuc)
            print(f"{ext} dims {dims}: n {acts[0].shape[0]} d2 {d2:.9g} fd64 {f64:.9g} tr {tr} |dmu| {res['mud'][-1]:.4g} "
                  f"feat err {res['feat_err'][-1]:.3e} d2 err {res['d2_err'][-1]:.3e} sqrtm imag {imag:.3e} "
                  f"sqrtm vs nuclear {res['sq_vs_nuc'][-1]:.3e}", flush=True)
            if dims == 2048 and ext == "png":
                out["ref_feat_2048"] = np.stack([x.reshape(3, 2, 2048) for x in acts]).astype(np.float32)
        return {k: np.asarray(v) for k, v in res.items()}

    r = one_scale("png", R.DIMS, (a, b))
    out.update(ref_d2=r["d2"], fd64=r["fd64"], tr_s=r["tr"], mu_dist=r["mud"], ref_vs_fp64_feat=r["feat_err"],
               ref_vs_fp64_d2=r["d2_err"], sqrtm_imag=r["imag"], sqrtm_vs_nuclear=r["sq_vs_nuc"])
    u = one_scale("jpg", (2048, 64), (out["a_jpg"], out["b_jpg"]))
    out.update(ref_d2_unit=u["d2"], fd64_unit=u["fd64"], ref_vs_fp64_feat_unit=u["feat_err"],
               ref_vs_fp64_d2_unit=u["d2_err"])

    path = os.path.join(HERE, "sifid_inception_139x123.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")

    keys = sorted(InceptionV3([3]).state_dict().keys())
    import json
    kp = os.path.join(HERE, "state_dict_keys_inception.json")
    with open(kp, "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print(f"wrote {kp} ({len(keys)} keys)")


if __name__ == "__main__":
    main()
