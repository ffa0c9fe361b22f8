"""The premises of tests/test_gpu_tn_forms.py, checked without a GPU on its own form table, operand generators
and dispatch transcription, so that the GPU file cannot pass because its table or its reference drifted:

  * every case satisfies 16 K < 2^24, its integer reference is its own fp32 rounding, and its Gaussian
    reference rounded to fp32 stays inside the stated bound on its own;
  * plan(), the Python transcription of tn_splits, kchunk and the dispatch predicates of mhada_gemm_tn (bm,
    vec_a, rsrc, fuse_cs, the skinny and LDS-tiled conditions), sends every case to the kernel its row names,
    with the S, the last-stage length and the column-sum route its row claims; tn_splits is compared with
    mhada_gemm_tn_splits where the library loads;
  * every instantiation mhada_gemm_tn can launch has a case, read off csrc/train_ops.hip itself.
"""
import os
import re

import pytest
import torch

import test_gpu_tn_forms as TF
from mhada_hip import _lib

CASES = [p.values[0] for p in TF.FORMS]
SRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "csrc", "train_ops.hip")


def test_names_are_unique_and_rows_complete():
    names = [fm["name"] for fm in CASES]
    assert len(names) == len(set(names))
    for fm in CASES:
        assert fm["kernel"] and fm["cond"] and fm["S"] >= 1
        assert (fm["last"] is not None) == fm["kernel"].startswith("gemm_tn_kernel")


@pytest.mark.parametrize("fm", TF.FORMS)
def test_dispatch_transcription_matches_the_row(fm):
    for colsum in (False, True):
        pl = TF.plan(fm, colsum, False)
        assert pl["kernel"] == fm["kernel"], (pl["kernel"], fm["kernel"])
        assert pl["S"] == fm["S"], pl["S"]
        assert fm["last"] is None or pl["last"] == fm["last"], pl["last"]
        assert pl["cs"] == (fm["cs"] if colsum else None), pl["cs"]
        one = TF.plan(fm, colsum, True)
        assert one["kernel"] == fm["kernel"] and one["S"] == 1 and one["wf"] == one["per"]
        assert one["kchunk"] >= fm["K"]
        if fm["cs"] == "fused":
            assert pl["fuse"] == colsum and pl["per"] == fm["nb"] * (fm["M"] * fm["N"] + (fm["M"] if colsum else 0))
    # the row's words against the predicates
    k = fm["kernel"]
    if k.startswith("gemm_tn_kernel"):
        mode, vec, bm, rs = k[len("gemm_tn_kernel<"):-1].split(",")
        assert mode == TF.MODE_NAME[fm["mode"]] and int(bm) == (64 if fm["M"] <= 64 else 128) and fm["M"] > 4
        assert (vec == "true") == (fm["a_off"] == 0 and fm["M"] % 4 == 0 and fm["lda"] % 4 == 0)
        assert (rs == "true") == (vec == "true" and fm["mode"] == TF.ROWS and fm["ldb"] < TF.BIG_LDB)
    else:
        assert fm["M"] <= 4
        assert k.startswith("tn_skinny_lds_kernel") == (fm["mode"] != TF.ROWS and fm["img"][3] % 64 == 0 and fm["lda"] == 4
                                                        and bool(fm["lds"]))


def test_tn_splits_is_the_librarys():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmhada_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    shapes = {(fm["M"], fm["N"], fm["K"]) for fm in CASES}
    shapes |= {(M, N, K) for M in (1, 4, 5, 64, 65, 512) for N in (4, 128, 132, 4608) for K in (1, 255, 257, 2047, 2048, 10 ** 6)}
    for M, N, K in sorted(shapes):
        assert lib.mhada_gemm_tn_splits(M, N, K) == TF.tn_splits(M, N, K), (M, N, K)


def test_big_ldb_turns_the_buffer_resources_off():
    assert 32 * TF.BIG_LDB * 4 >= 0x7ff00000 and 32 * TF.BIG_LDB * 4 <= 0x7fffffff
    assert 32 * 140 * 4 < 0x7ff00000


def test_slab_reduce_loops_have_a_case():
    S = {fm["name"]: fm["S"] for fm in CASES if fm["mode"] == TF.ROWS and fm["M"] > 4}
    assert any(s >= 9 for s in S.values()) and any(2 <= s <= 8 for s in S.values())
    assert any(fm["S"] >= 2 for fm in CASES if fm["kernel"].startswith("tn_skinny_lds"))


def test_every_launched_instantiation_has_a_case():
    """The instantiations are read off the launch code of mhada_gemm_tn; the table may leave none out."""
    src = open(SRC).read()
    body = src[src.index('extern "C" int mhada_gemm_tn('):src.index('extern "C" int mhada_colsum(')]
    modes = re.findall(r"TN_LAUNCH\(MHADA_A_(\w+)\);", body)
    assert sorted(modes) == ["CONV3X3", "CONV3X3_ZERO", "PATCH8", "ROWS"]
    launched = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?(\w+)<([^>]*)>", body):
        kern, targs = m.group(1), [t.strip().replace("MHADA_A_", "") for t in m.group(2).split(",")]
        for mode in (modes if targs[0] == "MODE" else [targs[0]]):
            if kern == "gemm_tn_kernel":
                launched.add("gemm_tn_kernel<%s>" % ",".join([mode] + targs[1:] + ["false"] * (4 - len(targs))))
            else:
                launched.add(f"{kern}<{mode}>")
    launched.discard("tn_skinny_kernel<PATCH8>")  # refused before the launch: "PATCH8 needs M > 4"
    assert "PATCH8 needs M > 4" in body
    assert sorted(launched) == TF.INSTANTIATIONS
    assert {fm["kernel"] for fm in CASES} == launched


@pytest.mark.parametrize("fm", TF.FORMS)
def test_exact_case_premises(fm):
    pb = TF.problem(fm, True)
    pb.exact_premises(fm)
    assert bool((pb.mag >= pb.ref.abs()).all())
    assert pb.cols.shape == (fm["nb"], fm["K"], fm["N"])
    for k in TF.probe_ks(fm, TF.plan(fm, False, False)["kchunk"]):
        assert 0 <= k < fm["K"]


@pytest.mark.parametrize("fm", TF.FORMS)
def test_gaussian_reference_alone_is_inside_the_bound(fm):
    pb = TF.problem(fm, False)
    assert torch.equal(pb.a.float().double(), pb.a) and torch.equal(pb.b.float().double(), pb.b)
    assert bool(((pb.ref.float().double() - pb.ref).abs() <= TF.bound_c(fm, pb, 1)).all())
    assert bool(((pb.cs.float().double() - pb.cs).abs() <= TF.bound_cs(fm, pb)).all())
    assert TF.gamma(fm["K"] + 1024) < 1e-3


def test_colsum_cases():
    for rows, C, wf, chunks in TF.COLSUM_CASES:
        assert 4 * rows < 2 ** 24 and C % 4 == 0
    assert {c[1] // 4 > 256 for c in TF.COLSUM_CASES} == {True, False}  # one and two column blocks
