"""The premises of tests/test_gpu_row_forms.py, checked without a GPU on its own form table, its dispatch
transcription and the probes, references and bounds of tests/row_probe.py, so that the GPU file cannot pass because
its table or its reference drifted:

  * plan() sends every row to the kernel the row names, the names are unique, and every instantiation the entries
    can launch (read off csrc/small_ops.hip, csrc/train_ops.hip and csrc/attn_hd.hip themselves) has a row;
  * DESIGN.md "Row-kernel forms under test" lists the same rows;
  * the probes do what they claim in fp32 torch: the select probe's off-key exponentials are exactly 0, the uniform
    and integer cases are exact, the clamp-boundary rows land on the intended side;
  * the fp32 torch evaluation of every formula stays within half of its bound: the condition that fixes
    row_probe.C_RSQRT and row_probe.C_EXP;
  * one deliberately mis-addressed result per family falls outside the bound.
"""
import os
import re

import pytest
import torch

import row_probe as P
import test_gpu_row_forms as T
from mhada_hip import _lib

ROWS = [p.values[0] for p in T.FORMS]
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "csrc")
REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
F32 = torch.float32


def ratio(got, ref, bound):
    return ((got.double() - ref).abs() / bound).max().item()


# --------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------
def test_names_are_unique_and_rows_complete():
    names = [fm["name"] for fm in ROWS]
    assert len(names) == len(set(names))
    for fm in ROWS:
        assert fm["kernel"] and fm["cond"] and fm["fam"] in T.RUN


@pytest.mark.parametrize("fm", T.FORMS)
def test_dispatch_transcription_matches_the_row(fm):
    assert T.plan(fm) == fm["kernel"]
    if fm["fam"] == "attn" and fm["entry"] != "attn":
        for lay in T.LAYOUTS:  # the entries refuse a pstride below the payload
            assert T.pstride_of(fm, lay) >= fm["L"] * lay[0] * lay[1] * 64 * (3 if fm["entry"] == "bwd_s3" else 1)
    if fm["kernel"] == "vit_batch_copy_v_s3_kernel":
        assert all(T.pstride_of(fm, lay) % 4 == 0 for lay in T.LAYOUTS)
    if fm["name"] == "vba_s3_L1_pstride_odd":
        assert all(T.pstride_of(fm, lay) % 4 != 0 for lay in T.LAYOUTS)


def _body(src, start, end):
    return src[src.index(start):src.index(end, src.index(start))]


def launched_instantiations():
    small = open(os.path.join(CSRC, "small_ops.hip")).read()
    train = open(os.path.join(CSRC, "train_ops.hip")).read()
    hd = open(os.path.join(CSRC, "attn_hd.hip")).read()
    out = set()
    # LayerNorm: the LN_CASE macro of each entry, expanded over its cases
    for start, end in (('extern "C" int mhada_layernorm_half2(', 'extern "C" int mhada_split3_weight('),
                       ('extern "C" int mhada_layernorm(', 'extern "C" int mhada_vit_batch_attn(')):
        body = _body(small, start, end)
        widths = re.findall(r"LN_CASE\((\d+)\)\n", body)
        assert widths == ["4", "8", "16", "32"]
        for t, form in re.findall(r"layernorm_kernel<(\w+), VPL(?:, (\d))?>", body):
            out |= {f"layernorm_kernel<{t}, {v}, {form or 0}>" for v in widths}
    # the other entries of small_ops.hip, as written at their launches
    body = _body(small, 'extern "C" int mhada_vit_batch_attn(', 'extern "C" int mhada_transpose_v(')
    body += _body(small, 'extern "C" int mhada_cosine_prep(', "template <typename YT>\nstatic")
    out |= {m.replace(",", ", ").replace(",  ", ", ") for m in re.findall(r"hipLaunchKernelGGL\(\(?(\w+(?:<[^>]*>)?)\)?,", body)}
    # train_ops.hip
    body = _body(train, "static int layernorm_fwd_launch(", 'extern "C" int mhada_relu_bwd(')
    body += _body(train, 'extern "C" int mhada_vit_batch_attn_bwd(', "mhada_vit_batch_attn_bwd_split3\");")
    out |= set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+(?:<[^>]*>)?)\)?,", body))
    out |= set(re.findall(r"attn_bwd_prep_kernel<\d+>", _body(train, "static int launch_bwd_prep(", 'extern "C" int mhada_attn_train_bwd_prep(')))
    out.discard("slab_reduce_kernel")  # the TN forms file's
    out.discard("D == 32 ? attn_bwd_prep_kernel<32> : D == 64 ? attn_bwd_prep_kernel<64> : attn_bwd_prep_kernel<128>")
    out |= set(re.findall(r"hipLaunchKernelGGL\(\((vit_batch_attn_hd_kernel<\w+, \d+>)\)", hd))
    return {k for k in out if "?" not in k}


def test_every_launched_instantiation_has_a_row():
    launched = launched_instantiations()
    named = {k for fm in ROWS for k in fm["kernel"].split(" + ")}
    assert launched == named, (sorted(launched - named), sorted(named - launched))
    assert len(named) >= 40


def test_design_md_lists_the_same_rows():
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    sec = text[text.index("#### Row-kernel forms under test"):]
    nxt = re.search(r"\n#{2,4} ", sec[10:])
    sec = sec[:nxt.start() + 10] if nxt else sec
    listed = re.findall(r"^\| `([^`]+)` \| `([^`]+)` \| (.*?) \|$", sec, re.M)
    assert [(n, k, c) for n, k, c in listed] == [(fm["name"], fm["kernel"], fm["cond"].replace("|", "\\|")) for fm in ROWS]


# --------------------------------------------------------------------------------------------------
# the probes do what they claim, in fp32 torch
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("L", [2, 3, 5, 8, 11])
def test_select_probe_is_exact_in_fp32(L, D):
    for ntok, heads in T.LAYOUTS:
        for bf in (False, True):
            qkv, sel = P.attn_select(L, ntok, heads, D, bf16=bf)
            assert torch.equal(qkv.to(torch.bfloat16 if bf else F32).double(), qkv)       # every value representable
            q, k, v, s, p = P.attn_parts(qkv, F32)
            e = torch.exp(s - s.amax(-1, keepdim=True))
            on = torch.nn.functional.one_hot(sel, L).permute(1, 2, 0, 3).bool()              # [n][h][i][j]
            assert bool((e[on] == 1).all()) and bool((e[~on] == 0).all())
            assert bool(((s.amax(-1, keepdim=True) - s)[~on] >= 128).all())
            want = torch.gather(qkv[:, :, 2], 0, sel[..., None].expand(L, ntok, heads, D)).reshape(L, ntok, heads * D)
            assert torch.equal(P.attn_f32(qkv).double(), want)
            assert len({int(x) for x in sel[:, 2 // heads, 2 % heads]}) < L or L == 2   # pair 2: a key selected twice
            dout = P.int_dout(L, ntok, heads, D)
            ex = P.select_bwd_exact(sel, dout, heads, D)
            assert (P.attn_bwd_ref(qkv, dout) - ex).abs().max() < 1e-30
            assert torch.equal(ex[:, :, 2].sum(0), dout.view(L, ntok, heads, D).sum(0))


@pytest.mark.parametrize("L", [2, 4, 8])
def test_uniform_probe_is_exact_in_fp32(L):
    for ntok, heads in T.LAYOUTS:
        qkv, dout = P.attn_uniform(L, ntok, heads, 64), P.int_dout(L, ntok, heads, 64)
        ref = P.attn_ref(qkv)
        assert torch.equal(P.attn_f32(qkv).double(), ref) and torch.equal(ref.bfloat16().double(), ref)
        x = qkv.float().requires_grad_(True)
        P.attn_ref(x, F32).backward(dout.float())
        assert torch.equal(x.grad.double(), P.attn_bwd_ref(qkv, dout))


def test_integer_cases_are_exact_in_fp32():
    for cols in (256, 512, 1024, 2048):
        x, g, b, m0, k = P.ln_exact(131, cols)
        assert torch.equal(x.float().sum(-1).double() / cols, m0)
        assert torch.equal(x.float().flip(-1).cumsum(-1)[:, -1].double() / cols, m0)          # another order
        assert bool(((x - m0[:, None]).abs() == torch.pow(2.0, k)[:, None]).all()) and bool((x.sum(-1) == cols * m0).all())
        assert len(set(b.tolist())) == cols and bool((g == g.round()).all())
    assert 16 * 33 * 1023 ** 2 < 2 ** 53
    o = P.fold_operands(2, 3, True)
    r = P.fold_ref(o, 1.0, 2, 3)
    assert torch.equal(r["wq"].float().double(), r["wq"]) and torch.equal(r["wkv"].float().double(), r["wkv"])


def test_clamp_rows_land_on_the_intended_side():
    c = float(P.CLAMP)
    assert float(P.CLAMP_BELOW) < c < float(P.CLAMP_ABOVE)
    assert P.CLAMP.view(torch.int32).item() == 0x358637BD and P.CLAMP_BELOW.view(torch.int32).item() == 0x358637BC
    assert P.VAR_GRID_BELOW < c < P.VAR_GRID_ABOVE
    for D in (32, 64, 128):
        dout, x, m, e2, active = P.prep_clamp_rows(D)
        assert torch.equal(e2.float().double(), e2) and torch.equal(m.float().double(), m)
        for dt in (F32, torch.float64):
            r = P.prep_ref(dout, x, m, e2, dt)
            assert bool(((r["dvar"] == 0).all(-1) == active).all()) and bool(((r["dvar"] != 0).all(-1) == ~active).all())
        var32 = e2.float() - m.float() * m.float()
        assert torch.equal(var32.double(), e2 - m * m)                                      # exact, contracted or not


# --------------------------------------------------------------------------------------------------
# the fp32 torch evaluation stays within half of each bound (fixes C_RSQRT and C_EXP)
# --------------------------------------------------------------------------------------------------
def test_fp32_layernorm_within_half_the_bound():
    worst = 0.0
    for cols in (256, 512, 1024, 2048):
        for rows, offset in ((5, 0.0), (131, 0.0), (5, 1000.0)):
            x, g, b = P.ln_gauss(rows, cols, offset, seed=rows)
            r, f = P.ln_ref(x, g, b), P.ln_f32(x, g, b)
            bd = P.ln_bound(x, g, r)
            worst = max(worst, ratio(f["y"], r["y"], bd["y"]), ratio(f["mean"], r["mean"], bd["mean"]),
                        ratio(f["rstd"], r["rstd"], bd["rstd"]))
            assert r["rstd"].min() > 0.1                                                     # well conditioned
    print("fp32 LayerNorm error / bound", worst)
    assert worst <= 0.5


def test_fp32_layernorm_backward_within_half_the_bound():
    for cols in (256, 1024):
        x, g, b = P.ln_gauss(129, cols, seed=129)
        dy = P.randn(129, cols, seed=1029)
        r = P.ln_ref(x, g, b)
        ref, bd = P.ln_bwd_ref(x, dy, g), P.ln_bwd_bound(x, dy, g, r)
        xf, gf = x.float().requires_grad_(True), g.float().requires_grad_(True)
        bf = b.float().requires_grad_(True)
        P.ln_ref(xf, gf, bf, dt=F32)["y"].backward(dy.float())
        for name, t in (("dx", xf.grad), ("dgamma", gf.grad), ("dbeta", bf.grad)):
            assert ratio(t, ref[name], bd[name]) <= 0.5, name


def test_fp32_attention_within_half_the_bound():
    worst = wb = 0.0
    for D in (32, 64, 128):
        for L in (2, 3, 5, 8, 9, 11):
            for ntok, heads in T.LAYOUTS:
                qkv = P.attn_gauss(L, ntok, heads, D, seed=L)
                worst = max(worst, ratio(P.attn_f32(qkv), P.attn_ref(qkv), P.attn_bound(qkv)))
                if D == 64 and L <= 8:
                    dout = P.randn(L, ntok, heads * D, seed=950 + L)
                    x = qkv.float().requires_grad_(True)
                    P.attn_ref(x, F32).backward(dout.float())
                    wb = max(wb, ratio(x.grad, P.attn_bwd_ref(qkv, dout), P.attn_bwd_bound(qkv, dout)))
    print("fp32 attention error / bound", worst, "backward", wb)
    assert worst <= 0.5 and wb <= 0.5


def test_fp32_small_ops_within_half_the_bound():
    for D in (32, 64, 128):
        o = P.prep_gauss(9, D, seed=9)
        r, f = P.prep_ref(*o), P.prep_ref(*o, dt=F32)
        bd = P.prep_bound(*o, r)
        for name in ("dx", "dm", "dvar", "dd"):
            assert ratio(f[name], r[name], bd[name]) <= 0.5, name
    x = P.randn(7, 64, seed=3)
    ref = P.rownorm_ref(x)
    assert ratio(P.rownorm_ref(x.float()), ref, P.rownorm_bound(ref, False)) <= 0.5
    for ks in (1.0, 1.4426950216293335):
        o = P.fold_operands(2, 3, False, seed=5)
        r = P.fold_ref(o, ks, 2, 3)
        f = P.fold_ref({k: v.float() for k, v in o.items()}, ks, 2, 3)
        bd = P.fold_bound(r, False)
        for name in ("wq", "wkv", "bkv", "v_mu"):
            # no intrinsic here: wq and bkv round once, so their bound u |ref| is the rounding itself
            assert ((f[name].double() - r[name]).abs() <= (0.5 if name == "v_mu" else 1.0) * bd[name]).all(), name
    # the forward resize is PyTorch's fp32 one: its CPU fp32 evaluation against the fp64 matrix
    for (bh, bw), (oh, ow) in P.POS_SIZES[1:]:
        for C in (5, 64):
            W, pos = P.resize_matrix(bh, bw, oh, ow), P.randn(C, bh, bw, seed=C)
            f = torch.nn.functional.interpolate(pos.float()[None], size=(oh, ow), mode="bilinear", align_corners=False)
            assert ratio(f.reshape(C, -1).t(), P.pos_fwd(pos, W), P.pos_fwd_bound(pos, W, (oh, ow))) <= 0.5
    xs = (P.randn(3, 33, 68, seed=1) * 2 + 1000).float().double()
    r = P.in_ref(xs)
    assert r["rstd"].min() > 0.1 and torch.allclose(r["var"], xs.var(1, unbiased=False), rtol=1e-9)


# --------------------------------------------------------------------------------------------------
# a mis-addressed result falls outside the bound
# --------------------------------------------------------------------------------------------------
def test_misaddressed_results_fall_outside_the_bound():
    # LayerNorm: two columns swapped (exact probe: beta moves the element by at least 1)
    for xgb in (P.ln_exact(5, 256)[:3], P.ln_gauss(5, 256, seed=5)):
        r = P.ln_ref(*xgb)
        y = r["y"].clone()
        y[:, [10, 11]] = y[:, [11, 10]]
        assert ratio(y, r["y"], P.ln_bound(xgb[0], xgb[1], r)["y"]) > 1
        last = r["y"].clone()
        last[-1] = last[-2]                                    # the last row dropped (left at its neighbour's)
        assert ratio(last, r["y"], P.ln_bound(xgb[0], xgb[1], r)["y"]) > 1
    # attention: one key counted twice
    qkv = P.attn_gauss(3, 7, 3, 64, seed=3)
    q, k, v, s, p = P.attn_parts(qkv)
    w = torch.exp(s - s.amax(-1, keepdim=True))
    w[..., 1] *= 2
    bad = ((w / w.sum(-1, keepdim=True)) @ v).permute(2, 0, 1, 3).reshape(3, 7, 192)
    assert ratio(bad, P.attn_ref(qkv), P.attn_bound(qkv)) > 1
    dout = P.randn(3, 7, 192, seed=953)
    ref = P.attn_bwd_ref(qkv, dout)
    bad = ref.clone()
    bad[-1, :, 2] = 0                                          # dv of the last key dropped
    assert ratio(bad, ref, P.attn_bwd_bound(qkv, dout)) > 1
    # positional embedding: the adjoint without the last target row; the forward reading a neighbouring source
    W = P.resize_matrix(5, 3, 11, 7)
    g = P.randn(77, 5, seed=15)
    Wd = W.clone()
    Wd[-7:] = 0
    assert ratio(P.pos_bwd(g, Wd), P.pos_bwd(g, W), P.pos_bwd_bound(g, W)) > 1
    pos = P.randn(5, 5, 3, seed=5)
    assert ratio(P.pos_fwd(pos.roll(1, -1), W), P.pos_fwd(pos, W), P.pos_fwd_bound(pos, W, (11, 7))) > 1
    # InstanceNorm: the last token left out
    x = P.randn(1, 17, 4, seed=18) * 2
    r, rb = P.in_ref(x), P.in_ref(x[:, :-1])
    bd = P.in_bound(x, r)
    assert ratio(rb["mu"], r["mu"], bd["mu"]) > 1 and ratio(rb["rstd"], r["rstd"], bd["rstd"]) > 1
    # fold: rstd_c of the neighbouring column; cosine prep: the norm over 63 elements; prep: m and e2 swapped
    o = P.fold_operands(1, 1, False)
    r = P.fold_ref(o, 1.0, 1, 1)
    bad = P.fold_ref(dict(o, rstd_c=o["rstd_c"].roll(1, -1)), 1.0, 1, 1)
    assert ratio(bad["wq"], r["wq"], P.fold_bound(r, False)["wq"]) > 1
    x = P.randn(7, 64, seed=3)
    ref = P.rownorm_ref(x)
    assert ratio(x / x[:, :63].pow(2).sum(-1, keepdim=True).sqrt(), ref, P.rownorm_bound(ref, True)) > 1
    dout, xx, m, e2 = P.prep_gauss(9, 32, seed=9)
    r = P.prep_ref(dout, xx, m, e2)
    bad = P.prep_ref(dout, xx, m.roll(1, 0), e2.roll(1, 0))
    assert ratio(bad["dd"].view(-1, 1), r["dd"].view(-1, 1), P.prep_bound(dout, xx, m, e2, r)["dd"].view(-1, 1)) > 1
