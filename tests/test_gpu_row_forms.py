"""Every LayerNorm, batch-axis attention, positional-embedding, InstanceNorm, fold, cosine-prep and backward-prep
kernel form of csrc/small_ops.hip and csrc/train_ops.hip (and the head-width batch attention of csrc/attn_hd.hip),
element by element.

FORMS is a table of rows, each naming the kernel instantiation it must reach, the dispatch condition that sends it
there and the knobs that pin it (DESIGN.md "Row-kernel forms under test" holds the same table); plan() transcribes
each entry's host dispatch and tests/test_row_forms_cpu.py holds it against the table and the sources without a
GPU.  The C entries are called directly through _lib on pointers into NaN-pattern buffers, so the test chooses
pointer offsets, splits, workspace sizes, pstride and rows == 0 itself.  Probes, fp64 references and the derived
bounds are in tests/row_probe.py.  Each row is checked these ways (as far as they apply to it):

  exact    inputs whose result is known bit for bit: plane outputs are the documented split of the fp32 form's
           output; L = 1 attention returns V; the "select" probe (one key per query survives __expf) returns
           v[sel(i)] and, backwards, dq = dk = 0 and integer dv; the "uniform" probe (q = 0) returns exact means;
           LayerNorm rows m0 +- 2^k return mean == m0; the fold with power-of-two rstd returns exact products;
           cosine prep leaves the V' half and the other side untouched; integer InstanceNorm inputs give the same
           mu / rstd bits for every splits; backward-prep rows just below / at / above var = 1e-6f take the
           documented branch.
  canary   every operand sits between guards of the quiet-NaN patterns 0x7FC12345 / 0x7FC1: guards intact, inputs
           unchanged, every payload element written and finite, pstride padding and workspace guards intact.
  bound    Gaussian operands, every element within the derived bound of the fp64 reference.
  adjoint  backward entries against fp64 autograd (pos_embed_bwd: W^T g for the dense fp64 resize matrix W).
  repeat   a second call returns the same bits.

Largest kernel error / bound per form (profiles/r28_row_forms_bounds.log, one line per row): fp32 outputs of the passing rows
from 0.001 (vba_hd128_f32_L3) to 0.35 (ln_f32_c256), attention backward at most 0.03; the rows whose bound is a single
rounding sit just under 1 by construction: 0.98 to 0.996 for the fold's one-rounding products (u |ref|), 0.99 for
the InstanceNorm mean (its fp32 store), 0.996 for every bf16 store (the 2^-8 |ref| term).

The file found two defects, both fixed with it:
  * ln_x3_c512 (gauss, 5 rows): the BF16X3 planes of layernorm_kernel<bf16, 8, 1> were not the split of
    layernorm_kernel<float, 8, 0>'s output (an exact check, so no multiple of a bound: the two instantiations were
    contracted into fmas differently and their fp32 values differed in the last bit).  Every output form now shares
    one arithmetic with pinned roundings, the one mhada_layernorm_half2 already had.
  * pos_bwd_8x8_3x5: 9.82 times the adjoint bound gamma(n + 3) |W|^T |g|.  pos_embed_bwd_kernel re-derived the
    forward's fp32 source coordinate and took the weights as its fractional part: an absolute error of a few ulps
    of the coordinate (up to 8 there) in a weight that may be far smaller.  It now keeps the coordinate as the
    integer fraction ((2 o + 1) n - m) / (2 m), so each weight is one rounded quotient.
The forward keeps PyTorch's fp32 coordinate arithmetic, which tests/test_gpu_kernels.py::test_pos_embed pins to 1e-6
of fp32 F.interpolate (the integer-fraction form lies 2.0e-6 from it at 32 x 32 -> 135 x 240).  Its bound therefore
carries the coordinate's rounding, gamma(3) (s + 0.5) times the local neighbour difference of pos
(row_probe.pos_fwd_bound); a first version of this file left that term out, and the forward rows stood at 1.54
(pos_fwd_5x3_11x7), 3.01 (pos_fwd_8x8_3x5) and 1.23 (pos_fwd_1x4_6x9) times gamma(7) |W| |p| alone, as fp32 torch on
the CPU does too (1.52, 3.08).
"""
import math

import pytest
import torch

import row_probe as P

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
if torch.cuda.is_available():
    from mhada_hip import _lib
    DEV = "cuda"
else:  # collection without a GPU: the table is still built (every test here is marked gpu)
    _lib = None
    DEV = "cpu"

NAN32, NAN16 = 0x7FC12345, 0x7FC1  # guard bit patterns (quiet NaNs), as the other forms files
PAD = 256                          # guard elements before and after every buffer (keeps 16-byte alignment)
OK, ERR_ARG = 0, 1
DT_CODE = {F32: 0, BF16: 1}
X3 = 2                             # MHADA_BF16X3
LAYOUTS = [(7, 3), (45, 1)]        # (ntok, heads): 21 pairs (invalid waves / groups), 45 pairs (two vec blocks)
DEFAULT_KNOBS = dict(vit_attn_vec=1)
LOG2E = 1.4426950408889634


# --------------------------------------------------------------------------------------------------
# the form table
# --------------------------------------------------------------------------------------------------
def row(name, kernel, cond, fam, **kw):
    return dict(name=name, kernel=kernel, cond=cond, fam=fam, **kw)


TN = {F32: "float", BF16: "bf16"}
SN = {F32: "f32", BF16: "bf16"}


def _forms():
    f = []
    # ---- mhada_layernorm / mhada_layernorm_half2: rows 1, 5, 131 ------------------------------------------
    for cols in (256, 512, 1024, 2048):
        v = cols // 64
        f.append(row(f"ln_f32_c{cols}", f"layernorm_kernel<float, {v}, 0>", f"mhada_layernorm, y_dtype fp32, cols {cols}",
                     "ln", out="f32", cols=cols))
        f.append(row(f"ln_bf16_c{cols}", f"layernorm_kernel<bf16, {v}, 0>", f"mhada_layernorm, y_dtype bf16, cols {cols}",
                     "ln", out="bf16", cols=cols))
        f.append(row(f"ln_x3_c{cols}", f"layernorm_kernel<bf16, {v}, 1>", f"mhada_layernorm, y_dtype BF16X3, cols {cols}",
                     "ln", out="x3", cols=cols))
        f.append(row(f"ln_h2_c{cols}", f"layernorm_kernel<f16, {v}, 2>", f"mhada_layernorm_half2, cols {cols}",
                     "ln", out="h2", cols=cols))
    # ---- mhada_layernorm_fwd(_split3), mhada_layernorm_bwd ---------------------------------------------------
    for cols in (256, 512, 1024):
        v = cols // 64
        f.append(row(f"ln_train_c{cols}", f"ln_fwd_train_kernel<{v}>", f"mhada_layernorm_fwd, cols {cols} (planes null)",
                     "ln_train", cols=cols, planes=False))
        f.append(row(f"ln_train_s3_c{cols}", f"ln_fwd_train_kernel<{v}>", f"mhada_layernorm_fwd_split3, cols {cols}",
                     "ln_train", cols=cols, planes=True))
        f.append(row(f"ln_bwd_c{cols}", f"ln_bwd_kernel<{v}>", f"mhada_layernorm_bwd, cols {cols}; rows 1, 127, 128, 129, 261; "
                     "generous and exactly minimal workspace", "ln_bwd", cols=cols))
    # ---- mhada_vit_batch_attn ----------------------------------------------------------------------------------
    A = lambda name, kernel, cond, **kw: f.append(row(name, kernel, cond, "attn", **dict(  # noqa: E731
        dict(entry="attn", dt=F32, D=64, L=1, vec=1, qoff=0, ooff=0), **kw)))
    for dt in (F32, BF16):
        for D in (32, 64, 128):
            A(f"vba_copy_{SN[dt]}_d{D}", "vit_batch_copy_v_kernel", f"L = 1, qkv and out 16-byte aligned, {SN[dt]}, head_dim {D}",
              dt=dt, D=D)
    for L in (2, 3, 8):
        A(f"vba_small_f32_L{L}", "vit_batch_attn_small_kernel<float>", f"fp32, head_dim 64, L = {L} <= 8", L=L)
    A("vba_small_f32_L1_misaligned", "vit_batch_attn_small_kernel<float>", "fp32, L = 1, qkv one element off its 16-byte boundary",
      qoff=1)
    A("vba_small_bf16_novec", "vit_batch_attn_small_kernel<bf16>", "bf16, L = 3, vit_attn_vec = 0", dt=BF16, L=3, vec=0)
    A("vba_small_bf16_misaligned", "vit_batch_attn_small_kernel<bf16>", "bf16, L = 5, vit_attn_vec = 1, out one element off",
      dt=BF16, L=5, ooff=1)
    for L in (2, 3, 4):
        A(f"vba_vec4_L{L}", "vit_batch_attn_vec_kernel<bf16, 4>", f"bf16, aligned, vit_attn_vec = 1, L = {L} <= 4", dt=BF16, L=L)
    for L in (5, 8):
        A(f"vba_vec8_L{L}", "vit_batch_attn_vec_kernel<bf16, 8>", f"bf16, aligned, vit_attn_vec = 1, 4 < L = {L} <= 8", dt=BF16, L=L)
    for dt in (F32, BF16):
        for L in (9, 11):
            A(f"vba_online_{SN[dt]}_L{L}", f"vit_batch_attn_kernel<{TN[dt]}>", f"{SN[dt]}, head_dim 64, L = {L} > 8", dt=dt, L=L)
    for D in (32, 128):
        for dt in (F32, BF16):
            for L in (1, 3, 9):
                A(f"vba_hd{D}_{SN[dt]}_L{L}", f"vit_batch_attn_hd_kernel<{TN[dt]}, {D}>",
                  f"head_dim {D}, {SN[dt]}, L = {L}" + (", qkv one element off (no copy)" if L == 1 else ""), dt=dt, D=D, L=L,
                  qoff=1 if L == 1 else 0)
    # ---- plane and backward entries --------------------------------------------------------------------------
    A("vba_s3_copy", "vit_batch_copy_v_s3_kernel", "mhada_vit_batch_attn_split3, L = 1, aligned, pstride % 4 == 0", entry="s3",
      pextra=8)
    A("vba_s3_L1_pstride_odd", "vit_batch_attn_small_s3_kernel", "mhada_vit_batch_attn_split3, L = 1, pstride % 4 != 0", entry="s3",
      pextra=3)
    for L in (2, 8):
        A(f"vba_s3_L{L}", "vit_batch_attn_small_s3_kernel", f"mhada_vit_batch_attn_split3, L = {L}, pstride larger than the output",
          entry="s3", L=L, pextra=40)
    for L in (1, 3, 8):
        A(f"vba_h2_L{L}", "vit_batch_attn_small_h2_kernel", f"mhada_vit_batch_attn_half2, L = {L}", entry="h2", L=L, pextra=24)
    for L in (1, 2, 3, 8):
        A(f"vba_bwd_L{L}", "vit_batch_attn_bwd_kernel", f"mhada_vit_batch_attn_bwd, L = {L} (planes null)", entry="bwd", L=L)
        A(f"vba_bwd_s3_L{L}", "vit_batch_attn_bwd_kernel", f"mhada_vit_batch_attn_bwd_split3, L = {L}, pstride larger than dqkv",
          entry="bwd_s3", L=L, pextra=56)
    # ---- positional embedding ----------------------------------------------------------------------------------
    for (src, dst) in P.POS_SIZES:
        tag = f"{src[0]}x{src[1]}_{dst[0]}x{dst[1]}"
        what = "equal sizes: the copy branch" if src == dst else f"({src[0]}, {src[1]}) -> ({dst[0]}, {dst[1]})"
        f.append(row(f"pos_fwd_{tag}", "pos_embed_kernel", f"mhada_pos_embed, {what}; C 5 and 64", "pos", bwd=False, src=src, dst=dst))
        f.append(row(f"pos_bwd_{tag}", "pos_embed_bwd_kernel", f"mhada_pos_embed_bwd, {what}; C 5 and 64", "pos", bwd=True, src=src,
                     dst=dst))
    # ---- InstanceNorm ----------------------------------------------------------------------------------------
    for C in (4, 68, 132):
        cond = f"C {C}; N 1, 15, 17, 33; B 1, 3; splits 1, 3, 16, 17, 40"
        f.append(row(f"in_stats_c{C}", "in_partial_kernel + in_finalize_kernel", "mhada_instnorm_stats, " + cond, "in", bwd=False, C=C))
        f.append(row(f"in_bwd_c{C}", "inb_partial_kernel + inb_finalize_kernel + inb_apply_kernel", "mhada_instnorm_bwd, " + cond,
                     "in", bwd=True, C=C))
    # ---- fold, cosine prep, backward prep ------------------------------------------------------------------------
    for dt in (F32, BF16):
        for (B, H) in ((1, 1), (2, 3)):
            for ks, kn in ((LOG2E, "log2e"), (1.0, "1")):
                f.append(row(f"fold_{SN[dt]}_b{B}h{H}_k{kn}", f"fold_kernel<{TN[dt]}>", f"mhada_fold_block, {SN[dt]}, B {B} H {H}, "
                             f"kscale {kn}", "fold", dt=dt, B=B, H=H, kscale=ks))
        for side, ld in (("q", "64"), ("kv", "128"), ("both", "64 and 128")):
            f.append(row(f"cosprep_{SN[dt]}_{side}", f"rownorm_kernel<{TN[dt]}>", f"mhada_cosine_prep, {SN[dt]}, "
                         + {"q": "Ns == 0 (q only)", "kv": "Nc == 0 (kv only)", "both": "q and kv"}[side] + f", ld {ld}; 1 and 7 rows",
                         "cosprep", dt=dt, side=side))
    for D in (32, 64, 128):
        f.append(row(f"bwd_prep_d{D}", f"attn_bwd_prep_kernel<{D}>", ("mhada_attn_train_bwd_prep" if D == 64 else
                     f"mhada_attn_train_bwd_prep_hd, D {D}") + "; rows 1, 7, 9", "prep", D=D))
    return f


FORMS = [pytest.param(fm, id=fm["name"]) for fm in _forms()]


def plan(fm):
    """The kernel each entry's host code launches for the row's arguments (a transcription of the dispatch in
    csrc/small_ops.hip, csrc/train_ops.hip and csrc/attn_hd.hip)."""
    fam = fm["fam"]
    if fam == "ln":
        assert fm["cols"] in (256, 512, 1024, 2048)
        v = fm["cols"] // 64
        return {"f32": f"layernorm_kernel<float, {v}, 0>", "bf16": f"layernorm_kernel<bf16, {v}, 0>",
                "x3": f"layernorm_kernel<bf16, {v}, 1>", "h2": f"layernorm_kernel<f16, {v}, 2>"}[fm["out"]]
    if fam in ("ln_train", "ln_bwd"):
        assert fm["cols"] in (256, 512, 1024)
        return ("ln_fwd_train_kernel<%d>" if fam == "ln_train" else "ln_bwd_kernel<%d>") % (fm["cols"] // 64)
    if fam == "attn":
        e, dt, D, L = fm["entry"], fm["dt"], fm["D"], fm["L"]
        esz = 4 if dt == F32 else 2
        q_al, o_al = (fm["qoff"] * esz) % 16 == 0, (fm["ooff"] * esz) % 16 == 0
        if e == "attn":
            if L == 1 and q_al and o_al:
                return "vit_batch_copy_v_kernel"
            if D != 64:
                return f"vit_batch_attn_hd_kernel<{TN[dt]}, {D}>"
            if L <= 8:
                if dt != F32 and fm["vec"] and q_al and o_al:
                    return "vit_batch_attn_vec_kernel<bf16, %d>" % (4 if L <= 4 else 8)
                return f"vit_batch_attn_small_kernel<{TN[dt]}>"
            return f"vit_batch_attn_kernel<{TN[dt]}>"
        assert D == 64 and L <= 8
        if e == "s3":
            return "vit_batch_copy_v_s3_kernel" if L == 1 and q_al and o_al and pstride_of(fm, LAYOUTS[0]) % 4 == 0 \
                and pstride_of(fm, LAYOUTS[1]) % 4 == 0 else "vit_batch_attn_small_s3_kernel"
        return "vit_batch_attn_small_h2_kernel" if e == "h2" else "vit_batch_attn_bwd_kernel"
    if fam == "pos":
        return "pos_embed_bwd_kernel" if fm["bwd"] else "pos_embed_kernel"
    if fam == "in":
        assert fm["C"] % 4 == 0
        return "inb_partial_kernel + inb_finalize_kernel + inb_apply_kernel" if fm["bwd"] else "in_partial_kernel + in_finalize_kernel"
    if fam == "fold":
        return f"fold_kernel<{TN[fm['dt']]}>"
    if fam == "cosprep":
        return f"rownorm_kernel<{TN[fm['dt']]}>"
    assert fm["D"] in (32, 64, 128)
    return f"attn_bwd_prep_kernel<{fm['D']}>"


def pstride_of(fm, layout):
    ntok, heads = layout
    n = fm["L"] * ntok * heads * 64 * (3 if fm["entry"] == "bwd_s3" else 1)
    return n + fm.get("pextra", 0)


# every instantiation the entries can launch (test_row_forms_cpu.py reads the same list off the sources)
INSTANTIATIONS = sorted({p.values[0]["kernel"] for p in FORMS})


# --------------------------------------------------------------------------------------------------
# NaN-pattern buffers and calls
# --------------------------------------------------------------------------------------------------
class Buf:
    """A tensor of `shape` inside a flat NaN-pattern buffer: PAD + off pattern elements before it, PAD after."""

    def __init__(self, dtype, shape, src=None, off=0):
        self.dtype, self.shape, self.off = dtype, tuple(shape), PAD + off
        self.n = math.prod(self.shape)
        self.idt, self.pat, self.w = {F32: (torch.int32, NAN32, 1), F64: (torch.int32, NAN32, 2)}.get(dtype, (torch.int16, NAN16, 1))
        self.raw = torch.empty((self.n + self.off + PAD) * self.w, dtype=self.idt, device=DEV)
        self.src = None
        self.reset()
        if src is not None:
            self.src = src.reshape(self.shape).to(dtype).to(DEV)
            self.t.copy_(self.src)

    def reset(self):
        self.raw.fill_(self.pat)
        if self.src is not None:
            self.t.copy_(self.src)

    @property
    def flat(self):
        return self.raw.view(self.dtype)

    @property
    def t(self):
        return self.flat[self.off:self.off + self.n].view(self.shape)

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.off * self.flat.element_size()

    def cpu(self):
        return self.t.detach().cpu().clone()

    def guards_intact(self):
        a, b = self.off * self.w, (self.off + self.n) * self.w
        return bool((self.raw[:a] == self.pat).all()) and bool((self.raw[b:] == self.pat).all())

    def unchanged(self):
        return self.guards_intact() and torch.equal(self.t, self.src)

    def untouched(self, sl):
        """The payload elements flat[sl] (relative to the payload) still hold the pattern."""
        return bool((self.raw[self.off * self.w:(self.off + self.n) * self.w][sl] == self.pat).all())


def rc_of(name, *args):
    return getattr(_lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    _lib.check(rc_of(name, *args), name)
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


class Worst:
    def __init__(self, fm):
        self.fm, self.w = fm, 0.0

    def hold(self, got, ref, bound, what):
        """Every element finite and within the bound of the reference."""
        got = got.double()
        assert bool(torch.isfinite(got).all()), f"{self.fm['name']} {what}: an element not written, or not finite"
        err = (got - ref).abs()
        ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, math.inf).double()).max().item() if got.numel() else 0.0
        print(f"RATIO {self.fm['name']:30s} {what:44s} {ratio:.4f}")
        self.w = max(self.w, ratio)
        assert ratio <= 1.0, f"{self.fm['name']} {what}: error / bound = {ratio:.3f}"


def ins_ok(what, *bufs):
    for b in bufs:
        assert b.unchanged(), what + ": an input was written"


def twice(fn, outs, what):
    """Run fn on freshly pattern-filled outputs twice: guards intact, identical bits.  Returns the CPU copies."""
    res = []
    for _ in range(2):
        for o in outs:
            o.reset()
        fn()
        for o in outs:
            assert o.guards_intact(), what + ": written outside an output"
        res.append([o.cpu() for o in outs])
    for a, b in zip(*res):
        assert same_bits(a, b), what + ": a second call returned other bits"
    return res[0]


# --------------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------------
def ln_call(out, x, g, b, rows, cols, scale=1.0):
    """One inference LayerNorm call; returns the y buffer ([rows][cols], or [planes][rows][cols])."""
    kind = {"f32": (F32, 1), "bf16": (BF16, 1), "x3": (BF16, 3), "h2": (F16, 2)}[out]
    y = Buf(kind[0], (kind[1], rows, cols) if kind[1] > 1 else (rows, cols))

    def fn():
        if out == "h2":
            call("mhada_layernorm_half2", x.ptr, y.ptr, g.ptr, b.ptr, rows, cols, P.LN_EPS, scale)
        else:
            call("mhada_layernorm", x.ptr, y.ptr, {"f32": 0, "bf16": 1, "x3": X3}[out], g.ptr, b.ptr, rows, cols, P.LN_EPS)
    return twice(fn, [y], f"ln {out} {rows}x{cols}")[0]


def run_ln(fm, w):
    out, cols = fm["out"], fm["cols"]
    cases = [(rows, kind, 0.0) for rows in (1, 5, 131) for kind in ("exact", "gauss")]
    if cols == 512 and out in ("f32", "x3", "h2"):
        cases.append((5, "gauss", 1000.0))
    for rows, kind, offset in cases:
        what = f"{kind} rows {rows}" + (" offset 1000" if offset else "")
        xs, gs, bs = P.ln_exact(rows, cols)[:3] if kind == "exact" else P.ln_gauss(rows, cols, offset, seed=rows)
        scale = 4.0 if kind == "exact" else 64.0
        x, g, b = Buf(F32, (rows, cols), xs), Buf(F32, (cols,), gs), Buf(F32, (cols,), bs)
        y = ln_call(out, x, g, b, rows, cols, scale)
        ins_ok(fm["name"] + " " + what, x, g, b)
        r = P.ln_ref(xs, gs, bs)
        bd = P.ln_bound(xs, gs, r, bf16_out=out == "bf16")["y"]
        if out in ("f32", "bf16"):
            w.hold(y, r["y"], bd, what)
            continue
        y32 = ln_call("f32", x, g, b, rows, cols)
        if out == "x3":  # the documented split of the fp32 form's output, bit for bit
            assert same_bits(y, P.split3(y32)), f"{fm['name']} {what}: planes are not the split of the fp32 form's output"
            w.hold(y.float().double().sum(0), r["y"], bd + 2.0 ** -23 * r["y"].abs(), what + " (p0 + p1 + p2)")
        else:
            if cols == 512:  # the kernel's own claim: bit-identical to the fp32 form at cols = 512
                assert same_bits(y, P.half2(y32, scale)), f"{fm['name']} {what}: planes are not the split of the fp32 form's output"
            plane = 2.0 ** -21 * r["y"].abs() + 2 * 6.103515625e-05 / scale
            w.hold(y.float().double().sum(0) / scale, r["y"], bd + plane, what + " ((hi + lo) / scale)")


def test_ln_rows_zero_and_bad_cols():
    x, g, b = Buf(F32, (4, 512)), Buf(F32, (512,)), Buf(F32, (512,))
    for out in ("f32", "bf16", "x3"):
        y = Buf(BF16 if out != "f32" else F32, (3, 4, 512))
        assert rc_of("mhada_layernorm", x.ptr, y.ptr, {"f32": 0, "bf16": 1, "x3": X3}[out], g.ptr, b.ptr, 0, 512, P.LN_EPS) == OK
        torch.cuda.synchronize()
        assert y.untouched(slice(None)) and y.guards_intact(), "rows == 0 wrote something"
        assert rc_of("mhada_layernorm", x.ptr, y.ptr, {"f32": 0, "bf16": 1, "x3": X3}[out], g.ptr, b.ptr, 4, 320, P.LN_EPS) == ERR_ARG
    y = Buf(F16, (2, 4, 512))
    assert rc_of("mhada_layernorm_half2", x.ptr, y.ptr, g.ptr, b.ptr, 0, 512, P.LN_EPS, 4.0) == OK
    assert rc_of("mhada_layernorm_half2", x.ptr, y.ptr, g.ptr, b.ptr, 4, 320, P.LN_EPS, 4.0) == ERR_ARG
    torch.cuda.synchronize()
    assert y.untouched(slice(None)) and y.guards_intact()


def ln_train_call(x, g, b, rows, cols, planes):
    y, st = Buf(F32, (rows, cols)), Buf(F32, (rows, 2))
    outs = [y, st]
    if planes:
        pl = Buf(BF16, (3, rows, cols))
        outs.append(pl)
        fn = lambda: call("mhada_layernorm_fwd_split3", x.ptr, y.ptr, pl.ptr, st.ptr, g.ptr, b.ptr, rows, cols, P.LN_EPS)  # noqa: E731
    else:
        fn = lambda: call("mhada_layernorm_fwd", x.ptr, y.ptr, st.ptr, g.ptr, b.ptr, rows, cols, P.LN_EPS)  # noqa: E731
    return twice(fn, outs, f"ln_train {rows}x{cols}")


def run_ln_train(fm, w):
    cols = fm["cols"]
    cases = [(rows, kind, 0.0) for rows in (1, 5, 131) for kind in ("exact", "gauss")]
    if cols == 512:
        cases.append((5, "gauss", 1000.0))
    for rows, kind, offset in cases:
        what = f"{kind} rows {rows}" + (" offset 1000" if offset else "")
        ex = P.ln_exact(rows, cols)
        xs, gs, bs = ex[:3] if kind == "exact" else P.ln_gauss(rows, cols, offset, seed=rows)
        x, g, b = Buf(F32, (rows, cols), xs), Buf(F32, (cols,), gs), Buf(F32, (cols,), bs)
        res = ln_train_call(x, g, b, rows, cols, fm["planes"])
        ins_ok(fm["name"] + " " + what, x, g, b)
        r = P.ln_ref(xs, gs, bs)
        bd = P.ln_bound(xs, gs, r)
        w.hold(res[0], r["y"], bd["y"], what + " y")
        w.hold(res[1][:, 0], r["mean"], bd["mean"], what + " mean")
        w.hold(res[1][:, 1], r["rstd"], bd["rstd"], what + " rstd")
        if kind == "exact":
            assert same_bits(res[1][:, 0], ex[3].float()), f"{fm['name']} {what}: mean != m0"
            w.hold(res[1][:, 1], (torch.pow(4.0, ex[4]) + P.LN_EPS).rsqrt(), bd["rstd"], what + " rstd vs (4^k + eps)^-1/2")
        if fm["planes"]:  # the split of this entry's own y, and y is the plane-less entry's
            assert same_bits(res[2], P.split3(res[0])), f"{fm['name']} {what}: planes are not the split of y"
            base = ln_train_call(x, g, b, rows, cols, False)
            assert same_bits(base[0], res[0]) and same_bits(base[1], res[1]), f"{fm['name']} {what}: y / stats differ from mhada_layernorm_fwd"


def run_ln_bwd(fm, w):
    cols = fm["cols"]
    for rows in (1, 127, 128, 129, 261):
        what = f"rows {rows}"
        xs, gs, bs = P.ln_gauss(rows, cols, seed=rows)
        dys = P.randn(rows, cols, seed=900 + rows)
        r = P.ln_ref(xs, gs, bs)
        # the stats the backward is handed: the fp64 ones rounded to fp32 (the bound allows for that rounding)
        sts = torch.stack([r["mean"], r["rstd"]], 1)
        x, dy, g, st = Buf(F32, (rows, cols), xs), Buf(F32, (rows, cols), dys), Buf(F32, (cols,), gs), Buf(F32, (rows, 2), sts)
        need = (-(-rows // 128) * 2 + 2) * cols
        dx, dg, db = Buf(F32, (rows, cols)), Buf(F32, (cols,)), Buf(F32, (cols,))
        got = {}
        for label, wf in (("generous", need + 4 * cols + 64), ("minimal", need)):
            work = Buf(F32, (wf,))
            fn = lambda: call("mhada_layernorm_bwd", x.ptr, dy.ptr, st.ptr, g.ptr, dx.ptr, dg.ptr, db.ptr, work.ptr, wf, rows, cols)  # noqa: E731
            got[label] = twice(fn, [dx, dg, db, work], f"{fm['name']} {what} {label}")[:3]
            assert work.guards_intact(), f"{fm['name']} {what} {label}: workspace guard"
        for a, b_ in zip(got["generous"], got["minimal"]):
            assert same_bits(a, b_), f"{fm['name']} {what}: the minimal workspace returned other bits"
        work = Buf(F32, (need,))
        assert rc_of("mhada_layernorm_bwd", x.ptr, dy.ptr, st.ptr, g.ptr, dx.ptr, dg.ptr, db.ptr, work.ptr, need - 1, rows, cols) == ERR_ARG
        torch.cuda.synchronize()
        ins_ok(fm["name"] + " " + what, x, dy, g, st)
        ref, bd = P.ln_bwd_ref(xs, dys, gs), P.ln_bwd_bound(xs, dys, gs, r)
        for name, t in zip(("dx", "dgamma", "dbeta"), got["minimal"]):
            w.hold(t, ref[name], bd[name], f"{what} {name}")


# --------------------------------------------------------------------------------------------------
# batch-axis attention
# --------------------------------------------------------------------------------------------------
def attn_forward(fm, layout, qkv_src):
    """One forward call of the row's entry; returns (out fp32-or-bf16 [L][ntok][C] or planes, qkv buffer)."""
    ntok, heads = layout
    e, dt, D, L = fm["entry"], fm["dt"], fm["D"], fm["L"]
    C = heads * D
    qkv = Buf(dt, (L, ntok, 3, heads, D), qkv_src, off=fm["qoff"])
    what = f"{fm['name']} {ntok}x{heads}"
    if e == "attn":
        out = Buf(dt, (L, ntok, C), off=fm["ooff"])
        fn = lambda: call("mhada_vit_batch_attn", qkv.ptr, out.ptr, DT_CODE[dt], L, ntok, heads, D)  # noqa: E731
        res = twice(fn, [out], what)[0]
    else:
        ps, n = pstride_of(fm, layout), L * ntok * C
        np_ = 3 if e == "s3" else 2
        out = Buf(BF16 if e == "s3" else F16, ((np_ - 1) * ps + n,))
        osc = Buf(F32, (C,), torch.pow(2.0, (torch.arange(C) % 4).double()))
        if e == "s3":
            fn = lambda: call("mhada_vit_batch_attn_split3", qkv.ptr, out.ptr, ps, L, ntok, heads, D)  # noqa: E731
        else:
            fn = lambda: call("mhada_vit_batch_attn_half2", qkv.ptr, out.ptr, ps, osc.ptr, L, ntok, heads, D)  # noqa: E731
        flat = twice(fn, [out], what)[0]
        for p in range(np_ - 1):  # the padding between the payload and the next plane
            assert out.untouched(slice(p * ps + n, (p + 1) * ps)), what + ": pstride padding written"
        res = torch.stack([flat[p * ps:p * ps + n] for p in range(np_)]).view(np_, L, ntok, C)
        assert osc.unchanged()
    assert qkv.unchanged(), what + ": qkv was written"
    return res


def fp32_form_output(fm, layout, qkv_src):
    base = dict(fm, entry="attn", dt=F32, qoff=0, ooff=0)
    return attn_forward(base, layout, qkv_src)


def out_scale(C):
    return torch.pow(2.0, (torch.arange(C) % 4).double()).float()


def check_forward(fm, layout, qkv_src, w, what, exact=None):
    """exact: the fp64 tensor the fp32 / bf16 output must equal bit for bit (None: bound check)."""
    e, dt = fm["entry"], fm["dt"]
    L, ntok = fm["L"], layout[0]
    C = layout[1] * fm["D"]
    got = attn_forward(fm, layout, qkv_src)
    qr = qkv_src.to(dt).double()
    if e == "attn":
        if exact is not None:
            assert same_bits(got, exact.to(dt)), f"{fm['name']} {what}: not the exact result"
        else:
            w.hold(got, P.attn_ref(qr), P.attn_bound(qr, bf16_out=dt == BF16), what)
        return
    y32 = fp32_form_output(fm, layout, qkv_src)
    if exact is not None:
        assert same_bits(y32, exact.float()), f"{fm['name']} {what}: the fp32 form is not exact"
    else:
        w.hold(y32, P.attn_ref(qr), P.attn_bound(qr), what + " (fp32 form)")
    want = P.split3(y32) if e == "s3" else P.half2(y32 * out_scale(C), 1.0)
    assert same_bits(got, want), f"{fm['name']} {what}: planes are not the split of the fp32 form's output"


def check_backward(fm, layout, qkv_src, dout_src, w, what, exact=None):
    """exact: the fp64 dqkv the result must equal (None: bound check against fp64 autograd)."""
    ntok, heads = layout
    L, C = fm["L"], heads * 64
    qkv, dout = Buf(F32, (L, ntok, 3, heads, 64), qkv_src), Buf(F32, (L, ntok, C), dout_src)
    dq = Buf(F32, (L, ntok, 3, heads, 64))
    outs = [dq]
    n = L * ntok * 3 * C
    if fm["entry"] == "bwd_s3":
        ps = pstride_of(fm, layout)
        pl = Buf(BF16, (2 * ps + n,))
        outs.append(pl)
        fn = lambda: call("mhada_vit_batch_attn_bwd_split3", qkv.ptr, dout.ptr, dq.ptr, pl.ptr, ps, L, ntok, heads, 64)  # noqa: E731
    else:
        fn = lambda: call("mhada_vit_batch_attn_bwd", qkv.ptr, dout.ptr, dq.ptr, L, ntok, heads, 64)  # noqa: E731
    res = twice(fn, outs, f"{fm['name']} {what}")
    ins_ok(f"{fm['name']} {what}", qkv, dout)
    got = res[0]
    if fm["entry"] == "bwd_s3":
        for p in range(2):
            assert pl.untouched(slice(p * ps + n, (p + 1) * ps)), f"{fm['name']} {what}: pstride padding written"
        planes = torch.stack([res[1][p * ps:p * ps + n] for p in range(3)]).view(3, *got.shape)
        assert same_bits(planes, P.split3(got)), f"{fm['name']} {what}: planes are not the split of dqkv"
    if exact is not None:
        assert bool((got.double() == exact).all()), f"{fm['name']} {what}: not the exact gradient"
    else:
        w.hold(got, P.attn_bwd_ref(qkv_src, dout_src), P.attn_bwd_bound(qkv_src, dout_src), what)
    return got


def run_attn(fm, w):
    e, dt, D, L = fm["entry"], fm["dt"], fm["D"], fm["L"]
    with _lib.tuning(vit_attn_vec=fm["vec"]):
        for layout in LAYOUTS:
            ntok, heads = layout
            lay = f"{ntok}x{heads}"
            gauss = P.attn_gauss(L, ntok, heads, D, seed=L)
            if e in ("bwd", "bwd_s3"):
                dout = P.randn(L, ntok, heads * D, seed=950 + L)
                got = check_backward(fm, layout, gauss, dout, w, f"{lay} gauss")
                if L == 1:  # dv = dout, dq = dk = 0
                    assert bool((got[:, :, :2] == 0).all()) and same_bits(got[:, :, 2].reshape(dout.shape), dout.float())
                else:
                    sel_qkv, sel = P.attn_select(L, ntok, heads, D)
                    idout = P.int_dout(L, ntok, heads, D)
                    check_backward(fm, layout, sel_qkv, idout, w, f"{lay} select", exact=P.select_bwd_exact(sel, idout, heads, D))
                if L in (2, 4, 8):  # every term a dyadic rational: the fp64 autograd result is exact, and so must fp32 be
                    uni, idout = P.attn_uniform(L, ntok, heads, D), P.int_dout(L, ntok, heads, D)
                    check_backward(fm, layout, uni, idout, w, f"{lay} uniform", exact=P.attn_bwd_ref(uni, idout))
                continue
            if L == 1:  # V bit for bit, whichever kernel ran
                v = gauss.to(dt).double()[:, :, 2].reshape(1, ntok, heads * D)
                check_forward(fm, layout, gauss, w, f"{lay} L = 1", exact=v)
                continue
            check_forward(fm, layout, gauss, w, f"{lay} gauss")
            sel_qkv, sel = P.attn_select(L, ntok, heads, D, bf16=dt == BF16)
            v = sel_qkv[:, :, 2]                                                   # [L][ntok][heads][D]
            want = torch.gather(v, 0, sel[..., None].expand(L, ntok, heads, D)).reshape(L, ntok, heads * D)
            check_forward(fm, layout, sel_qkv, w, f"{lay} select", exact=want)
            if L in (2, 4, 8):
                uni = P.attn_uniform(L, ntok, heads, D)
                check_forward(fm, layout, uni, w, f"{lay} uniform", exact=P.attn_ref(uni))


def test_attn_refusals():
    ntok, heads, C = 7, 3, 192
    qkv, out = Buf(F32, (9, ntok, 3 * C)), Buf(BF16, (3 * 9 * ntok * 3 * C + 64,))
    dout, dq, osc = Buf(F32, (9, ntok, C)), Buf(F32, (9, ntok, 3 * C)), Buf(F32, (C,))
    n = 2 * ntok * C
    cases = [
        ("mhada_vit_batch_attn", (qkv.ptr, out.ptr, 0, 2, ntok, heads, 48)),                       # head_dim 48
        ("mhada_vit_batch_attn_split3", (qkv.ptr, out.ptr, 9 * ntok * C, 9, ntok, heads, 64)),     # L = 9
        ("mhada_vit_batch_attn_split3", (qkv.ptr, out.ptr, n, 2, ntok, heads, 48)),
        ("mhada_vit_batch_attn_split3", (qkv.ptr, out.ptr, n - 1, 2, ntok, heads, 64)),            # pstride too small
        ("mhada_vit_batch_attn_half2", (qkv.ptr, out.ptr, 9 * ntok * C, osc.ptr, 9, ntok, heads, 64)),
        ("mhada_vit_batch_attn_half2", (qkv.ptr, out.ptr, n, osc.ptr, 2, ntok, heads, 48)),
        ("mhada_vit_batch_attn_half2", (qkv.ptr, out.ptr, n - 1, osc.ptr, 2, ntok, heads, 64)),
        ("mhada_vit_batch_attn_bwd", (qkv.ptr, dout.ptr, dq.ptr, 9, ntok, heads, 64)),
        ("mhada_vit_batch_attn_bwd", (qkv.ptr, dout.ptr, dq.ptr, 2, ntok, heads, 48)),
        ("mhada_vit_batch_attn_bwd_split3", (qkv.ptr, dout.ptr, dq.ptr, out.ptr, 27 * ntok * C, 9, ntok, heads, 64)),
        ("mhada_vit_batch_attn_bwd_split3", (qkv.ptr, dout.ptr, dq.ptr, out.ptr, 3 * n, 2, ntok, heads, 48)),
        ("mhada_vit_batch_attn_bwd_split3", (qkv.ptr, dout.ptr, dq.ptr, out.ptr, 3 * n - 1, 2, ntok, heads, 64)),
    ]
    for name, args in cases:
        assert rc_of(name, *args) == ERR_ARG, (name, args[2:])
    torch.cuda.synchronize()
    for b in (out, dq):
        assert b.untouched(slice(None)) and b.guards_intact(), "a refused call wrote something"


# --------------------------------------------------------------------------------------------------
# positional embedding
# --------------------------------------------------------------------------------------------------
def run_pos(fm, w):
    (bh, bw), (oh, ow) = fm["src"], fm["dst"]
    W = P.resize_matrix(bh, bw, oh, ow)
    for C in (5, 64):
        what = f"C {C}"
        if not fm["bwd"]:
            ps = P.randn(C, bh, bw, seed=C)
            pos, out = Buf(F32, (C, bh, bw), ps), Buf(F32, (oh * ow, C))
            got = twice(lambda: call("mhada_pos_embed", pos.ptr, out.ptr, C, bh, bw, oh, ow), [out], fm["name"])[0]
            ins_ok(fm["name"], pos)
            if (bh, bw) == (oh, ow):
                assert same_bits(got, ps.reshape(C, -1).t().float()), fm["name"] + ": the copy branch is not a copy"
            w.hold(got, P.pos_fwd(ps, W), P.pos_fwd_bound(ps, W, (oh, ow)), what)
        else:
            gs = P.randn(oh * ow, C, seed=10 + C)
            g, gp = Buf(F32, (oh * ow, C), gs), Buf(F32, (C, bh * bw))
            got = twice(lambda: call("mhada_pos_embed_bwd", g.ptr, gp.ptr, C, bh, bw, oh, ow), [gp], fm["name"])[0]
            ins_ok(fm["name"], g)
            zero = (W != 0).sum(0) == 0
            assert bool((bits(got)[:, zero] == 0).all()), fm["name"] + ": a source pixel no target reads is not +0.0"
            w.hold(got, P.pos_bwd(gs, W), P.pos_bwd_bound(gs, W), what)


# --------------------------------------------------------------------------------------------------
# InstanceNorm
# --------------------------------------------------------------------------------------------------
SPLITS = (1, 3, 16, 17, 40)


def run_in(fm, w):
    C = fm["C"]
    for B in (1, 3):
        for N in (1, 15, 17, 33):
            kinds = [("gauss", 0.0), ("int", 0.0)] + ([("gauss", 1000.0)] if (B, N) == (3, 33) else [])
            for kind, offset in kinds:
                if kind == "int":  # 16 N max|x|^2 <= 16 33 2^20 < 2^53: the fp64 sums are exact for any splits
                    idx = torch.arange(B * N * C).view(B, N, C)
                    xs = ((idx * 7919) % 2047 - 1023).double()
                    dys = ((idx * 31) % 17 - 8).double()
                else:
                    xs = (P.randn(B, N, C, seed=N + B) * 2 + P.randn(B, 1, C, seed=50 + N) + offset).float().double()
                    dys = P.randn(B, N, C, seed=70 + N + B)
                ref = P.in_ref(xs)
                first = None
                for splits in SPLITS:
                    what = f"B {B} N {N} {kind}{' offset 1000' if offset else ''} splits {splits}"
                    if not fm["bwd"]:
                        x, mu, rs = Buf(F32, (B, N, C), xs), Buf(F32, (B, C)), Buf(F32, (B, C))
                        work = Buf(F64, (splits * B * C * 2,))
                        got = twice(lambda: call("mhada_instnorm_stats", x.ptr, mu.ptr, rs.ptr, work.ptr, B, N, C, splits, P.IN_EPS),
                                    [mu, rs, work], fm["name"] + " " + what)[:2]
                        ins_ok(fm["name"] + " " + what, x)
                        bd = P.in_bound(xs, ref)
                        w.hold(got[0], ref["mu"], bd["mu"], what + " mu")
                        w.hold(got[1], ref["rstd"], bd["rstd"], what + " rstd")
                    else:
                        ys = ((xs - ref["mu"][:, None]) * ref["rstd"][:, None]).float().double() if kind != "int" else \
                            ((torch.arange(B * N * C).view(B, N, C) * 13) % 9 - 4).double()
                        rss = ref["rstd"].float().double() if kind != "int" else torch.pow(2.0, (torch.arange(B * C).view(B, C) % 3).double())
                        dy, y, rs, dx = Buf(F32, (B, N, C), dys), Buf(F32, (B, N, C), ys), Buf(F32, (B, C), rss), Buf(F32, (B, N, C))
                        work = Buf(F64, (splits * B * C * 2 + B * C,))  # + B C 2 floats
                        got = twice(lambda: call("mhada_instnorm_bwd", dy.ptr, y.ptr, rs.ptr, dx.ptr, work.ptr, B, N, C, splits),
                                    [dx, work], fm["name"] + " " + what)[:1]
                        ins_ok(fm["name"] + " " + what, dy, y, rs)
                        w.hold(got[0], P.in_bwd_ref(dys, ys, rss), P.in_bwd_bound(dys, ys, rss), what + " dx")
                    if kind == "int":
                        first = first or got
                        for a, b_ in zip(first, got):
                            assert same_bits(a, b_), f"{fm['name']} {what}: bits depend on splits"


# --------------------------------------------------------------------------------------------------
# fold, cosine prep, backward prep
# --------------------------------------------------------------------------------------------------
def run_fold(fm, w):
    dt, B, H, ks = fm["dt"], fm["B"], fm["H"], fm["kscale"]
    ksf = float(torch.tensor(ks, dtype=F32))
    for exact in (False,) + ((True,) if ks == 1.0 else ()):
        what = "pow2" if exact else "gauss"
        o = P.fold_operands(B, H, exact, seed=B + H)
        names = ("wf", "wg", "wh", "bg", "bh", "rstd_c", "mu_s", "rstd_s")
        ins = [Buf(F32, o[n].shape, o[n]) for n in names]
        wq, wkv = Buf(dt, (B, H, 64, 64)), Buf(dt, (B, H, 128, 64))
        bkv, vmu = Buf(F32, (H * 128,)), Buf(F32, (B, H * 64))
        got = twice(lambda: call("mhada_fold_block", *[b.ptr for b in ins], wq.ptr, wkv.ptr, bkv.ptr, vmu.ptr, ks, DT_CODE[dt], B, H),
                    [wq, wkv, bkv, vmu], fm["name"] + " " + what)
        ins_ok(fm["name"] + " " + what, *ins)
        r = P.fold_ref(o, ksf, B, H)
        bd = P.fold_bound(r, dt == BF16)
        for name, t in zip(("wq", "wkv", "bkv", "v_mu"), got):
            w.hold(t, r[name], bd[name], f"{what} {name}")
        # the V half is wh (bf16: its rounding), bkv's V half is +0.0
        assert same_bits(got[1][:, :, 64:], o["wh"].to(dt)[None].expand(B, H, 64, 64).contiguous()), fm["name"] + ": V half is not wh"
        assert bool((bits(got[2]).view(H, 128)[:, 64:] == 0).all()), fm["name"] + ": bkv[:, 64:] is not +0.0"
        if exact:
            assert same_bits(got[0], r["wq"].to(dt)) and same_bits(got[1], r["wkv"].to(dt)), fm["name"] + ": exact products"


def run_cosprep(fm, w):
    dt, side = fm["dt"], fm["side"]
    for (B, H, N) in ((1, 1, 1), (1, 7, 1), (1, 1, 7)):
        what = f"B {B} H {H} N {N}"
        qs, kvs = P.randn(B, H, N, 64, seed=N + H), P.randn(B, H, N, 128, seed=20 + N + H)
        q, kv = Buf(dt, qs.shape, qs), Buf(dt, kvs.shape, kvs)
        Nc, Ns = (N if side != "kv" else 0), (N if side != "q" else 0)
        qa, ka = (q.ptr if Nc else None), (kv.ptr if Ns else None)
        runs = []
        for _ in range(2):  # in place: restore the operands before each call
            q.reset()
            kv.reset()
            call("mhada_cosine_prep", qa, ka, DT_CODE[dt], B, H, Nc, Ns)
            assert q.guards_intact() and kv.guards_intact(), fm["name"] + ": written outside the rows"
            runs.append((q.cpu(), kv.cpu()))
        assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), fm["name"] + ": a second call returned other bits"
        gq, gkv = runs[0]
        assert same_bits(gkv[..., 64:], kvs.to(dt)[..., 64:].contiguous()), f"{fm['name']} {what}: the V' half changed"
        if Nc:
            ref = P.rownorm_ref(qs.to(dt).double())
            w.hold(gq, ref, P.rownorm_bound(ref, dt == BF16), what + " q")
        else:
            assert same_bits(gq, qs.to(dt)), f"{fm['name']} {what}: q changed in a kv-only call"
        if Ns:
            ref = P.rownorm_ref(kvs.to(dt).double()[..., :64])
            w.hold(gkv[..., :64], ref, P.rownorm_bound(ref, dt == BF16), what + " k")
        else:
            assert same_bits(gkv, kvs.to(dt)), f"{fm['name']} {what}: kv changed in a q-only call"


def prep_call(D, ops4, rows, what):
    dout, x, m, e2 = ops4
    ins = [Buf(F32, (rows, D), dout), Buf(F32, (rows, D), x), Buf(F32, (rows, 2 * D), torch.cat([m, e2], 1))]
    dx, dmo, dd = Buf(F32, (rows, D)), Buf(F32, (rows, 2 * D)), Buf(F32, (rows,))
    if D == 64:
        fn = lambda: call("mhada_attn_train_bwd_prep", *[b.ptr for b in ins], dx.ptr, dmo.ptr, dd.ptr, rows)  # noqa: E731
    else:
        fn = lambda: call("mhada_attn_train_bwd_prep_hd", *[b.ptr for b in ins], dx.ptr, dmo.ptr, dd.ptr, rows, D)  # noqa: E731
    got = twice(fn, [dx, dmo, dd], what)
    ins_ok(what, *ins)
    return dict(dx=got[0], dm=got[1][:, :D], dvar=got[1][:, D:], dd=got[2])


def run_prep(fm, w):
    D = fm["D"]
    for rows in (1, 7, 9):
        o = P.prep_gauss(rows, D, seed=rows)
        got = prep_call(D, o, rows, f"{fm['name']} rows {rows}")
        r = P.prep_ref(*o)
        bd = P.prep_bound(*o, r)
        for name in ("dx", "dm", "dvar", "dd"):
            w.hold(got[name], r[name], bd[name], f"rows {rows} {name}")
    # var just below 1e-6f (0x358637BC), exactly 1e-6f (0x358637BD), just above (0x358637BE) with m = 0, and
    # 536 / 537 x 2^-29 with m = 1/8: dvar is exactly 0 where var < 1e-6f and nonzero from 1e-6f on
    *o, active = P.prep_clamp_rows(D)
    got = prep_call(D, o, 5, fm["name"] + " clamp rows")
    r = P.prep_ref(*o)
    assert bool(((r["dvar"] == 0).all(-1) == active).all())
    assert bool(((got["dvar"] == 0).all(-1) == active).all()) and bool(((got["dvar"] != 0).all(-1) == ~active).all()), \
        fm["name"] + ": the var >= 1e-6f branch"
    bd = P.prep_bound(*o, r)
    for name in ("dx", "dm", "dvar", "dd"):
        w.hold(got[name], r[name], bd[name], f"clamp rows {name}")
    if D != 64:  # rows == 0: OK, nothing written
        b = [Buf(F32, (2 * D,)) for _ in range(6)]
        assert rc_of("mhada_attn_train_bwd_prep_hd", *[t.ptr for t in b], 0, D) == OK
        torch.cuda.synchronize()
        assert all(t.untouched(slice(None)) and t.guards_intact() for t in b)


RUN = dict(ln=run_ln, ln_train=run_ln_train, ln_bwd=run_ln_bwd, attn=run_attn, pos=run_pos, fold=run_fold, cosprep=run_cosprep,
           prep=run_prep)
RUN["in"] = run_in


@pytest.mark.parametrize("fm", FORMS)
def test_form(fm):
    w = Worst(fm)
    try:
        RUN[fm["fam"]](fm, w)
    finally:  # a failing row is logged with the ratio that failed it
            print(f"BOUND {fm['name']:30s} {fm['kernel']:64s} worst error/bound = {w.w:.4f}")


def test_zz_knobs_are_back_at_their_defaults():
    """Last in the module: every tuning() context above restored its knobs."""
    for k, v in DEFAULT_KNOBS.items():
        assert _lib.get_tuning(k) == v, k
