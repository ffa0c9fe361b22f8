"""Every mhada_gemm_tn / mhada_colsum kernel form, element by element (csrc/train_ops.hip).

FORMS is a table of cases, each naming the kernel instantiation it must reach and the dispatch condition of
mhada_gemm_tn that sends it there (DESIGN.md "TN GEMM forms under test" holds the same table;
profiles/r16_tn_forms_kernels.txt is the kernel trace of this file).  plan() is a Python transcription of the
entry's dispatch (tn_splits, kchunk, vec_a, rsrc, fuse_cs, the skinny conditions); tests/test_tn_forms_cpu.py
checks it against the table and the library without a GPU.  The C entry is called directly with a GemmTnArgs
of the test's own, so that ldc, the workspace size and the alignment of A are the test's to choose.  Every
case runs in the cross product of {ldc = N, ldc = N + 4} x {colsum, none} x {workspace of S * per floats
(G * per for the LDS-tiled kernel), workspace of exactly per floats}, per = nb (M N (+ M if fused)), and is
checked five ways:

  exact   operands are integers in [-4, 4] and 16 K < 2^24: every partial sum in any order is an exact fp32
          integer, so C and the column sums must be the fp64 reference bit for bit in every variant (the
          one-slab and many-slab runs therefore agree too).  The reference is asserted to be its own fp32
          rounding.
  canary  A, B, C, the column sums and the workspace each sit between guards that hold the quiet-NaN pattern
          0x7FC12345, as do the padding columns of lda > M, ldb > N and ldc = N + 4 and whatever follows the
          last legal element of A and B.  All guards must be intact afterwards, A and B unchanged, and the
          padded run must return the dense run's bits.
  probe   A = 0 except a single 1.0 at (k, m): row m of C must be im2col row k of the reference bit for bit
          and every other row +0.0, for k at the four corner pixels, one pixel on each edge, an interior
          pixel of the last image, kchunk - 1, kchunk and K - 1.
  bound   Gaussian operands: |C - ref| <= 2 gamma_{K+S} (|A|^T |B|) for every element, gamma_n = n u / (1 - n u),
          u = 2^-24, S the slab count of the run (factor 1: any order of round-to-nearest additions of the K
          products and the S slabs, zero terms exact; factor 2: the project's headroom for truncating adders
          inside the MFMA, as tests/test_gpu_gemm_forms.py); column sums within 2 gamma_K sum_k |A[k][m]|.
          Largest measured error / bound per case: profiles/r16_tn_forms_bounds.log, quoted below.
  repeat  a second call on the Gaussian operands returns the same bits.

Column sums: 'fused' (the MFMA kernel's epilogue), 'unfused' (mhada_colsum after the GEMM: M = 4, dense
aligned A) or refused: the entry writes C, then returns an error and leaves the column sums alone (every
VEC_A = false form and every M = 3 form; pinned here as the entry's behaviour, C is still checked).

A K stage shorter than 32 rows can only end the last split: kchunk is a multiple of 32 (asserted in plan()).
tn_skinny_kernel<PATCH8> is instantiated by the launch macro but refused before it ("PATCH8 needs M > 4"),
and "too many splits" cannot be reached (S <= 1024): neither has a case.

Largest measured error / bound: 0.27 for C and 0.20 for the fused column sums, both on
gemm_tn_kernel<ROWS,true,BM,false> at K = 3 (three terms: the bound is a few ulp); beyond K = 3 the largest are
0.10 for C (tn_skinny_lds_kernel<CONV3X3>, K = 15) and 0.023 for the column sums (K = 20).  The file takes 4 s.
"""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from mhada_hip import _lib

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ROWS, PATCH8, CONV3X3, ZERO = _lib.A_ROWS, _lib.A_PATCH8, _lib.A_CONV3X3, _lib.A_CONV3X3_ZERO
MODE_NAME = {ROWS: "ROWS", PATCH8: "PATCH8", CONV3X3: "CONV3X3", ZERO: "CONV3X3_ZERO"}
DEV = "cuda" if torch.cuda.is_available() else "cpu"

DEFAULT_KNOBS = dict(tn_skinny_lds=1)
NAN32 = 0x7FC12345  # guard bit pattern (a quiet NaN)
GUARD = 64          # guard floats before and after every buffer
UR = 2.0 ** -24
BIG_LDB = 16773120  # 32 * ldb * 4 = 0x7FF80000 >= 0x7FF00000: no per-stage buffer resources
CS_DENSE = "colsum needs a dense, aligned A"
CS_C4 = "mhada_colsum: C % 4 == 0"
CS_BATCH = "batched column sums need"


def gamma(n):
    return n * UR / (1 - n * UR)


# --------------------------------------------------------------------------------------------------
# the form table
# --------------------------------------------------------------------------------------------------
def form(name, kernel, cond, *, mode=ROWS, M, N=0, K=0, lda=None, ldb=None, a_off=0, nb=1, img=None, pad=0, lds=1, S,
         last=None, cs):
    """img = (B, H, W, Cin) of the NHWC layer input (conv modes) or (B, C, H, W) of the NCHW image (PATCH8);
    a_off = floats by which the A pointer is moved off its 16-byte boundary; lds = the tn_skinny_lds knob;
    S = slabs at the full workspace (splits, or the LDS-tiled kernel's blocks G), last = rows of the last
    K stage of the last split (MFMA kernel), cs = the column sums' route ('fused', 'unfused' or the error)."""
    grid = None
    if mode == PATCH8:
        B, C, H, W = img
        grid = (H // 8, W // 8)
        N, K = 64 * C, B * grid[0] * grid[1]
    elif mode in (CONV3X3, ZERO):
        B, H, W, C = img
        pad = pad if mode == ZERO else 1
        grid = (H + 2 * (pad - 1), W + 2 * (pad - 1))
        N, K = 9 * C, B * grid[0] * grid[1]
    lda = lda or M
    sza, szb = 0, 0
    if nb > 1:  # the per-head layout: B rows hold the nb heads side by side, A is one dense block per head
        ldb, szb, sza = nb * N, N, K * lda
    ldb = ldb or (N if mode == ROWS else 0)
    return pytest.param(dict(name=name, kernel=kernel, cond=cond, mode=mode, M=M, N=N, K=K, lda=lda, ldb=ldb, a_off=a_off,
                             nb=nb, sza=sza, szb=szb, img=img, grid=grid, pad=pad, lds=lds, S=S, last=last, cs=cs), id=name)


def gk(mode, vec, bm, rs=False):
    t = lambda b: "true" if b else "false"  # noqa: E731
    return f"gemm_tn_kernel<{MODE_NAME[mode]},{t(vec)},{bm},{t(rs)}>"


IMG_A, IMG_B = (2, 5, 7, 32), (3, 9, 13, 16)  # rows narrower than the 32-pixel K stage; N = 288 / 144


def _forms():
    f = []
    # ---- ROWS through per-stage buffer resources (RS) ---------------------------------------------
    rs = "ROWS, 16-B A rows, 32 max(lda, ldb) 4 < 0x7ff00000"
    for M, bm in ((64, 64), (132, 128)):
        f.append(form(f"rs{bm}_k257", gk(ROWS, True, bm, True), rs + "; two splits, the second ends in a 1-row stage",
                      M=M, N=132, K=257, S=2, last=1, cs="fused"))
        f.append(form(f"rs{bm}_k31", gk(ROWS, True, bm, True), rs + "; a single stage shorter than 32", M=M, N=132, K=31,
                      S=1, last=31, cs="fused"))
    f.append(form("rs64_lda68", gk(ROWS, True, 64, True), rs + "; lda = M + 4", M=64, N=132, K=257, lda=68, S=2, last=1,
                  cs="fused"))
    f.append(form("rs128_ldb140", gk(ROWS, True, 128, True), rs + "; ldb = N + 8", M=132, N=132, K=257, ldb=140, S=2,
                  last=1, cs="fused"))
    f.append(form("rs64_s10", gk(ROWS, True, 64, True), rs + "; S = 10: the 8-deep loop of slab_reduce_kernel, then its tail",
                  M=64, N=64, K=2305, S=10, last=1, cs="fused"))
    f.append(form("rs64_s3", gk(ROWS, True, 64, True), rs + "; S = 3: the tail loop of slab_reduce_kernel alone", M=64, N=64,
                  K=700, S=3, last=28, cs="fused"))
    f.append(form("rs64_batched", gk(ROWS, True, 64, True), rs + "; nb = 3 (blockIdx.z), ldb = nb N, szb = N, sza = K M",
                  M=64, N=64, K=1537, nb=3, S=2, last=1, cs="fused"))
    # ---- ROWS, 16-B A rows, without buffer resources -------------------------------------------------
    for M, bm in ((64, 64), (132, 128)):
        f.append(form(f"rows_v{bm}_bigldb", gk(ROWS, True, bm), "ROWS, 16-B A rows, 32 ldb 4 >= 0x7ff00000: p.rsrc off", M=M,
                      N=132, K=3, ldb=BIG_LDB, S=1, last=3, cs="fused"))
    # ---- ROWS, element loads of A ----------------------------------------------------------------------
    f.append(form("rows_s64_m30", gk(ROWS, False, 64), "M % 4 != 0", M=30, N=132, K=257, S=2, last=1, cs=CS_DENSE))
    f.append(form("rows_s128_m130", gk(ROWS, False, 128), "M % 4 != 0", M=130, N=132, K=257, S=2, last=1, cs=CS_DENSE))
    f.append(form("rows_s64_unaligned", gk(ROWS, False, 64), "M % 4 == 0, the A pointer one float off 16 bytes", M=64, N=132,
                  K=257, a_off=1, S=2, last=1, cs=CS_DENSE))
    # ---- conv modes on the MFMA kernel ----------------------------------------------------------------
    SL = {(IMG_A, 1): (1, 6), (IMG_A, 2): (1, 30), (IMG_B, 1): (2, 31), (IMG_B, 2): (2, 15)}  # (S, last) of image, pad
    for mode, pad, imgs in ((CONV3X3, 1, (IMG_A, IMG_B, IMG_B, IMG_A)), (ZERO, 1, (IMG_B, IMG_A, IMG_A, IMG_B)),
                            (ZERO, 2, (IMG_A, IMG_B, IMG_B, IMG_A))):
        tag = "reflect" if mode == CONV3X3 else f"zero{pad}"
        for (M, bm, vec), img in zip(((64, 64, True), (132, 128, True), (30, 64, False), (130, 128, False)), imgs):
            S, last = SL[img, pad]
            f.append(form(f"conv_{tag}_m{M}", gk(mode, vec, bm),
                          f"{MODE_NAME[mode]} pad {pad}, M = {M}" + ("" if vec else " (M % 4 != 0)") +
                          ": cxx wraps image rows and an image boundary within one issue()", mode=mode, M=M, img=img, pad=pad,
                          S=S, last=last, cs="fused" if vec else CS_DENSE))
    f.append(form("conv_reflect_h2", gk(CONV3X3, True, 64), "reflect at H = 2, the smallest legal height", mode=CONV3X3, M=64,
                  img=(2, 2, 7, 16), S=1, last=28, cs="fused"))
    f.append(form("conv_reflect_w2", gk(CONV3X3, True, 128), "reflect at W = 2, the smallest legal width", mode=CONV3X3, M=132,
                  img=(2, 5, 2, 16), S=1, last=20, cs="fused"))
    # ---- the patch-embedding weight gradient ----------------------------------------------------------
    for M, bm, vec in ((64, 64, True), (132, 128, True), (30, 64, False), (130, 128, False)):
        f.append(form(f"patch8_m{M}", gk(PATCH8, vec, bm), "PATCH8, N = 192: a partial column tile, min(n, N - 4) clamp",
                      mode=PATCH8, M=M, img=(2, 3, 24, 40), S=1, last=30, cs="fused" if vec else CS_DENSE))
    # ---- M <= 4: the gather form -------------------------------------------------------------------------
    sk = "tn_skinny_kernel<%s>"
    f.append(form("sk_rows_m3_n36", sk % "ROWS", "M <= 4; tpc = 9 does not divide 256; two splits, the second ragged", M=3,
                  N=36, K=4551, S=2, cs=CS_DENSE))
    f.append(form("sk_rows_m4_n36", sk % "ROWS", "M = 4, as above; mhada_colsum after the GEMM", M=4, N=36, K=4551, S=2,
                  cs="unfused"))
    f.append(form("sk_rows_m4_n1028", sk % "ROWS", "M <= 4; a second blockIdx.y with one quad", M=4, N=1028, K=300, S=1,
                  cs="unfused"))
    IMG_S = (3, 37, 41)  # K = 4551 (pad 1), 5031 (pad 2): two splits, the second ragged
    for mode, pad in ((CONV3X3, 1), (ZERO, 1), (ZERO, 2)):
        tag = "reflect" if mode == CONV3X3 else f"zero{pad}"
        f.append(form(f"sk_{tag}_m3_c32", sk % MODE_NAME[mode], "M <= 4, Cin % 64 != 0", mode=mode, M=3, img=IMG_S + (32,),
                      pad=pad, S=2, cs=CS_DENSE))
        f.append(form(f"sk_{tag}_m4_c64_gather", sk % MODE_NAME[mode], "M <= 4, Cin % 64 == 0, tn_skinny_lds = 0", mode=mode,
                      M=4, img=IMG_S + (64,), pad=pad, lds=0, S=2, cs="unfused"))
    # ---- M <= 4, Cin % 64 == 0, lda == 4: the LDS-tiled form ---------------------------------------------
    for mode, pad in ((CONV3X3, 1), (ZERO, 1), (ZERO, 2)):
        tag = "reflect" if mode == CONV3X3 else f"zero{pad}"
        k = "tn_skinny_lds_kernel<%s>" % MODE_NAME[mode]
        c = "M <= 4, conv, Cin % 64 == 0, lda == 4, aligned A; "
        f.append(form(f"lds_{tag}_m3_c64", k, c + "8 tiles ragged both ways, the last one pixel wide", mode=mode, M=3, lda=4,
                      img=(2, 6, 33, 64), pad=pad, S=8, cs=CS_C4))
        f.append(form(f"lds_{tag}_m4_c128", k, c + "two channel blocks", mode=mode, M=4, lda=4, img=(2, 6, 33, 128), pad=pad,
                      S=8, cs="unfused"))
        f.append(form(f"lds_{tag}_m4_c64_small", k, c + "an image smaller than one tile", mode=mode, M=4, lda=4,
                      img=(1, 3, 5, 64), pad=pad, S=pad, cs="unfused"))
        f.append(form(f"lds_{tag}_m3_c128_small", k, c + "smaller than one tile, two channel blocks", mode=mode, M=3, lda=4,
                      img=(1, 3, 5, 128), pad=pad, S=pad, cs=CS_C4))
    return f


FORMS = _forms()
BY_NAME = {p.values[0]["name"]: p.values[0] for p in FORMS}

# every instantiation mhada_gemm_tn can launch (csrc/train_ops.hip, TN_LAUNCH and the LDS-tiled branch)
INSTANTIATIONS = sorted(
    [gk(ROWS, True, bm, True) for bm in (64, 128)] +
    [gk(mode, vec, bm) for mode in (ROWS, PATCH8, CONV3X3, ZERO) for vec in (True, False) for bm in (64, 128)] +
    ["tn_skinny_kernel<%s>" % MODE_NAME[m] for m in (ROWS, CONV3X3, ZERO)] +
    ["tn_skinny_lds_kernel<%s>" % MODE_NAME[m] for m in (CONV3X3, ZERO)])

# mhada_colsum through its own entry: (rows, C, workspace floats or None = what ops.colsum sizes, chunks)
COLSUM_CASES = [(37, 12, None, 1), (200, 2048, None, 3), (8200, 64, None, 127), (8200, 64, 64, 1)]


# --------------------------------------------------------------------------------------------------
# the dispatch of mhada_gemm_tn, transcribed
# --------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def tn_bm(M):
    return 64 if M <= 64 else 128


def tn_splits(M, N, K):
    if M <= 4:
        return max(1, min(1024, K // 2048))
    tiles = cdiv(M, tn_bm(M)) * cdiv(N, 128)
    return max(1, min(cdiv(1024, tiles), cdiv(K, 256)))


def plan(fm, colsum, one_slab, splits=tn_splits):
    """What mhada_gemm_tn does with case fm: the kernel, the slab count S (G for the LDS-tiled kernel), kchunk,
    the workspace the test hands over and the column sums' route."""
    M, N, K, nb, mode, lda, ldb = (fm[k] for k in ("M", "N", "K", "nb", "mode", "lda", "ldb"))
    a_al = fm["a_off"] % 4 == 0
    vec_a = a_al and lda % 4 == 0 and M % 4 == 0
    rsrc = vec_a and mode == ROWS and 32 * max(lda, ldb) * 4 < 0x7ff00000
    fuse = bool(colsum) and vec_a and M > 4
    S0 = max(1, splits(M, N, K) // nb)
    per = (M * N + (M if fuse else 0)) * nb
    lds = M <= 4 and mode in (CONV3X3, ZERO) and fm["img"][3] % 64 == 0 and lda == 4 and a_al and bool(fm["lds"])
    nt = 0
    if lds:
        nt = (K // (fm["grid"][0] * fm["grid"][1])) * cdiv(fm["grid"][1], 32) * cdiv(fm["grid"][0], 4)
    wf = per if one_slab else max(S0, nt) * per
    S = min(S0, wf // per)
    kchunk = cdiv(cdiv(K, S), 32) * 32
    S = cdiv(K, kchunk)
    assert kchunk % 32 == 0 and (S - 1) * kchunk < K  # only the last split can end in a short stage
    bm = tn_bm(M)
    if lds:
        kernel, slabs = "tn_skinny_lds_kernel<%s>" % MODE_NAME[mode], min(nt, 1024, wf // per)
    elif M <= 4:
        kernel, slabs = "tn_skinny_kernel<%s>" % MODE_NAME[mode], S
    else:
        kernel, slabs = gk(mode, vec_a, bm, rsrc), S
    if not colsum:
        cs = None
    elif lds:
        cs = CS_C4 if M % 4 else "unfused"
    elif fuse:
        cs = "fused"
    elif nb > 1:
        cs = CS_BATCH
    elif lda != M or M % 4 or not a_al:
        cs = CS_DENSE
    else:
        cs = "unfused"
    rows_last = K - (S - 1) * kchunk
    return dict(kernel=kernel, S=slabs, kchunk=kchunk, per=per, wf=wf, cs=cs, vec_a=vec_a, rsrc=rsrc, fuse=fuse, bm=bm,
                last=rows_last % 32 or 32)


# --------------------------------------------------------------------------------------------------
# host side: operands and fp64 references (built once per case, never changed)
# --------------------------------------------------------------------------------------------------
def b_shape(fm):
    if fm["mode"] == ROWS:
        return (fm["nb"], fm["K"], fm["N"])
    return tuple(fm["img"])


def im2col(fm, b):
    """The [nb][K][N] matrix the kernels contract A with, from the logical B operand (fp64)."""
    mode, K, N = fm["mode"], fm["K"], fm["N"]
    if mode == ROWS:
        return b
    if mode == PATCH8:  # [token][c*64 + ky*8 + kx]
        return F.unfold(b, 8, stride=8).permute(0, 2, 1).reshape(1, K, N)
    Bn, H, W, C = b.shape
    xn = b.permute(0, 3, 1, 2)
    xp = F.pad(xn, (1, 1, 1, 1), mode="reflect") if mode == CONV3X3 else F.pad(xn, (fm["pad"],) * 4)
    cols = F.unfold(xp, 3)  # [B][ci*9 + tap][pixel] on the output grid
    L = cols.shape[-1]
    assert L == fm["grid"][0] * fm["grid"][1]
    return cols.view(Bn, C, 9, L).permute(0, 3, 2, 1).reshape(1, K, N)  # -> [pixel][tap*Cin + ci]


class Problem:
    """fp64 copies of the fp32 operands of one case, the fp64 reference and the absolute-value sums."""

    def __init__(self, fm, exact):
        g = torch.Generator(device="cpu").manual_seed(zlib.crc32(fm["name"].encode()) + int(exact))
        nb, K, M = fm["nb"], fm["K"], fm["M"]
        if exact:
            a = torch.randint(-4, 5, (nb, K, M), generator=g).double()
            b = torch.randint(-4, 5, b_shape(fm), generator=g).double()
        else:
            a = torch.randn(nb, K, M, generator=g).double()
            b = torch.randn(b_shape(fm), generator=g).double()
        self.a, self.b = a, b
        self.cols = im2col(fm, b)
        at = a.transpose(1, 2)
        self.ref = at @ self.cols                    # [nb][M][N]
        self.mag = at.abs() @ self.cols.abs()
        self.cs, self.csmag = a.sum(1), a.abs().sum(1)  # [nb][M]

    def exact_premises(self, fm):
        assert 16 * fm["K"] < 2 ** 24
        assert self.a.abs().max() <= 4 and self.b.abs().max() <= 4
        assert torch.equal(self.a, self.a.round()) and torch.equal(self.b, self.b.round())
        assert torch.equal(self.ref.float().double(), self.ref) and torch.equal(self.cs.float().double(), self.cs)
        assert self.mag.max().item() < 2 ** 24


@functools.lru_cache(maxsize=None)
def _problem(name, exact):
    return Problem(BY_NAME[name], exact)


def problem(fm, exact):
    return _problem(fm["name"], exact)


def bound_c(fm, pb, slabs):
    return 2 * gamma(fm["K"] + slabs) * pb.mag


def bound_cs(fm, pb):
    return 2 * gamma(fm["K"]) * pb.csmag


def probe_ks(fm, kchunk):
    """The k of the gather probes: corners, edges, an interior pixel of the last image, the split boundary."""
    K, ks = fm["K"], []
    if fm["grid"]:
        gh, gw = fm["grid"]
        last = K // (gh * gw) - 1
        px = [(0, 0, 0), (0, 0, gw - 1), (0, gh - 1, 0), (0, gh - 1, gw - 1),                      # corners
              (0, 0, gw // 2), (0, gh - 1, gw // 2), (0, gh // 2, 0), (0, gh // 2, gw - 1),        # edges
              (last, gh // 2, gw // 2)]                                                            # interior
        ks = [(b * gh + y) * gw + x for b, y, x in px]
    else:
        ks = [0]
    ks += [kchunk - 1, kchunk, K - 1]
    return [k for i, k in enumerate(ks) if 0 <= k < K and k not in ks[:i]]


# --------------------------------------------------------------------------------------------------
# device side: guarded buffers and one call per run
# --------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


class Buf:
    """A strided fp32 view inside a flat allocation: GUARD floats (+ off) | the view's span | GUARD floats.
    Everything that is not an element of the view holds the NaN pattern: the guards, the padding columns
    of a leading dimension, and what follows the last legal element.  big: an uninitialised allocation
    whose guards alone are set (the one large B)."""

    def __init__(self, size, stride, off=0, big=False):
        self.size, self.stride = tuple(size), tuple(stride)
        self.span = 1 + sum((n - 1) * s for n, s in zip(size, stride))
        self.lo = GUARD + off
        n = self.lo + self.span + GUARD
        if big:
            flat = torch.empty(n, dtype=torch.int32, device=DEV)
            flat[:self.lo] = NAN32
            flat[self.lo + self.span:] = NAN32
        else:
            flat = torch.full((n,), NAN32, dtype=torch.int32, device=DEV)
        self.flat = flat.view(F32)
        self.v = self.flat.as_strided(self.size, self.stride, self.lo)
        self.valid = None
        if not big:
            self.valid = torch.zeros(n, dtype=torch.bool, device=DEV)
            self.valid.as_strided(self.size, self.stride, self.lo).fill_(True)

    def ptr(self):
        return self.flat.data_ptr() + 4 * self.lo

    def fill(self, src):
        self.v.copy_(src.to(F32))
        return self

    def snapshot(self):
        self.saved = bits(self.flat).clone()
        return self

    def unchanged(self):
        return torch.equal(bits(self.flat), self.saved)

    def intact(self):
        return bool((bits(self.flat)[~self.valid] == NAN32).all())

    def untouched(self):
        return bool((bits(self.flat) == NAN32).all())


def a_buf(fm):
    return Buf((fm["nb"], fm["K"], fm["M"]), (fm["sza"], fm["lda"], 1), off=fm["a_off"])


def b_buf(fm):
    if fm["mode"] == ROWS:
        return Buf((fm["nb"], fm["K"], fm["N"]), (fm["szb"], fm["ldb"], 1), big=fm["ldb"] == BIG_LDB)
    shape = tuple(fm["img"])
    stride = [1] * 4
    for i in (2, 1, 0):
        stride[i] = stride[i + 1] * shape[i + 1]
    return Buf(shape, stride)


def operands(fm, pb):
    return a_buf(fm).fill(pb.a).snapshot(), b_buf(fm).fill(pb.b).snapshot()


def tn_args(fm, a, b, c, ldc, cs):
    args = _lib.GemmTnArgs()
    args.M, args.N, args.K = fm["M"], fm["N"], fm["K"]
    args.a, args.lda, args.b, args.ldb, args.b_mode = a, fm["lda"], b, fm["ldb"], fm["mode"]
    if fm["mode"] == PATCH8:
        args.img_c, args.img_h, args.img_w = fm["img"][1:]
    elif fm["mode"] != ROWS:
        args.img_h, args.img_w, args.img_c = fm["img"][1:]
    args.pad = fm["pad"]
    args.c, args.ldc, args.colsum = c, ldc, cs
    args.nb, args.sza, args.szb = fm["nb"], fm["sza"], fm["szb"]
    return args


def call_tn(args, work, wf):
    lib = _lib.load()
    rc = lib.mhada_gemm_tn(ctypes.byref(args), work, wf, torch.cuda.current_stream().cuda_stream)
    msg = (lib.mhada_last_error() or b"").decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg


def run(fm, dA, dB, colsum, one_slab, padded, wf=None):
    """One mhada_gemm_tn call between guards.  Returns (C [nb*M][N], column sums [nb*M] or None, plan)."""
    pl = plan(fm, colsum, one_slab, _lib.load().mhada_gemm_tn_splits)
    M, N, nb = fm["M"], fm["N"], fm["nb"]
    ldc = N + 4 if padded else N
    wf = wf or pl["wf"]
    c = Buf((nb * M, N), (ldc, 1))
    cs = Buf((nb * M,), (1,)) if colsum else None
    work = Buf((wf,), (1,))
    what = f"{fm['name']} colsum={colsum} one_slab={one_slab} ldc={ldc}"
    with _lib.tuning(tn_skinny_lds=fm["lds"]):
        rc, msg = call_tn(tn_args(fm, dA.ptr(), dB.ptr(), c.ptr(), ldc, cs.ptr() if colsum else None), work.ptr(), wf)
    assert c.intact(), what + ": C written outside [M][N]"
    assert work.intact(), what + ": workspace written outside its work_floats"
    assert dA.unchanged() and dB.unchanged(), what + ": an operand was written"
    if colsum and pl["cs"] not in ("fused", "unfused"):  # refused after C: an error, the column sums left alone
        assert rc == 1 and pl["cs"] in msg, (what, rc, msg)
        assert cs.untouched(), what + ": column sums written by a refused call"
        return c.v.clone(), None, pl
    assert rc == 0, (what, rc, msg)
    assert cs is None or cs.intact(), what + ": column sums written outside [nb][M]"
    return c.v.clone(), cs.v.clone() if colsum else None, pl


VARIANTS = [(colsum, one_slab, padded) for colsum in (False, True) for one_slab in (False, True) for padded in (False, True)]


def variants(fm):
    # (the batched form is refused with ldc != N: test_gemm_tn_rejections)
    return [v for v in VARIANTS if not (v[2] and fm["nb"] > 1)]


# --------------------------------------------------------------------------------------------------
# the tests
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fm", FORMS)
def test_form_exact_and_canaries(fm):
    """Integer operands: C and the column sums are the fp64 reference's bits in every variant, guards intact."""
    pb = problem(fm, True)
    pb.exact_premises(fm)
    dA, dB = operands(fm, pb)
    ref = bits(pb.ref.reshape(-1, fm["N"]).float().to(DEV))
    ref_cs = bits(pb.cs.reshape(-1).float().to(DEV))
    for colsum, one_slab, padded in variants(fm):
        c, cs, pl = run(fm, dA, dB, colsum, one_slab, padded)
        what = f"{fm['name']} colsum={colsum} one_slab={one_slab} padded={padded}"
        assert pl["kernel"] == fm["kernel"], what
        if not one_slab:
            assert pl["S"] == fm["S"], (what, pl["S"])
        assert torch.equal(bits(c), ref), what + ": C is not the fp64 reference's bits"
        assert (cs is not None) == (colsum and fm["cs"] in ("fused", "unfused")), what
        if cs is not None:
            assert torch.equal(bits(cs), ref_cs), what + ": the column sums are not the fp64 reference's bits"


@pytest.mark.parametrize("fm", FORMS)
def test_form_gather_probe(fm):
    """A single 1.0 in A picks one im2col row: row m of C is row k of the reference, every other row +0.0."""
    pb = problem(fm, True)
    dB = b_buf(fm).fill(pb.b).snapshot()
    dA = a_buf(fm)
    M, N, nb = fm["M"], fm["N"], fm["nb"]
    pl = plan(fm, False, False, _lib.load().mhada_gemm_tn_splits)
    kchunk = pl["kchunk"] if "lds" not in pl["kernel"] else 4 * fm["grid"][1]  # (LDS-tiled: the second row of tiles)
    ms = (0, M - 1, M // 2, min(M - 1, 64), min(M - 1, 31), min(M - 1, 32))
    cols = pb.cols.float().to(DEV)
    ks = probe_ks(fm, kchunk)
    for i, k in enumerate(ks):
        z, m = i % nb, ms[i % len(ms)]
        dA.v.zero_()
        dA.v[z, k, m] = 1.0
        dA.snapshot()
        c, _, _ = run(fm, dA, dB, False, False, bool(i & 1) and nb == 1)
        want = torch.zeros(nb, M, N, device=DEV)
        want[z, m] = cols[z, k]
        assert torch.equal(bits(c), bits(want.view(-1, N))), f"{fm['name']}: probe k={k} m={m} z={z}"


@pytest.mark.parametrize("fm", FORMS)
def test_form_componentwise_bound_and_repeat(fm):
    """Gaussian operands: the componentwise bound of the module docstring; a second call returns the same bits."""
    pb = problem(fm, False)
    dA, dB = operands(fm, pb)
    worst, worst_cs = 0.0, 0.0
    for colsum, one_slab, padded in variants(fm):
        c, cs, pl = run(fm, dA, dB, colsum, one_slab, padded)
        c2, cs2, _ = run(fm, dA, dB, colsum, one_slab, padded)
        what = f"{fm['name']} colsum={colsum} one_slab={one_slab} padded={padded}"
        assert torch.equal(bits(c), bits(c2)), what + ": C differs between two calls"
        err = (c.double().cpu().view(pb.ref.shape) - pb.ref).abs()
        assert bool(torch.isfinite(err).all()), what
        ratio = (err / bound_c(fm, pb, pl["S"]).clamp_min(1e-300)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, what + f": error / bound = {ratio:.3f}"
        if cs is not None:
            assert torch.equal(bits(cs), bits(cs2)), what + ": the column sums differ between two calls"
            err = (cs.double().cpu().view(pb.cs.shape) - pb.cs).abs()
            assert bool(torch.isfinite(err).all()), what
            ratio = (err / bound_cs(fm, pb).clamp_min(1e-300)).max().item()
            worst_cs = max(worst_cs, ratio)
            assert ratio <= 1.0, what + f": column sums error / bound = {ratio:.3f}"
    print(f"BOUND {fm['name']:28s} {fm['kernel']:46s} worst error/bound: C {worst:.4f} colsum {worst_cs:.4f}")


def test_batched_equals_single_calls():
    """nb = 3: every batch is bit for bit its own single call (integer operands), C and the fused column sums."""
    fm = BY_NAME["rs64_batched"]
    pb = problem(fm, True)
    dA, dB = operands(fm, pb)
    c, cs, _ = run(fm, dA, dB, True, False, False)
    M, N = fm["M"], fm["N"]
    one = dict(fm, nb=1, sza=0, szb=0)
    for z in range(fm["nb"]):
        pl = plan(one, True, False, _lib.load().mhada_gemm_tn_splits)
        cz, csz, work = Buf((M, N), (N, 1)), Buf((M,), (1,)), Buf((pl["wf"],), (1,))
        args = tn_args(one, dA.ptr() + 4 * z * fm["sza"], dB.ptr() + 4 * z * fm["szb"], cz.ptr(), N, csz.ptr())
        rc, msg = call_tn(args, work.ptr(), pl["wf"])
        assert rc == 0, msg
        assert cz.intact() and csz.intact() and work.intact()
        assert torch.equal(bits(cz.v), bits(c[z * M:(z + 1) * M])), z
        assert torch.equal(bits(csz.v), bits(cs[z * M:(z + 1) * M])), z


@pytest.mark.parametrize("name", [p.values[0]["name"] for p in FORMS if p.values[0]["name"].startswith("lds_")])
def test_lds_form_equals_gather_form(name):
    """The LDS-tiled kernel and the gather kernel on the same integer operands, at G = tiles and G = 1."""
    fm = BY_NAME[name]
    pb = problem(fm, True)
    dA, dB = operands(fm, pb)
    gather = dict(fm, lds=0)
    g, _, pg = run(gather, dA, dB, False, False, False)
    assert pg["kernel"] == "tn_skinny_kernel<%s>" % MODE_NAME[fm["mode"]]
    for one_slab in (False, True):
        c, _, pl = run(fm, dA, dB, False, one_slab, False)
        assert pl["kernel"] == fm["kernel"] and pl["S"] == (1 if one_slab else fm["S"])
        assert torch.equal(bits(c), bits(g)), (name, one_slab)


def test_slab_reduce_split_counts():
    """The table holds a ROWS case whose S takes the 8-deep loop of slab_reduce_kernel (S >= 9) and one that
    takes its tail loop alone (2 <= S <= 8), per the library's own mhada_gemm_tn_splits."""
    lib = _lib.load()
    got = {}
    for name in ("rs64_s10", "rs64_s3"):
        fm = BY_NAME[name]
        got[name] = plan(fm, False, False, lib.mhada_gemm_tn_splits)["S"]
        assert lib.mhada_gemm_tn_splits(fm["M"], fm["N"], fm["K"]) == tn_splits(fm["M"], fm["N"], fm["K"])
    assert got["rs64_s10"] == 10 and got["rs64_s3"] == 3


@pytest.mark.parametrize("rows,C,wf,chunks", COLSUM_CASES)
def test_colsum_entry(rows, C, wf, chunks):
    """mhada_colsum through its own entry: integer operands, exact, out and work between guards."""
    g = torch.Generator(device="cpu").manual_seed(rows * 4099 + C)
    x = torch.randint(-4, 5, (rows, C), generator=g).double()
    ref = x.sum(0)
    assert 4 * rows < 2 ** 24 and torch.equal(ref.float().double(), ref)
    wf = wf or min(128, max(1, rows // 64)) * C
    ch = min(max(1, rows // 64), 128, wf // C)
    ch = cdiv(rows, cdiv(rows, ch))
    assert ch == chunks
    dx = Buf((rows, C), (C, 1)).fill(x).snapshot()
    out, work = Buf((C,), (1,)), Buf((wf,), (1,))
    lib = _lib.load()
    rc = lib.mhada_colsum(dx.ptr(), out.ptr(), rows, C, work.ptr(), wf, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.mhada_last_error()
    assert out.intact() and work.intact() and dx.unchanged()
    assert torch.equal(bits(out.v), bits(ref.float().to(DEV)))
    assert bool((bits(work.v[ch * C:]) == NAN32).all()), "workspace written beyond chunks * C"


# --------------------------------------------------------------------------------------------------
# rejections
# --------------------------------------------------------------------------------------------------
def test_gemm_tn_rejections():
    """Every fail() of mhada_gemm_tn once: status 1, its text, and C, the column sums and the workspace
    untouched (the two refusals that follow the GEMM: C's guards and the column sums)."""
    M = N = K = 64
    a = torch.ones(2 * K * M + 8, device=DEV)
    b = torch.ones(4 * 64 * 64 * 9 + 8, device=DEV)  # room for every operand shape below
    c, cs = Buf((2 * M * (N + 4),), (1,)), Buf((2 * M,), (1,))  # (flat: any ldc of the calls below stays inside)
    per = 2 * (M * N + M)
    work = Buf((per,), (1,))

    def rejected(match, late=False, **over):
        f = dict(M=M, N=N, K=K, a=a.data_ptr(), lda=M, b=b.data_ptr(), ldb=N, b_mode=ROWS, img_c=0, img_h=0, img_w=0,
                 pad=0, c=c.ptr(), ldc=N, colsum=cs.ptr(), nb=1, sza=0, szb=0, work=work.ptr(), wf=per)
        f.update(over)
        args = _lib.GemmTnArgs()
        for k, v in f.items():
            if k not in ("work", "wf"):
                setattr(args, k, v)
        rc, msg = call_tn(args, f["work"], f["wf"])
        assert rc == 1 and match in msg, (match, rc, msg)
        assert cs.untouched(), match
        if late:
            assert c.intact(), match
            c.flat.view(torch.int32).fill_(NAN32)
            work.flat.view(torch.int32).fill_(NAN32)
        else:
            assert c.untouched() and work.untouched(), match

    conv = dict(b_mode=CONV3X3, img_c=8, img_h=8, img_w=8, N=72, ldc=72, K=64, colsum=None)
    patch = dict(b_mode=PATCH8, img_c=1, img_h=16, img_w=32, N=64, K=8, colsum=None)
    for k in ("a", "b", "c", "work"):
        rejected("mhada_gemm_tn: null argument", **{k: None})
    for k in ("M", "N", "K"):
        rejected("mhada_gemm_tn: bad sizes", **{k: 0})
    rejected("bad sizes", K=-1)
    rejected("N must be a multiple of 4", N=62)
    rejected("B and the workspace must be 16-byte aligned", b=b.data_ptr() + 4)
    rejected("B and the workspace must be 16-byte aligned", work=work.ptr() + 8)
    rejected("ldc < N", ldc=N - 4)
    rejected("batched form needs ROWS mode", nb=2, **dict(conv, colsum=cs.ptr()))
    rejected("batched form needs ROWS mode", nb=2, M=4, lda=4)
    rejected("batched form needs ROWS mode", nb=2, ldc=N + 4)
    rejected("batched form needs ROWS mode", nb=2, sza=K * M + 2)
    rejected("batched form needs ROWS mode", nb=2, szb=N + 1)
    rejected("batch too large", nb=65536)
    rejected("ldb must be a multiple of 4", ldb=N + 2)
    rejected("PATCH8 needs H, W % 8 == 0, N == 64*C", **dict(patch, img_w=36))
    rejected("PATCH8 needs H, W % 8 == 0, N == 64*C", **dict(patch, img_h=12))
    rejected("PATCH8 needs H, W % 8 == 0, N == 64*C", **dict(patch, N=128, ldc=128))
    rejected("PATCH8 needs K == batch*(H/8)*(W/8)", **dict(patch, K=12))
    rejected("PATCH8 needs M > 4", **dict(patch, M=4, lda=4))
    rejected("pad 1 or 2", **dict(conv, b_mode=ZERO, pad=3))
    rejected("pad 1 or 2", **dict(conv, b_mode=ZERO, pad=-1))
    rejected("CONV needs N == 9*Cin, Cin % 4 == 0", **dict(conv, img_c=6))
    rejected("CONV needs N == 9*Cin, Cin % 4 == 0", **dict(conv, N=64))
    rejected("reflect needs H, W >= 2", **dict(conv, img_h=1, img_w=64))
    rejected("reflect needs H, W >= 2", **dict(conv, img_h=64, img_w=1))
    rejected("CONV needs K == batch*out_h*out_w", **dict(conv, K=60))
    rejected("CONV needs K == batch*out_h*out_w", **dict(conv, b_mode=ZERO, pad=2, K=64))
    rejected("bad b_mode", b_mode=3)
    rejected("bad b_mode", b_mode=7)
    rejected("workspace smaller than nb*(M*N (+M)) floats", wf=M * N + M - 1)
    rejected("workspace smaller than nb*(M*N (+M)) floats", wf=M * N)  # room for C's slab, not for the column sums
    rejected("workspace smaller than nb*(M*N (+M)) floats", nb=2, sza=K * M, wf=per - 1)
    rejected(CS_BATCH, late=True, nb=2, sza=K * M, a=a.data_ptr() + 4)
    rejected(CS_DENSE, late=True, a=a.data_ptr() + 4)
    rejected(CS_DENSE, late=True, M=62, lda=62)
    rejected(CS_DENSE, late=True, M=4, lda=8)
    rejected(CS_C4, late=True, **dict(conv, img_c=64, N=576, ldc=576, M=3, lda=4, colsum=cs.ptr()))


def test_colsum_rejections():
    rows, C = 64, 8
    x = torch.ones(rows * C + 8, device=DEV)
    out, work = Buf((C,), (1,)), Buf((2 * C,), (1,))
    lib = _lib.load()

    def rejected(match, **over):
        f = dict(x=x.data_ptr(), out=out.ptr(), rows=rows, C=C, work=work.ptr(), wf=2 * C)
        f.update(over)
        rc = lib.mhada_colsum(*f.values(), torch.cuda.current_stream().cuda_stream)
        msg = (lib.mhada_last_error() or b"").decode()
        torch.cuda.synchronize()
        assert rc == 1 and match in msg, (match, rc, msg)
        assert out.untouched() and work.untouched(), match

    for k in ("x", "out", "work"):
        rejected("mhada_colsum: bad args", **{k: None})
    rejected("mhada_colsum: bad args", rows=0)
    rejected("mhada_colsum: bad args", C=0)
    rejected(CS_C4, C=6)
    rejected(CS_C4, x=x.data_ptr() + 4)
    rejected(CS_C4, work=work.ptr() + 8)
    rejected("workspace smaller than C floats", wf=C - 1)


def test_zz_knobs_are_back_at_their_defaults():
    """Last in the module: every tuning() context above restored its knobs."""
    for k, v in DEFAULT_KNOBS.items():
        assert _lib.get_tuning(k) == v, k
