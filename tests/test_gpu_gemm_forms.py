"""Every mhada_gemm kernel form, element by element (csrc/gemm_impl.h, gemm.hip, conv_tile.hip).

FORMS is a table of cases, each naming the kernel it is meant to reach and the dispatch condition that
sends it there (DESIGN.md "GEMM forms under test" holds the same table; profiles/r09_gemm_forms_kernels.txt
is the kernel trace of this file).  Every case runs every epilogue its form accepts, dense and with
every leading dimension and z-stride padded by the smallest legal step, and is checked three ways:

  exact   operands are integers in [-4, 4] (K <= 4096: every partial sum is an integer below 2^24, so any
          summation order gives the same fp32 bits); C, c2, a bf16 C and vt must equal the fp64
          reference's roundings bit for bit.  The reference is asserted to be its own fp32 rounding.
  canary  every output sits between guard rows and beside padding columns that hold a NaN bit pattern;
          they must hold it afterwards, and the padded run must return the dense run's bits.
  bound   Gaussian operands; every fp32 element within 2 g (|A| |W|^T + |bias| + |R|), g = gamma_{K+2} in
          fp32 (factor 1: any order of round-to-nearest additions; factor 2: headroom for truncating
          adders inside the MFMA), bf16 outputs + 2^-8 |ref|.  Largest measured error / bound
          (profiles/r09_gemm_forms_bounds.log): 0.073 for an fp32 output (f32_persist_rows), 0.99 for a
          bf16 output (the 2^-8 |ref| term is the bf16 rounding itself).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    from mhada_hip._lib import A_CONV3X3, A_CONV3X3_UP2, A_CONV3X3_ZERO, A_PATCH8, A_ROWS, A_SPLIT3
    DEV = "cuda"
    CUS = torch.cuda.get_device_properties(0).multi_processor_count
else:  # collection without a GPU: the table is still built (every test here is marked gpu)
    A_ROWS, A_PATCH8, A_CONV3X3, A_CONV3X3_UP2, A_CONV3X3_ZERO, A_SPLIT3 = range(6)
    DEV, CUS = "cpu", 256

DEFAULT_KNOBS = dict(gemm_pp=1, gemm_persist=1, gemm_pp128=1, gemm_ldsepi=1, gemm_n64=128, gemm_rinit=1,
                     conv_c64=1, conv_dir=1, gemm_s3_order=1)
NAN32, NAN16 = 0x7FC12345, 0x7FC1  # guard bit patterns (quiet NaNs)
GUARD = 3                          # guard rows before, after and (padded runs) between problems
U = 2.0 ** -24


# --------------------------------------------------------------------------------------------------
# the form table
# --------------------------------------------------------------------------------------------------
def form(name, kernel, cond, *, cdt, M=0, N=0, K=0, mode=A_ROWS, adt=None, odt=None, nb=(1, 1), img=None, pad=0,
         mu=False, vt=False, knobs=None, direct=False):
    """img = (B, H, W, Cin) of the NHWC input (conv modes) or (C, H, W) of the NCHW image (PATCH8)."""
    adt = adt or cdt
    odt = odt or cdt
    if mode == A_PATCH8:
        C, H, W = img
        M, K = (H // 8) * (W // 8), 64 * C
    elif mode in (A_CONV3X3, A_CONV3X3_UP2, A_CONV3X3_ZERO):
        B, H, W, C = img
        oh, ow = ((2 * H, 2 * W) if mode == A_CONV3X3_UP2 else
                  (H + 2 * (pad - 1), W + 2 * (pad - 1)) if mode == A_CONV3X3_ZERO else (H, W))
        M, K = B * oh * ow, 9 * C
    return pytest.param(dict(name=name, kernel=kernel, cond=cond, cdt=cdt, adt=adt, odt=odt, M=M, N=N, K=K, mode=mode,
                             nb=nb, img=img, pad=pad, mu=mu, vt=vt, knobs=knobs or {}, direct=direct), id=name)


def _forms():
    f = []
    # ---- fp32 compute ------------------------------------------------------------------------------
    t128 = "gemm_kernel<f32,128,128>"
    for K in (32, 64, 96):  # one, two and an odd count of 32-wide K-tiles
        f.append(form(f"f32_t128_rows_k{K}", t128, "fp32, N > 64, below the persistent threshold", cdt=F32,
                      M=300, N=204, K=K, nb=(2, 3) if K == 96 else (1, 1)))
    f.append(form("f32_t128_centred", t128, "a_mu: kRowsCentred", cdt=F32, M=150, N=132, K=64, nb=(2, 2), mu=True))
    f.append(form("f32_t128_patch8", t128, "PATCH8 never takes the persistent kernel", cdt=F32, N=132, mode=A_PATCH8,
                  img=(3, 40, 24), nb=(2, 1)))
    f.append(form("f32_t128_conv", t128, "CONV3X3 below the persistent threshold", cdt=F32, N=132, mode=A_CONV3X3,
                  img=(2, 9, 15, 32)))
    f.append(form("f32_t128_up2", t128, "CONV3X3_UP2 never takes the persistent kernel", cdt=F32, N=68,
                  mode=A_CONV3X3_UP2, img=(2, 6, 5, 32)))
    for pad in (1, 2):
        f.append(form(f"f32_t128_zero{pad}", t128, "CONV3X3_ZERO below the persistent threshold", cdt=F32, N=132,
                      mode=A_CONV3X3_ZERO, img=(2, 7, 9, 32), pad=pad))
    f.append(form("f32_t128x64_k48", "gemm_kernel<f32,128,64>", "N <= 64, K % 32 != 0", cdt=F32, M=300, N=60, K=48,
                  nb=(1, 2)))
    f.append(form("f32_t128x64_centred", "gemm_kernel<f32,128,64>", "N <= 64 with a_mu", cdt=F32, M=300, N=64, K=64,
                  nb=(2, 2), mu=True))
    f.append(form("f32_t256x64_k48", "gemm_kernel<f32,256,64>", "N <= 64, K % 32 != 0, gemm_n64 = 256", cdt=F32,
                  M=300, N=60, K=48, nb=(1, 2), knobs=dict(gemm_n64=256)))
    f.append(form("f32_t256x64_centred", "gemm_kernel<f32,256,64>", "N <= 64 with a_mu, gemm_n64 = 256", cdt=F32,
                  M=300, N=64, K=64, nb=(2, 2), mu=True, knobs=dict(gemm_n64=256)))
    f.append(form("f32_n64_ring128", "gemm_n64_kernel<128,2,32>", "fp32 ROWS, N <= 64, K % 32 == 0, K < 1024", cdt=F32,
                  M=300, N=60, K=96, nb=(1, 3)))
    f.append(form("f32_n64_ring128_z8", "gemm_n64_kernel<128,2,32>", "as above, nz % 8 == 0 (per-XCD grouping)",
                  cdt=F32, M=150, N=64, K=32, nb=(2, 4)))
    f.append(form("f32_n64_ring256", "gemm_n64_kernel<256,2,64>", "fp32 ROWS, N <= 64, K >= 1024, K % 64 == 0",
                  cdt=F32, M=300, N=60, K=1024, nb=(1, 2)))
    f.append(form("f32_n64_ring256_k1088", "gemm_n64_kernel<256,2,64>", "as above, an odd count of K-tiles", cdt=F32,
                  M=257, N=64, K=1088))
    # persistent fp32: 8 * ceil(M/256) * ceil(N/256) * nz >= 7 * CUs
    ppf = "gemm_ppp_kernel<f32,256>"
    tm2 = -(-7 * CUS // 16)  # row tiles at N = 512 (two column tiles)
    f.append(form("f32_persist_rows", ppf, "fp32 ROWS, N > 128, 8 t256 >= 7 CUs", cdt=F32, M=tm2 * 256 - 100, N=512,
                  K=64))
    f.append(form("f32_below_persist", t128, "one row tile below 8 t256 >= 7 CUs", cdt=F32, M=(tm2 - 1) * 256 - 100,
                  N=512, K=64))
    f.append(form("f32_persist_rows_many", ppf, "more tiles than workgroups, partial column tile, 3 K-tiles", cdt=F32,
                  M=(CUS // 3 + 2) * 256 - 100, N=516, K=96))
    tmz = -(-7 * CUS // 64)
    f.append(form("f32_persist_rows_z", ppf, "nb1 * nb2 = 4 counted in t256", cdt=F32, M=tmz * 256 - 60, N=260, K=64,
                  nb=(2, 2)))
    hc = -(-tm2 * 256 // (2 * 60))
    f.append(form("f32_persist_conv", ppf, "fp32 CONV3X3, 8 t256 >= 7 CUs", cdt=F32, N=260, mode=A_CONV3X3,
                  img=(2, hc, 60, 32)))
    f.append(form("f32_persist_zero", ppf, "fp32 CONV3X3_ZERO, 8 t256 >= 7 CUs", cdt=F32, N=260, mode=A_CONV3X3_ZERO,
                  img=(2, hc, 60, 32), pad=1))
    f.append(form("f32_vt", t128 + " + store_vt_tile", "vt (N = 128, ROWS)", cdt=F32, M=200, N=128, K=64, nb=(2, 2),
                  mu=True, vt=True))
    # ---- bf16 compute ------------------------------------------------------------------------------
    ppb, pp1 = "gemm_ppp_kernel<bf16,256>", "gemm_pp_kernel"
    for odt in (BF16, F32):
        o = "o16" if odt == BF16 else "o32"
        f.append(form(f"bf16_persist_rows_{o}", ppb, "bf16 A, N > 128, K % 64 == 0, K >= 128", cdt=BF16, odt=odt,
                      M=600, N=260, K=128))
        f.append(form(f"bf16_persist_rows_z_{o}", ppb, "as above, z-batched, 3 K-tiles", cdt=BF16, odt=odt, M=300,
                      N=260, K=192, nb=(2, 2)))
        f.append(form(f"bf16_persist_conv_{o}", ppb, "bf16 CONV3X3, N > 128", cdt=BF16, odt=odt, N=260,
                      mode=A_CONV3X3, img=(2, 13, 11, 64)))
        f.append(form(f"bf16_oneshot_k64_{o}", pp1, "bf16 A, N > 128, K = 64 (one K-tile)", cdt=BF16, odt=odt, M=600,
                      N=260, K=64, nb=(1, 2)))
        f.append(form(f"bf16_oneshot_nopersist_{o}", pp1, "K >= 128 with gemm_persist = 0", cdt=BF16, odt=odt, M=600,
                      N=260, K=192, knobs=dict(gemm_persist=0)))
        f.append(form(f"bf16_pp128_rows_{o}", "gemm_ppp_kernel<bf16,128>", "N in 65..128, K >= 128", cdt=BF16,
                      odt=odt, M=600, N=100, K=192, nb=(2, 1)))
    f.append(form("bf16_persist_rows_many", ppb, "more tiles than workgroups", cdt=BF16, odt=F32,
                  M=(CUS // 4 + 2) * 256 - 100, N=772, K=128))
    # bf16 C with N % 8 == 0 and ldc % 8 == 0 (the padded run steps ldc by 8): the 16-byte stores of
    # store_tile_lds_bf16 run, on a partial column tile (8 columns), next to the canaries
    f.append(form("bf16_persist_rows_o16_w16", ppb, "as bf16_persist_rows_o16, 16-byte bf16 stores", cdt=BF16, M=600,
                  N=264, K=128, nb=(1, 2)))
    f.append(form("bf16_persist_conv_o16_w16", ppb, "bf16 CONV3X3, 16-byte bf16 stores", cdt=BF16, N=264,
                  mode=A_CONV3X3, img=(2, 13, 11, 64)))
    f.append(form("bf16_persist_rows_o16_many", ppb, "more tiles than workgroups, bf16 C, 16-byte stores", cdt=BF16,
                  M=(CUS // 3 + 2) * 256 - 100, N=520, K=128))
    f.append(form("bf16_oneshot_k64_o16_w16", pp1, "K = 64, 16-byte-aligned bf16 rows", cdt=BF16, M=600, N=264, K=64))
    f.append(form("bf16_pp128_rows_o16_w16", "gemm_ppp_kernel<bf16,128>", "N in 65..128, 16-byte-aligned bf16 rows",
                  cdt=BF16, M=600, N=104, K=128))
    for odt in (BF16, F32):
        f.append(form(f"bf16_pp128_rows_{'o16' if odt == BF16 else 'o32'}_many", "gemm_ppp_kernel<bf16,128>",
                      "more tiles than workgroups", cdt=BF16, odt=odt, M=(CUS + 3) * 256 - 100, N=104, K=192))
    f.append(form("bf16_persist_directepi", ppb, "gemm_ldsepi = 0: direct stores", cdt=BF16, odt=BF16, M=600, N=260,
                  K=128, knobs=dict(gemm_ldsepi=0)))
    f.append(form("bf16_persist_norinit", ppb, "gemm_rinit = 0: residual added in the epilogue", cdt=BF16, odt=F32,
                  M=600, N=260, K=128, knobs=dict(gemm_rinit=0)))
    f.append(form("f32_persist_norinit", ppf, "gemm_rinit = 0 on the fp32 persistent kernel", cdt=F32,
                  M=tm2 * 256 - 100, N=512, K=64, knobs=dict(gemm_rinit=0)))
    f.append(form("f32_persist_directepi", ppf, "gemm_ldsepi = 0 on the fp32 persistent kernel", cdt=F32,
                  M=tm2 * 256 - 100, N=512, K=64, knobs=dict(gemm_ldsepi=0)))
    f.append(form("f32_nopersist", t128, "gemm_persist = 0 above the threshold", cdt=F32, M=tm2 * 256 - 100, N=512,
                  K=64, knobs=dict(gemm_persist=0)))
    f.append(form("bf16_pp128_conv", "gemm_ppp_kernel<bf16,128>", "bf16 CONV3X3, N in 65..128", cdt=BF16, N=96,
                  mode=A_CONV3X3, img=(2, 13, 11, 64)))
    t256x128, t256 = "gemm_kernel<bf16,256,128>", "gemm_kernel<bf16,256,256>"
    f.append(form("bf16_t256x128_k64", t256x128, "N in 65..128, K = 64", cdt=BF16, M=600, N=100, K=64, nb=(2, 2)))
    f.append(form("bf16_t256x128_nopp128", t256x128, "K >= 128 with gemm_pp128 = 0", cdt=BF16, odt=F32, M=600, N=100,
                  K=192, knobs=dict(gemm_pp128=0)))
    f.append(form("bf16_t256x128_a32", t256x128, "fp32 A", cdt=BF16, adt=F32, odt=F32, M=600, N=100, K=128))
    f.append(form("bf16_t256x128_k64_w16", t256x128, "N in 65..128, K = 64, 16-byte bf16 stores", cdt=BF16, M=600,
                  N=104, K=64, nb=(2, 1)))
    f.append(form("bf16_t256_k72_o16_w16", "gemm_kernel<bf16,256,256>", "N > 128, K % 64 != 0, 16-byte bf16 stores",
                  cdt=BF16, M=600, N=264, K=72))
    # M = 200: the padded ldt (320) lies beyond the one 256-row tile, so the tail zeroing runs (z-batched);
    # M = 300: two row tiles that cover the padded ldt (384)
    f.append(form("bf16_vt", t256x128 + " + store_vt_tile", "vt (N = 128, ROWS)", cdt=BF16, adt=F32, M=200, N=128,
                  K=64, nb=(2, 2), mu=True, vt=True))
    f.append(form("bf16_vt_a16", t256x128 + " + store_vt_tile", "vt with bf16 A, no centring", cdt=BF16, M=300, N=128,
                  K=128, nb=(1, 2), vt=True))
    for adt in (BF16, F32):
        for odt in (BF16, F32):
            tag = f"a{16 if adt == BF16 else 32}_o{16 if odt == BF16 else 32}"
            f.append(form(f"bf16_t256_k72_{tag}", t256, "N > 128, K % 64 != 0", cdt=BF16, adt=adt, odt=odt, M=600,
                          N=260, K=72, nb=(1, 2) if adt == BF16 else (1, 1)))
    f.append(form("bf16_t256_a32", t256, "N > 128, fp32 A", cdt=BF16, adt=F32, odt=BF16, M=600, N=260, K=128))
    f.append(form("bf16_t256_nopp", t256, "gemm_pp = 0", cdt=BF16, M=600, N=260, K=192, nb=(2, 1),
                  knobs=dict(gemm_pp=0)))
    f.append(form("bf16_t256x128_nopp", t256x128, "gemm_pp = 0, N in 65..128", cdt=BF16, M=600, N=100, K=128,
                  knobs=dict(gemm_pp=0)))
    f.append(form("bf16_t256_zero2", t256, "CONV3X3_ZERO gather", cdt=BF16, odt=F32, N=260, mode=A_CONV3X3_ZERO,
                  img=(2, 9, 11, 64), pad=2))
    f.append(form("bf16_t256_patch8", t256, "PATCH8 gather (fp32 image)", cdt=BF16, adt=F32, odt=F32, N=260,
                  mode=A_PATCH8, img=(3, 40, 72), nb=(2, 1)))
    for adt in (BF16, F32):
        f.append(form(f"bf16_t128_up2_a{16 if adt == BF16 else 32}", "gemm_kernel<bf16,128,128,UP2>", "CONV3X3_UP2",
                      cdt=BF16, adt=adt, N=132, mode=A_CONV3X3_UP2, img=(2, 6, 5, 64)))
    f.append(form("bf16_n64_128", "gemm_kernel<bf16,128,64>", "N <= 64", cdt=BF16, M=300, N=60, K=128, nb=(2, 2)))
    f.append(form("bf16_n64_128_a32_o16", "gemm_kernel<bf16,128,64>", "N <= 64, a32_o16", cdt=BF16, adt=F32, odt=BF16,
                  M=300, N=64, K=64, mu=True, nb=(2, 2)))
    f.append(form("bf16_n64_256", "gemm_kernel<bf16,256,64>", "N <= 64, gemm_n64 = 256", cdt=BF16, odt=F32, M=300, N=60,
                  K=192, nb=(2, 2), knobs=dict(gemm_n64=256)))
    # ---- direct conv kernels (dense runs; a padded ldc / ldw takes the GEMM form, as the knob does) ----
    for mode, tag in ((A_CONV3X3, ""), (A_CONV3X3_UP2, "_up2")):
        f.append(form(f"conv_c64{tag}", "conv3x3_c64", "bf16 64 -> 64, dense, bias, no residual", cdt=BF16, N=64,
                      mode=mode, img=(2, 9, 13, 64), direct=True))
        f.append(form(f"conv_c64{tag}_off", "gemm_kernel<bf16,128,64>", "conv_c64 = 0", cdt=BF16, N=64, mode=mode,
                      img=(2, 9, 13, 64), knobs=dict(conv_c64=0)))
    for ci, co in ((128, 64), (128, 128), (256, 128)):
        f.append(form(f"conv_dir_{ci}_{co}", "conv3x3_dir", "bf16 CONV3X3, dense, bias, no residual", cdt=BF16, N=co,
                      mode=A_CONV3X3, img=(2, 9, 13, ci), direct=True))
        f.append(form(f"conv_dir_{ci}_{co}_off", "gemm_kernel / gemm_ppp_kernel<bf16,128>", "conv_dir = 0", cdt=BF16,
                      N=co, mode=A_CONV3X3, img=(2, 9, 13, ci), knobs=dict(conv_dir=0)))
    # ---- SPLIT3 ------------------------------------------------------------------------------------
    for order in (1, 0):
        for K0 in (64, 192):
            f.append(form(f"split3_order{order}_k{K0}", "gemm_s3_kernel" if order else "gemm_ppp_kernel<bf16,SPLIT3>",
                          f"A_SPLIT3, gemm_s3_order = {order}", cdt=BF16, odt=F32, M=300, N=260, K=6 * K0,
                          mode=A_SPLIT3, knobs=dict(gemm_s3_order=order)))
        f.append(form(f"split3_order{order}_o16", "gemm_s3_kernel" if order else "gemm_ppp_kernel<bf16,SPLIT3>",
                      f"A_SPLIT3, bf16 C, gemm_s3_order = {order}", cdt=BF16, odt=BF16, M=300, N=260, K=6 * 128,
                      mode=A_SPLIT3, knobs=dict(gemm_s3_order=order)))
        for odt in (BF16, F32):  # two column tiles (the second 8 wide), more tiles than workgroups
            f.append(form(f"split3_order{order}_{'o16' if odt == BF16 else 'o32'}_many",
                          "gemm_s3_kernel" if order else "gemm_ppp_kernel<bf16,SPLIT3>",
                          f"A_SPLIT3, more tiles than workgroups, gemm_s3_order = {order}", cdt=BF16, odt=odt,
                          M=(CUS // 2 + 2) * 256 - 100, N=264, K=6 * 128, mode=A_SPLIT3, knobs=dict(gemm_s3_order=order)))
    return f


FORMS = _forms()


# --------------------------------------------------------------------------------------------------
# operands in dense / padded layouts
# --------------------------------------------------------------------------------------------------
def ceil_to(x, m):
    return -(-x // m) * m


def nan_fill(n, dtype):
    if dtype == F32:
        return torch.full((n,), NAN32, dtype=torch.int32, device=DEV).view(F32)
    return torch.full((n,), NAN16, dtype=torch.int16, device=DEV).view(BF16)


class Buf:
    """[nb1][nb2][rows][cols] with row stride ld inside one flat NaN-pattern buffer: GUARD rows before the
    first and after the last problem, and (gap) between problems."""

    def __init__(self, dtype, nb, rows, cols, ld, gap, src=None):
        self.dtype, self.nb, self.rows, self.cols, self.ld = dtype, nb, rows, cols, ld
        g = GUARD if gap else 0
        self.s2 = (rows + g) * ld
        self.s1 = nb[1] * self.s2 + g * ld
        self.off = GUARD * ld
        self.flat = nan_fill(2 * GUARD * ld + nb[0] * self.s1, dtype)
        if src is not None:
            self.view().copy_(src.reshape(nb[0], nb[1], rows, cols))

    @property
    def t(self):  # the tensor whose data_ptr is problem (0, 0), row 0
        return self.flat[self.off:]

    @property
    def s(self):
        return (self.s1, self.s2)

    def view(self):
        return self.flat.as_strided((*self.nb, self.rows, self.cols), (self.s1, self.s2, self.ld, 1), self.off)

    def get(self):
        return self.view().clone()

    def guards_intact(self):
        valid = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        valid.as_strided((*self.nb, self.rows, self.cols), (self.s1, self.s2, self.ld, 1), self.off).fill_(True)
        iv = self.flat.view(torch.int32 if self.dtype == F32 else torch.int16)
        return bool((iv[~valid] == (NAN32 if self.dtype == F32 else NAN16)).all())


def ints(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).double().to(DEV)


def gauss(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def a_matrix(fm, a64):
    """The GEMM's A operand [nb1][nb2][M][K] (fp64) gathered from the logical input a64 as a_mode says."""
    mode = fm["mode"]
    if mode in (A_ROWS, A_SPLIT3):
        return a64
    if mode == A_PATCH8:  # a64 [nb1][nb2][C][H][W]; k = c * 64 + ky * 8 + kx
        nb1, nb2 = fm["nb"]
        cols = F.unfold(a64.flatten(0, 1), 8, stride=8)  # [nz][C * 64][L]
        return cols.transpose(1, 2).reshape(nb1, nb2, fm["M"], fm["K"])
    x = a64.permute(0, 3, 1, 2)  # NHWC -> NCHW
    B, C = x.shape[:2]
    if mode == A_CONV3X3_UP2:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    if mode == A_CONV3X3_ZERO:
        x = F.pad(x, (fm["pad"],) * 4)
    else:
        x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    cols = F.unfold(x, 3)  # [B][C * 9][L], row c * 9 + tap; the GEMM's k = tap * C + c
    L = cols.shape[-1]
    return cols.view(B, C, 9, L).permute(0, 3, 2, 1).reshape(1, 1, B * L, 9 * C)


class Problem:
    """Logical operands of one case (fp64 copies of exactly the values the kernel computes with), the
    products shared by all epilogues, and the reference of each epilogue."""

    def __init__(self, fm, exact):
        self.fm, self.exact = fm, exact
        nb, M, N, K, mode = fm["nb"], fm["M"], fm["N"], fm["K"], fm["mode"]
        cdt, adt, odt = fm["cdt"], fm["adt"], fm["odt"]
        draw = (lambda *s, seed, scale=1.0: ints(*s, seed=seed)) if exact else gauss
        K0 = K // 6 if mode == A_SPLIT3 else K
        if mode in (A_ROWS, A_SPLIT3):
            ashape = (*nb, M, K0)
        elif mode == A_PATCH8:
            ashape = (*nb, *fm["img"])
        else:
            ashape = fm["img"]
        a = draw(*ashape, seed=1)
        if not exact and mode == A_CONV3X3_UP2:
            # multiples of 1/8: the x2 bilinear blend (weights in sixteenths) is then exact in fp32 in any
            # association, so the operand's bf16 rounding is defined by the header alone
            a = (a * 8).round() / 8
        if mode == A_SPLIT3:
            self.a_dev = a.float()  # split into planes on the device
        else:
            self.a_dev = a.to(adt)
        a = self.a_dev.double()
        self.mu_dev = None
        if fm["mu"]:
            self.mu_dev = draw(*nb, 1, K, seed=2).float()
            a = (self.a_dev.float() - self.mu_dev).double()  # a - a_mu formed in fp32 ...
        am = a_matrix(fm, a)
        if mode == A_CONV3X3_UP2 and cdt == BF16:
            assert torch.equal(am.float().double(), am)
            if exact:  # multiples of 1/16 below 4: the upsampled operand is its own bf16 rounding
                assert torch.equal(am.bfloat16().double(), am)
        if mode != A_SPLIT3:
            am = am.to(cdt).double()  # ... then rounded to the compute type (round to nearest)
        self.w_dev = draw(*nb, N, K0, seed=3, scale=K0 ** -0.5).to(F32 if mode == A_SPLIT3 else cdt)
        w = self.w_dev.double()
        self.bias_dev = draw(*nb, 1, N, seed=4).float()
        self.r_dev = draw(*nb, M, N, seed=5).to(odt)
        mask = draw(*nb, M, N, seed=6)
        if not exact:
            mask[..., ::7] = 0.0
        self.mask_dev = mask.float()
        assert bool((self.mask_dev == 0).any()) and bool((self.mask_dev < 0).any())
        self.base = am @ w.transpose(-1, -2)
        self.absb = am.abs() @ w.abs().transpose(-1, -2)
        self.g = (K0 + 2) * U / (1 - (K0 + 2) * U)

    def ref(self, ep):
        """(fp64 reference, componentwise bound) of epilogue ep."""
        y, mag = self.base, self.absb
        if ep["bias"]:
            y = y + self.bias_dev.double()
            mag = mag + self.bias_dev.double().abs()
        if ep["relu"] == 1:
            y = torch.relu(y)
        if ep["relu"] == 2:
            y = torch.where(self.mask_dev > 0, y, torch.zeros_like(y))
        elif ep["res"]:
            y = y + self.r_dev.double()
            mag = mag + self.r_dev.double().abs()
        return y, 2 * self.g * mag


def epilogues(fm):
    """Every epilogue the form accepts."""
    mode, odt = fm["mode"], fm["odt"]
    E = lambda **kw: dict(dict(bias=True, relu=0, res=False, c2=False, planes=False, c_null=False), **kw)  # noqa: E731
    if fm["vt"]:
        return [E(), E(bias=False)]
    eps = [E(), E(relu=1), E(res=True), E(relu=1, res=True), E(bias=False, res=True)]
    if odt == F32:
        eps.append(E(res=True, c2=True))
        eps.append(E(relu=1, c2=True))
        if mode in (A_ROWS, A_SPLIT3):
            eps.append(E(relu=2, res=True))
    if mode == A_SPLIT3 and odt == F32:
        eps += [E(res=True, c2=True, planes=True), E(relu=1, c2=True, planes=True, c_null=True),
                E(relu=2, res=True, c2=True, planes=True)]
    return eps


def run(fm, pb, ep, padded):
    """One mhada_gemm call; returns dict of outputs ([nb1][nb2][M][N] tensors) after the guard checks."""
    nb, M, N, K, mode = fm["nb"], fm["M"], fm["N"], fm["K"], fm["mode"]
    cdt, adt, odt = fm["cdt"], fm["adt"], fm["odt"]
    ea, ec = (4 if adt == F32 else 8), (4 if cdt == F32 else 8)
    p = lambda step: step if padded else 0  # noqa: E731
    kw = dict(M=M, N=N, K=K, compute=cdt, a_mode=mode, nb=nb, relu=ep["relu"], pad=fm["pad"])
    keep = []
    if mode == A_ROWS:
        A = Buf(adt, nb, M, K, K + p(ea), padded, pb.a_dev)
        kw.update(a=A.t, lda=A.ld, sa=A.s)
    elif mode == A_SPLIT3:
        K0 = K // 6
        planes = ops.split3_rows(pb.a_dev.reshape(M, K0).contiguous())
        A = Buf(BF16, (1, 1), 3 * M, K0, K0 + p(8), False, planes)  # lda > K0: contiguous planes of M * lda
        kw.update(a=A.t, lda=A.ld)
    elif mode == A_PATCH8:
        C, H, W = fm["img"]
        A = Buf(adt, nb, 1, C * H * W, C * H * W + p(4), padded, pb.a_dev)
        kw.update(a=A.t, sa=A.s, img=(C, H, W))
    else:
        B, H, W, C = fm["img"]
        A = Buf(adt, (1, 1), 1, pb.a_dev.numel(), pb.a_dev.numel(), False, pb.a_dev)
        kw.update(a=A.t, img=(C, H, W))
    keep.append(A)
    if mode == A_SPLIT3:
        w6 = ops.split3_weight(pb.w_dev.reshape(N, K // 6))
        Wb = Buf(BF16, nb, N, K, K + p(ec), padded, w6)
    else:
        Wb = Buf(cdt, nb, N, K, K + p(ec), padded, pb.w_dev)
    kw.update(w=Wb.t, ldw=Wb.ld, sw=Wb.s)
    if fm["mu"]:
        MU = Buf(F32, nb, 1, K, K + p(4), padded, pb.mu_dev)
        kw.update(a_mu=MU.t, smu=MU.s)
    if ep["bias"]:
        Bb = Buf(F32, nb, 1, N, ceil_to(N, 4) + p(4), padded, pb.bias_dev)
        kw.update(bias=Bb.t, sb=Bb.s)
    ldn = ceil_to(N, 4)
    cstep = 8 if odt == BF16 and N % 8 == 0 else 4  # keep 16-byte bf16 rows 16-byte aligned in the padded run
    if ep["res"]:
        src = pb.mask_dev if ep["relu"] == 2 else pb.r_dev
        Rb = Buf(odt, nb, M, N, ldn + p(cstep), padded, src)
        kw.update(r=Rb.t, ldr=Rb.ld, sr=Rb.s)
    outs = {}
    ccols = 64 if fm["vt"] else N  # with vt, columns 64..127 of C are not written
    Cb = Buf(odt, nb, M, ccols, ldn + p(cstep), padded)
    if ep["c_null"]:
        kw.update(c=None, ldc=Cb.ld)
    else:
        kw.update(c=Cb.t, ldc=Cb.ld, sc=Cb.s)
        outs["c"] = Cb
    if ep["c2"]:
        if ep["planes"]:
            C2 = Buf(BF16, (1, 1), 3 * M, N, ldn + p(4), False)
            kw.update(c2=C2.flat[C2.off:C2.off + 3 * M * C2.ld].view(3, M, C2.ld), ldc2=C2.ld, c2_planes=True)
        else:
            C2 = Buf(BF16, nb, M, N, ldn + p(4), padded)
            kw.update(c2=C2.t, ldc2=C2.ld, sc2=C2.s)
        outs["c2"] = C2
    if fm["vt"]:
        VT = Buf(odt, nb, 128, ceil_to(M, 64) + p(64), ceil_to(M, 64) + p(64), padded)
        kw.update(vt=VT.t, ldt=VT.ld, svt=VT.s)
        outs["vt"] = VT
    with _lib.tuning(**fm["knobs"]):
        ops.gemm(**kw)
    torch.cuda.synchronize()
    res = {}
    for k, b in outs.items():
        assert b.guards_intact(), f"{fm['name']} {ep} padded={padded}: {k} written outside [M][N]"
        res[k] = b.get()
    return res


def split3_bounds(out, ref, f32):
    def rel(a, b):
        return ((a.double() - b).norm() / (b.norm() + 1e-30)).item()
    e, e32 = rel(out, ref), rel(f32, ref)
    assert e < 2e-6 and e <= 2.5 * e32 + 1e-7, (e, e32)
    return e / 2e-6


def check(fm, exact):
    pb = Problem(fm, exact)
    odt, M, N = fm["odt"], fm["M"], fm["N"]
    worst = 0.0
    kv = None
    for ep in epilogues(fm):
        ref, bound = pb.ref(ep)
        if exact:
            # the CPU-side premise of the exact check: the reference is its own fp32 rounding
            assert torch.equal(ref.float().double().cpu(), ref.cpu()), "reference left the exact fp32 range"
        dense = run(fm, pb, ep, padded=False)
        padded = run(fm, pb, ep, padded=True)
        for k in dense:
            if k == "vt":  # the padded image is wider: its first ceil64(M) positions are the dense image
                assert torch.equal(dense[k], padded[k][..., :dense[k].shape[-1]]), f"{fm['name']} {ep}: padded vt"
            elif exact or not fm["direct"]:  # (a direct conv kernel's padded run is the GEMM form: other bits)
                assert torch.equal(dense[k], padded[k]), f"{fm['name']} {ep}: padded {k} differs from dense"
        for tag, got in (("dense", dense), ("padded", padded)):
            what = f"{fm['name']} {ep} {tag}"
            if "c" in got and fm["vt"]:
                ref_c = ref[..., :64]
                bound_c = bound[..., :64]
            else:
                ref_c, bound_c = ref, bound
            if "c" in got:
                c = got["c"]
                if exact:
                    assert torch.equal(c, ref_c.float().to(odt)), what + ": C"
                elif fm["mode"] == A_SPLIT3 and odt == F32:
                    if ep["relu"] != 2:
                        f32 = ops.linear(pb.a_dev.reshape(M, -1), pb.w_dev.reshape(N, -1),
                                         pb.bias_dev.reshape(N) if ep["bias"] else None, F32,
                                         residual=pb.r_dev.reshape(M, N) if ep["res"] else None, relu=bool(ep["relu"]))
                        worst = max(worst, split3_bounds(c.reshape(M, N), ref.reshape(M, N), f32))
                    else:  # the masked result: the norm bound alone (ops.linear has no SPLIT3-free twin here)
                        e = ((c.double() - ref).norm() / ref.norm()).item()
                        worst = max(worst, e / 2e-6)
                        assert e < 2e-6, what + f": relu = 2 error {e:.3e}"
                else:
                    b = bound_c + (2.0 ** -8 * ref_c.abs() if odt == BF16 else 0)
                    err = (c.double() - ref_c).abs()
                    ratio = (err / b.clamp_min(1e-300)).max().item()
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, what + f": error / bound = {ratio:.3f}"
            if "c2" in got:
                c2 = got["c2"]
                if ep["planes"]:
                    pl = c2.reshape(3, M, N)
                    if "c" in got:
                        full = got["c"].reshape(M, N)
                    else:
                        full = run(fm, pb, dict(ep, c2=False, planes=False, c_null=False), tag == "padded")["c"].reshape(M, N)
                    assert torch.equal(pl[0], full.bfloat16()), what + ": plane 0"
                    s = pl[0].double() + pl[1].double() + pl[2].double()
                    assert bool(((s - full.double()).abs() <= full.double().abs() * 2.0 ** -26).all()), what + ": planes"
                    if exact:
                        assert torch.equal(s, ref.reshape(M, N)), what + ": plane sum"
                else:
                    assert torch.equal(c2, got["c"].bfloat16()), what + ": c2 is not C's bf16 rounding"
                    if exact:
                        assert torch.equal(c2, ref.float().bfloat16()), what + ": c2"
            if "vt" in got:
                if kv is None or kv[0] is not ep:
                    # (the same tile kernel without vt: gemm_pp128 = 0 keeps N = 128 off the persistent form)
                    plain = dict(fm, vt=False, knobs=dict(fm["knobs"], gemm_pp128=0))
                    kv = (ep, run(plain, pb, ep, False)["c"])
                    # that run's K | V' rows against the reference, so vt is tied to fp64 and not only to itself
                    if exact:
                        assert torch.equal(kv[1], ref.float().to(odt)), what + ": K|V' rows of the plain run"
                    else:
                        b = bound + (2.0 ** -8 * ref.abs() if odt == BF16 else 0)
                        ratio = ((kv[1].double() - ref).abs() / b.clamp_min(1e-300)).max().item()
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, what + f": K|V' rows error / bound = {ratio:.3f}"
                tv = ops.transpose_v(kv[1].contiguous())
                ld0 = tv.shape[-1]
                assert torch.equal(got["vt"][..., :ld0], tv), what + ": vt"
                assert bool((got["vt"][..., ld0:] == 0).all()), what + ": vt positions M..ldt-1 not written 0"
    return worst


@pytest.mark.parametrize("fm", FORMS)
def test_form_exact_and_canaries(fm):
    """Integer operands: every output bit for bit, dense and padded, guards intact."""
    check(fm, exact=True)


@pytest.mark.parametrize("fm", FORMS)
def test_form_componentwise_bound(fm):
    """Gaussian operands: the componentwise fp32 bound (SPLIT3: its own tests' bounds), guards intact."""
    worst = check(fm, exact=False)
    print(f"BOUND {fm['name']:32s} {fm['kernel']:40s} worst error/bound = {worst:.4f}")


# --------------------------------------------------------------------------------------------------
# rejections
# --------------------------------------------------------------------------------------------------
def _rejected(match, odt=F32, **over):
    M, N, K = 64, 128, 64
    a = torch.ones(2 * M * K + 8, device=DEV)
    w = torch.ones(2 * N * K + 8, device=DEV)
    c = nan_fill(4 * M * N, odt)
    kw = dict(a=a, w=w, c=c, M=M, N=N, K=K, compute=F32, lda=K, ldw=K, ldc=N)
    kw.update(over)
    with pytest.raises(ValueError, match=match):
        ops.gemm(**kw)
    torch.cuda.synchronize()
    iv = c.view(torch.int32 if odt == F32 else torch.int16)
    assert bool((iv == (NAN32 if odt == F32 else NAN16)).all())


def test_rejections_leave_c_untouched():
    M, N = 64, 128
    mask = torch.ones(M * N, device=DEV)
    vt = nan_fill(128 * 64, F32)
    _rejected("multiples of 4", ldc=N + 2)
    _rejected("W must be 16-byte aligned", w=torch.ones(2 * N * 64 + 8, device=DEV)[1:])
    _rejected("relu = 2", relu=2, r=mask, ldr=N, vt=vt, ldt=64)
    _rejected("vt needs", N=124, vt=vt, ldt=64)
    _rejected("not z-batched", a_mode=A_CONV3X3, K=288, img=(32, 8, 8), nb=(2, 1), ldw=288)
    assert bool((vt.view(torch.int32) == NAN32).all())
    # SPLIT3: lda < K0; c2_planes without the LDS epilogue
    K0, Ns = 128, 256
    pl = torch.ones(3 * M * K0, device=DEV, dtype=BF16)
    w6 = torch.ones(Ns * 6 * K0, device=DEV, dtype=BF16)
    s3 = dict(a=pl, w=w6, N=Ns, K=6 * K0, compute=BF16, a_mode=A_SPLIT3, ldw=6 * K0, ldc=Ns)
    _rejected("SPLIT3 lda", lda=K0 - 8, **s3)
    c2 = nan_fill(3 * M * Ns, BF16).view(3, M, Ns)
    with _lib.tuning(gemm_ldsepi=0):
        _rejected("the LDS epilogue", lda=K0, c2=c2, ldc2=Ns, c2_planes=True, **s3)
    assert bool((c2.view(torch.int16) == NAN16).all())
    ops.gemm(c=nan_fill(M * Ns, F32), M=M, lda=K0, c2=c2, ldc2=Ns, c2_planes=True, **s3)  # accepted with the knob on
    torch.cuda.synchronize()
    assert not bool(torch.isnan(c2.float()).any())


def test_zz_knobs_are_back_at_their_defaults():
    """Last in the module: every tuning() context above restored its knobs."""
    for k, v in DEFAULT_KNOBS.items():
        assert _lib.get_tuning(k) == v, k
