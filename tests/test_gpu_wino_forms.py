"""Every Winograd conv kernel form, element by element (csrc/wino.hip).

FORMS is a table of forward cases, each naming the kernel it must reach and the dispatch condition that
sends it there; WG_FORMS is the same for the weight gradient (DESIGN.md "Winograd forms under test" holds
both tables; profiles/r15_wino_forms_kernels.txt is the kernel trace of this file).  Operands, fp64
references and the absolute-value sums are built on the host once per problem and shared by the kernel
routes (tests/test_wino_forms_cpu.py checks the premises below without a GPU).  fp64 F.conv2d is the only
oracle.  Every forward case runs four epilogues (bias + ReLU, neither, bias + relu_mask, relu_mask alone),
dense and with ldc = Cout + 4, and is checked three ways:

  exact   x integer in [-4, 4], filters in {-8, -4, 0, 4, 8} (U = G g G^T is an integer), integer bias:
          every transform term, product and partial sum in any order is an integer below 2^24, so the
          output must be the fp32 rounding of the fp64 reference bit for bit on every route.  Asserted on
          the host: the reference is its own fp32 rounding, and the absolute-value Winograd sum
          S = |A|^T [(|G| |g| |G|^T) . (|B|^T |d| |B|)] |A| summed over channels, + |bias|, is below 2^24.
  canary  x, U, the plane image, bias, mask and y each sit inside a larger allocation whose guard rows hold
          a quiet-NaN bit pattern, as do the ldc - Cout pad columns of y and mask.  y's guards must be
          intact; a read that strays into an input's guard turns the exact comparison into NaN; the padded
          run must return the dense run's bits; the mask holds +0.0 and -0.0 beside negative and positive
          entries: outputs there must be +0.0, elsewhere the unmasked run's bits.
  bound   Gaussian operands at the decoder's scale: every element within 2 gamma_n (S + |bias|) of fp64,
          gamma_n = n u / (1 - n u), u = 2^-24.  wino_kernel / wino4_kernel: n = Cin + 12 (two roundings in
          the input transform, four in the filter transform, the product, Cin accumulations, four in the
          output transform, one for the bias).  wino_s3_kernel: n = 6 Cin + 12 (six products per channel
          into the one accumulator) plus 2^-24 S for the three dropped cross products.  The factor 2 is the
          GEMM suite's headroom for truncating adders inside the MFMA.  Largest measured error / bound
          (profiles/r15_wino_forms_bounds.log): 0.048 (wino_kernel / wino4_kernel), 0.0055 (wino_s3_kernel).

SPLIT3 plane cases (wino_s3_kernel): operands on dyadic grids chosen so that named bf16 planes of V or U are
occupied, every kept cross product is a multiple of q, the absolute-value sum over the planes is below
2^24 q and the three dropped cross products are exactly zero: the output must again be the reference's
bits, which fails if a plane or one of the six kept cross products is lost.

Weight gradient (mhada_conv3x3_wgrad_wino called directly, the test sets work_floats and db): integer x and
g in [-2, 2] (A dY A^T, B^T d B and the tile sums are integers, G^T dU G a multiple of 1/4) must give dw and
db bit for bit for every split count; guards around dw, db and the workspace, workspace floats beyond
S * per untouched, NaN pad columns of g; Gaussian operands within 2 gamma_n S_w, S_w the absolute-value
contraction |G|^T [sum_tiles (|A| |dY| |A|^T) . (|B|^T |d| |B|)] |G|.  n = B H W + 9 for dw: one output's fp32
path takes two roundings in each of the two tile transforms, one product, one accumulation per tile
(B H W / 4) and one per split slab (S <= B H W / 128), four roundings in G^T . G: below the pixel count plus
9.  db sums the B H W gradient pixels in some tree: n = B H W, S_b = sum |g|.  Largest measured error /
bound: 0.0060 (dw), 0.0098 (db).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"
else:  # collection without a GPU: the tables and the host-side operands are still built
    DEV = "cpu"

DEFAULT_KNOBS = dict(wino4=1, wino_split3=1)
NAN32, NAN16 = 0x7FC12345, 0x7FC1  # guard bit patterns (quiet NaNs)
GUARD = 3                          # guard rows before and after every tensor
UR = 2.0 ** -24

G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=F64)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)
KEPT = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))  # the SPLIT3 cross products v_i u_j, in issue order


def gamma(n):
    return n * UR / (1 - n * UR)


# --------------------------------------------------------------------------------------------------
# the form tables
# --------------------------------------------------------------------------------------------------
ROUTES = {
    "wino": dict(kernel="wino_kernel", planes=False, knobs=dict(wino4=0), cond="U without the plane image, wino4 = 0"),
    "wino4": dict(kernel="wino4_kernel", planes=False, knobs={}, cond="U without the plane image, default knobs"),
    "wino4p": dict(kernel="wino4_kernel", planes=True, knobs=dict(wino_split3=0), cond="U with planes, wino_split3 = 0"),
    "s3": dict(kernel="wino_s3_kernel", planes=True, knobs={}, cond="U with planes, default knobs"),
}
# one partial tile; odd; exactly one block; a one-pixel remainder on both axes, several blocks; the base
GRIDS = [(1, 2, 2), (2, 3, 2), (2, 16, 16), (1, 17, 33), (2, 9, 13)]
PADS = [("reflect", 1), ("zero", 1), ("zero", 2)]
BASE = dict(grid=(2, 9, 13), pad=("reflect", 1), Ci=32, Co=64)
EPILOGUES = [dict(bias=True, relu=True, mask=False), dict(bias=False, relu=False, mask=False),
             dict(bias=True, relu=False, mask=True), dict(bias=False, relu=False, mask=True)]


def form(route, **over):
    fm = dict(BASE, route=route, **ROUTES[route])
    fm.update(over)
    B, H, W = fm["grid"]
    fm["name"] = f"{route}_{fm['pad'][0]}{fm['pad'][1]}_b{B}_{H}x{W}_{fm['Ci']}to{fm['Co']}"
    return pytest.param(fm, id=fm["name"])


def _forms():
    f = []
    for route, r in ROUTES.items():
        for grid in GRIDS:  # every grid with every padding (the base case among them)
            for pad in PADS:
                f.append(form(route, grid=grid, pad=pad))
        # Cin: one, three and four 8-channel chunks (fp32 kernels without planes); one SPLIT3 chunk, the
        # two-slot ring wrap (32, the base), an odd and an even chunk count; many chunks on one grid
        for Ci in ((16, 48, 64) if r["planes"] else (8, 24, 16, 48, 64)):
            f.append(form(route, Ci=Ci))
        f.append(form(route, Ci=256, pad=("zero", 1)))
        # Cout 128: the second output-channel block has its own U slice (with several spatial blocks too)
        f.append(form(route, Co=128))
        f.append(form(route, Co=128, Ci=16 if r["planes"] else 8, grid=(1, 17, 33), pad=("zero", 2)))
    return f


FORMS = _forms()

# SPLIT3 plane cases: operand grids (steps and ranges) found on the host so that the budget and the
# occupancy asserted in plane_problem() hold; "share" names the plane whose occupancy is asserted
PLANE_CASES = {
    "v2": dict(doc="two planes of V", x=("grid", 2.0 ** -9, 2.0, 0.0), w=("grid", 2.0 ** -2, 1.0, 0.5),
               share=("V", 1), top=dict(V=1, U=0)),
    "u2": dict(doc="two planes of U", x=("grid", 1.0, 1.0, 0.9), w=("grid", 2.0 ** -13, 1.0, 0.0),
               share=("U", 1), top=dict(V=0, U=1)),
    # (beyond the issue's list: the only case in which the v1 u1 product is not zero)
    "v2u2": dict(doc="two planes of each", x=("grid", 2.0 ** -7, 4.0, 0.0), w=("taps", 2.0 ** -8, 2.0, 2),
                 share=("V", 1), share_nz=("U", 1), top=dict(V=1, U=1)),
    "v3": dict(doc="three planes of V", x=("grid", 2.0 ** -19, 1.0, 0.0), w=("taps", 4.0, 4.0, 1),
               share=("V", 2), top=dict(V=2, U=0)),
    "u3": dict(doc="three planes of U", x=("onehot", 1.0, 1.0, 4), w=("grid", 2.0 ** -19, 0.5, 0.0),
               share=("U", 2), top=dict(V=0, U=2)),
}
PLANE_FORMS = [pytest.param(case, Ci, id=f"{case}_cin{Ci}") for case in PLANE_CASES for Ci in (16, 32, 48)]


def wg_form(name, kernel, cond, *, grid, zero, Ci=64, Co=64, S, one_slab=False):
    return pytest.param(dict(name=name, kernel=kernel, cond=cond, grid=grid, zero=zero, Ci=Ci, Co=Co, S=S,
                             one_slab=one_slab), id=name)


def _wg_forms():
    f = []
    for zero in (False, True):
        k = f"wino_wgrad_kernel<{'true' if zero else 'false'}> + wino_wgrad_finish_kernel"
        t = "zero" if zero else "reflect"
        f.append(wg_form(f"wg_{t}_1chunk", k, "one chunk, S = 1", grid=(1, 2, 16), zero=zero, S=1))
        f.append(wg_form(f"wg_{t}_32chunks", k, "32 chunks, S = 2", grid=(2, 16, 32), zero=zero, S=2))
        f.append(wg_form(f"wg_{t}_50chunks", k, "50 chunks, S = 3, the last split one chunk short", grid=(1, 20, 80),
                         zero=zero, S=3))
        f.append(wg_form(f"wg_{t}_50chunks_1slab", k, "50 chunks, work_floats of one slab: S = 1", grid=(1, 20, 80),
                         zero=zero, S=1, one_slab=True))
        f.append(wg_form(f"wg_{t}_cin128", k, "a second input-channel block", grid=(2, 16, 32), zero=zero, Ci=128, S=2))
        f.append(wg_form(f"wg_{t}_cout128", k, "a second output-channel block", grid=(2, 16, 32), zero=zero, Co=128,
                         S=2))
    return f


WG_FORMS = _wg_forms()


# --------------------------------------------------------------------------------------------------
# host side: operands, fp64 references, absolute-value sums (all on the CPU, cached per problem)
# --------------------------------------------------------------------------------------------------
def gen(*seed):
    return torch.Generator(device="cpu").manual_seed(sum(int(s) * 1000 ** i for i, s in enumerate(seed)) % (2 ** 31))


def pad_nchw(x, pad):
    """x NHWC fp64 -> the padded NCHW image the conv correlates."""
    xn = x.permute(0, 3, 1, 2)
    return F.pad(xn, (1, 1, 1, 1), mode="reflect") if pad[0] == "reflect" else F.pad(xn, (pad[1],) * 4)


def tiles(xp):
    """Padded NCHW image -> the 4 x 4 input patches d [B][C][ty][tx][4][4] of the 2 x 2 output tiles (zeros past
    the image: those positions reach only output rows / columns that are not stored)."""
    Hp, Wp = xp.shape[-2:]
    ty, tx = (Hp - 1) // 2, (Wp - 1) // 2
    xp = F.pad(xp, (0, 2 * tx + 2 - Wp, 0, 2 * ty + 2 - Hp))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)


def v_of(d, bt=BT):
    return torch.einsum("ij,bctxjk,lk->bctxil", bt, d, bt)


def u_of(w, g=G):
    return torch.einsum("ij,ocjk,lk->ocil", g, w, g)


def y_of(V, U, at, Ho, Wo):
    """A^T [sum_c U . V] A -> NHWC [B][Ho][Wo][Co]."""
    M = torch.einsum("bctxil,ocil->botxil", V, U)
    Y = torch.einsum("ij,botxjk,lk->botxil", at, M, at)
    B, Co, ty, tx = Y.shape[:4]
    return Y.permute(0, 2, 4, 3, 5, 1).reshape(B, 2 * ty, 2 * tx, Co)[:, :Ho, :Wo].contiguous()


def planes(t):
    """The three round-to-nearest bf16 planes of fp32-representable values (ops.split3_rows semantics), fp64."""
    t = t.float()
    p0 = t.bfloat16()
    r = t - p0.float()
    p1 = r.bfloat16()
    p2 = (r - p1.float()).bfloat16()
    return [p.double() for p in (p0, p1, p2)]


def split3_emulate(Vp, Up, Ho, Wo, kept=KEPT):
    """The SPLIT3 product in fp64 from the host-side planes: the kept cross products, then A^T . A."""
    out = 0
    for i, j in kept:
        out = out + y_of(Vp[i], Up[j], AT, Ho, Wo)
    return out


class Problem:
    """Logical operands of one forward problem (fp64 copies of exactly the fp32 values the kernels compute
    with), the fp64 reference, the absolute-value Winograd sum and the reference of each epilogue."""

    def __init__(self, grid, pad, Ci, Co, x, w, bias):
        self.grid, self.pad, self.Ci, self.Co = grid, pad, Ci, Co
        for t in (x, w, bias):
            assert torch.equal(t.float().double(), t)
        self.x, self.w, self.bias = x, w, bias  # NHWC, [Co][Ci][3][3], [Co]
        xp = pad_nchw(x, pad)
        self.Ho, self.Wo = xp.shape[-2] - 2, xp.shape[-1] - 2
        self.base = F.conv2d(xp, w).permute(0, 2, 3, 1).contiguous()
        self.V, self.U = v_of(tiles(xp)), u_of(w)
        self.S = y_of(v_of(tiles(xp).abs(), BT.abs()), u_of(w.abs(), G.abs()), AT.abs(), self.Ho, self.Wo)
        B = grid[0]
        m = torch.randint(-3, 4, (B, self.Ho, self.Wo, Co), generator=gen(7, Ci, Co, *grid)).double()
        m.view(-1)[::7] = -0.0
        m.view(-1)[3::7] = 0.0
        self.mask = m
        sb = torch.signbit(m)
        assert bool(((m == 0) & sb).any()) and bool(((m == 0) & ~sb).any()) and bool((m < 0).any()) and bool((m > 0).any())

    @property
    def w_packed(self):  # [Cout][9 Cin], k = tap * Cin + ci
        return self.w.permute(0, 2, 3, 1).reshape(self.Co, -1).contiguous()

    def ref(self, ep):
        """(fp64 reference, absolute-value sum) of epilogue ep."""
        y, mag = self.base, self.S
        if ep["bias"]:
            y = y + self.bias
            mag = mag + self.bias.abs()
        if ep["relu"]:
            y = torch.relu(y)
        if ep["mask"]:
            y = torch.where(self.mask > 0, y, torch.zeros_like(y))
        return y, mag

    def bound(self, route, mag):
        if ROUTES[route]["kernel"] == "wino_s3_kernel":
            return 2 * gamma(6 * self.Ci + 12) * mag + UR * mag
        return 2 * gamma(self.Ci + 12) * mag

    def exact_premises(self):
        """What the bit-for-bit comparison rests on (integer operands)."""
        for ep in EPILOGUES:
            y, mag = self.ref(ep)
            assert torch.equal(y.float().double(), y), "reference left the exact fp32 range"
            assert mag.max().item() < 2 ** 24, "absolute-value Winograd sum reaches 2^24"
        for t in (self.x, self.U, self.V, self.bias):
            assert torch.equal(t, t.round())


@functools.lru_cache(maxsize=None)
def problem(grid, pad, Ci, Co, exact):
    B, H, W = grid
    g = gen(1 + exact, Ci, Co, B, H, W, pad[1] + (pad[0] == "zero"))
    if exact:
        x = torch.randint(-4, 5, (B, H, W, Ci), generator=g).double()
        w = torch.randint(-2, 3, (Co, Ci, 3, 3), generator=g).double() * 4
        bias = torch.randint(-4, 5, (Co,), generator=g).double()
    else:  # the decoder's scale (test_wino_split3_fp64): values up to a few hundred
        x = (torch.rand(B, H, W, Ci, generator=g) * 400 - 120).double()
        w = (torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5).double()
        bias = torch.randn(Co, generator=g).double()
    return Problem(grid, pad, Ci, Co, x, w, bias)


def _grid_draw(spec, shape, g):
    kind, step, lim, arg = spec
    n = int(round(lim / step))
    if kind == "grid":  # multiples of step in [-lim, lim], a fraction arg of them zero
        t = torch.randint(-n, n + 1, shape, generator=g).double() * step
        if arg:
            t[torch.rand(shape, generator=g) < arg] = 0
        return t
    if kind == "onehot":  # x [B][H][W][Ci]: +-1 at the pixels (arg a, arg b) in one channel each, so that every
        B, H, W, Ci = shape  # 4 x 4 input patch holds at most one nonzero value; the channels cycle through Ci
        t = torch.zeros(shape, dtype=F64)
        idx = 0
        for b in range(B):
            for yy in range(0, H, arg):
                for xx in range(0, W, arg):
                    t[b, yy, xx, (7 * idx) % Ci] = 1.0 if idx % 3 else -1.0
                    idx += 1
        return t
    # "taps": a filter [Co][Ci][3][3] with arg nonzero taps per output channel, none of them a corner tap;
    # step == lim: the taps are +-lim (every U entry a power of two), else odd multiples of step in
    # (lim / 2, lim) (nine significant bits and more)
    Co, Ci = shape[:2]
    t = torch.zeros(shape, dtype=F64)
    where = ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1))
    for co in range(Co):
        for ci in torch.randperm(Ci, generator=g)[:arg].tolist():
            mag = lim if n == 1 else (2 * torch.randint(n // 4, n // 2, (), generator=g).item() + 1) * step
            sgn = 1 if torch.rand((), generator=g).item() < 0.5 else -1
            ky, kx = where[torch.randint(0, 5, (), generator=g).item()]
            t[co, ci, ky, kx] = sgn * mag
    return t


@functools.lru_cache(maxsize=None)
def plane_problem(case, Ci):
    """A SPLIT3 plane case with its premises asserted: returns (Problem, Vp, Up, q)."""
    c = PLANE_CASES[case]
    grid, pad, Co = BASE["grid"], BASE["pad"], BASE["Co"]
    B, H, W = grid
    g = gen(11, Ci, sorted(PLANE_CASES).index(case))
    x = _grid_draw(c["x"], (B, H, W, Ci), g)
    w = _grid_draw(c["w"], (Co, Ci, 3, 3), g)
    pb = Problem(grid, pad, Ci, Co, x, w, torch.zeros(Co, dtype=F64))
    q = c["x"][1] * (c["w"][1] / 4)  # V is a multiple of x's step, U of a quarter of w's
    assert torch.equal(pb.V.float().double(), pb.V) and torch.equal(pb.U.float().double(), pb.U)
    Vp, Up = planes(pb.V), planes(pb.U)
    assert torch.equal(Vp[0] + Vp[1] + Vp[2], pb.V) and torch.equal(Up[0] + Up[1] + Up[2], pb.U)
    # every term a multiple of q, the absolute-value sum over the planes below 2^24 q: exact in any order
    for t, step in ((pb.V, c["x"][1]), (pb.U, c["w"][1] / 4)):
        assert torch.equal((t / step).round() * step, t)
    Sp = y_of(sum(p.abs() for p in Vp), sum(p.abs() for p in Up), AT.abs(), pb.Ho, pb.Wo)
    assert Sp.max().item() < 2 ** 24 * q, (case, Ci, Sp.max().item() / q)
    pb.Sq = Sp.max().item() / q
    # plane occupancy: the named planes are filled, the planes above the case's top plane are empty
    share = lambda P, i: (P[i] != 0).double().mean().item()  # noqa: E731
    pb.shares = {"V": [share(Vp, i) for i in range(3)], "U": [share(Up, i) for i in range(3)]}
    op, i = c["share"]
    assert pb.shares[op][i] >= 0.25, (case, Ci, pb.shares)
    if "share_nz" in c:  # sparse filters: the share among U's nonzero entries
        op, i = c["share_nz"]
        pb.share_nz = pb.shares[op][i] / pb.shares[op][0]
        assert pb.share_nz >= 0.25, (case, Ci, pb.shares)
    for op, P in (("V", Vp), ("U", Up)):
        for i in range(c["top"][op] + 1, 3):
            assert not bool(P[i].any()), (case, Ci, op, i)
    # the six kept cross products give the reference exactly (the three dropped ones are zero)
    assert torch.equal(split3_emulate(Vp, Up, pb.Ho, pb.Wo), pb.base)
    assert torch.equal(pb.base.float().double(), pb.base)
    return pb, Vp, Up, q


class WgProblem:
    """Operands, fp64 dw / db and the absolute-value contractions of one weight-gradient problem."""

    def __init__(self, grid, zero, Ci, Co, exact):
        B, H, W = grid
        g = gen(21 + exact, Ci, Co, B, H, W, zero)
        if exact:
            x = torch.randint(-2, 3, (B, H, W, Ci), generator=g).double()
            gy = torch.randint(-2, 3, (B, H, W, Co), generator=g).double()
        else:
            x = torch.randn(B, H, W, Ci, generator=g).double()
            gy = torch.randn(B, H, W, Co, generator=g).double()
        self.grid, self.zero, self.Ci, self.Co, self.x, self.g = grid, zero, Ci, Co, x, gy
        xp = pad_nchw(x, ("zero", 1) if zero else ("reflect", 1))
        cols = F.unfold(xp, 3).view(B, Ci, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * Ci)
        self.dw = gy.reshape(-1, Co).T @ cols  # [Co][tap * Ci + ci]
        self.db = gy.reshape(-1, Co).sum(0)
        A = AT.T.abs()
        dY = gy.permute(0, 3, 1, 2).abs().unfold(2, 2, 2).unfold(3, 2, 2)  # [B][Co][ty][tx][2][2]
        Yh = torch.einsum("ij,botxjk,lk->botxil", A, dY, A)
        Vb = v_of(tiles(xp).abs(), BT.abs())
        dU = torch.einsum("botxil,bctxil->ocil", Yh, Vb)
        self.Sw = torch.einsum("ia,ocij,jb->oabc", G.abs(), dU, G.abs()).reshape(Co, 9 * Ci)
        self.Sb = gy.abs().reshape(-1, Co).sum(0)
        self.n = B * H * W


@functools.lru_cache(maxsize=None)
def wg_problem(grid, zero, Ci, Co, exact):
    return WgProblem(grid, zero, Ci, Co, exact)


def wg_exact_premises(pb):
    assert torch.equal(pb.dw.float().double(), pb.dw) and torch.equal(pb.db.float().double(), pb.db)
    assert 4 * pb.Sw.max().item() < 2 ** 24 and pb.Sb.max().item() < 2 ** 24  # in units of the 1/4 of G^T dU G


# --------------------------------------------------------------------------------------------------
# device side: guarded buffers and one call per run
# --------------------------------------------------------------------------------------------------
def ceil_to(x, m):
    return -(-x // m) * m


def nan_fill(n, dtype):
    if dtype == F32:
        return torch.full((n,), NAN32, dtype=torch.int32, device=DEV).view(F32)
    return torch.full((n,), NAN16, dtype=torch.int16, device=DEV).view(BF16)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


class Guarded:
    """A contiguous tensor of `shape` inside a larger allocation that holds the NaN pattern: GUARD rows (of the
    last dimension) before and after it, and the columns cols.. of every row (the padding of ldc / ldg)."""

    def __init__(self, dtype, shape, src=None, cols=None):
        self.dtype, self.shape, self.cols = dtype, tuple(shape), cols or shape[-1]
        self.n = math.prod(shape)
        self.g = ceil_to(GUARD * shape[-1], 8)
        self.flat = nan_fill(2 * self.g + self.n, dtype)
        self.t = self.flat[self.g:self.g + self.n].view(shape)
        if src is not None:
            self.t[..., :self.cols].copy_(src.to(dtype))

    def data(self):
        return self.t[..., :self.cols].clone()

    def intact(self):
        valid = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        valid[self.g:self.g + self.n].view(self.shape)[..., :self.cols] = True
        return bool((bits(self.flat)[~valid] == (NAN32 if self.dtype == F32 else NAN16)).all())


def prepack(pb, with_planes):
    """U (and the plane image) of pb's filters between guards, through the C entries."""
    Ci, Co = pb.Ci, pb.Co
    wp = Guarded(F32, (Co, 9 * Ci), pb.w_packed)
    U = Guarded(F32, (Ci // 8, 16, Co, 8))
    ops._call("mhada_wino_weights", wp.t, wp.t.data_ptr(), U.t.data_ptr(), Co, Ci)
    P = None
    if with_planes:
        P = Guarded(BF16, (Ci // 16, 16, 3, Co, 16))
        ops._call("mhada_wino_weights_split3", wp.t, wp.t.data_ptr(), P.t.data_ptr(), Co, Ci)
    torch.cuda.synchronize()
    assert U.intact() and (P is None or P.intact()), "prepack wrote outside its image"
    if P is not None:
        U.t.split3 = P.t
    return U, P


def u_logical(U):
    """[Cin/8][16][Cout][8] -> [Cout][Cin][4][4] (fp64)."""
    n8, _, Co, _ = U.shape
    return U.double().permute(2, 0, 3, 1).reshape(Co, n8 * 8, 4, 4)


def run_conv(fm, pb, U, ep, ldc):
    """One conv3x3_wino call with every operand between guards; y [B][Ho][Wo][Cout] after the guard check."""
    B = pb.grid[0]
    x = Guarded(F32, pb.x.shape, pb.x)
    bias = Guarded(F32, (pb.Co,), pb.bias) if ep["bias"] else None
    mask = Guarded(F32, (B, pb.Ho, pb.Wo, ldc), pb.mask, cols=pb.Co) if ep["mask"] else None
    y = Guarded(F32, (B, pb.Ho, pb.Wo, ldc), cols=pb.Co)
    with _lib.tuning(**fm["knobs"]):
        ops.conv3x3_wino(x.t, U.t, bias.t if bias else None, ep["relu"], pb.pad[0], pb.pad[1], out=y.t,
                         relu_mask=mask.t if mask else None)
    torch.cuda.synchronize()
    assert y.intact(), f"{fm['name']} {ep} ldc={ldc}: y written outside [B][Ho][Wo][Cout]"
    for b in (x, bias, mask):
        assert b is None or b.intact()
    return y.data()


def check(fm, exact):
    pb = problem(fm["grid"], fm["pad"], fm["Ci"], fm["Co"], exact)
    if exact:
        pb.exact_premises()
    U, _ = prepack(pb, fm["planes"])
    Co, worst = pb.Co, 0.0
    outs = {}
    for ep in EPILOGUES + [dict(bias=True, relu=False, mask=False)]:  # (the last: the unmasked twin of bias + mask)
        ref, mag = pb.ref(ep)
        dense, padded = run_conv(fm, pb, U, ep, Co), run_conv(fm, pb, U, ep, Co + 4)
        what = f"{fm['name']} {ep}"
        assert torch.equal(bits(dense), bits(padded)), what + ": the padded run differs from the dense run"
        outs[ep["bias"], ep["relu"], ep["mask"]] = dense
        if exact:
            assert torch.equal(bits(dense), bits(ref.float().to(DEV))), what + ": not the fp64 reference's bits"
        else:
            ratio = ((dense.double().cpu() - ref).abs() / pb.bound(fm["route"], mag).clamp_min(1e-300)).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, what + f": error / bound = {ratio:.3f}"
    for ep in EPILOGUES:
        if ep["mask"]:  # +0.0 wherever the mask is not positive (its +-0.0 entries too), the unmasked bits elsewhere
            got = outs[ep["bias"], ep["relu"], True]
            keep = (pb.mask > 0).to(DEV)
            want = torch.where(keep, bits(outs[ep["bias"], ep["relu"], False]), torch.zeros_like(bits(got)))
            assert torch.equal(bits(got), want), f"{fm['name']} {ep}: relu_mask"
    return worst


@pytest.mark.parametrize("fm", FORMS)
def test_form_exact_and_canaries(fm):
    """Integer operands: every output bit for bit, dense and padded, masked and not, guards intact."""
    check(fm, exact=True)


@pytest.mark.parametrize("fm", FORMS)
def test_form_componentwise_bound(fm):
    """Gaussian operands at the decoder's scale: the componentwise bound of the module docstring."""
    worst = check(fm, exact=False)
    print(f"BOUND {fm['name']:36s} {fm['kernel']:16s} worst error/bound = {worst:.4f}")


@pytest.mark.parametrize("case,Ci", PLANE_FORMS)
def test_split3_planes(case, Ci):
    """wino_s3_kernel on operands that occupy the case's bf16 planes: exact only if every plane and every
    kept cross product reaches the accumulator (premises asserted in plane_problem)."""
    pb, Vp, Up, q = plane_problem(case, Ci)
    fm = dict(BASE, route="s3", name=f"planes_{case}_cin{Ci}", **ROUTES["s3"])
    U, P = prepack(pb, True)
    # the device's plane image is the host's: U's planes as the emulation used them
    up = P.t.double().cpu().permute(2, 3, 0, 4, 1).reshape(3, pb.Co, Ci, 4, 4)  # [plane][Co][Ci][4][4]
    for i in range(3):
        assert torch.equal(up[i], Up[i]), f"{case}: plane {i} of the device's U image"
    ep = dict(bias=False, relu=False, mask=False)
    for ldc in (pb.Co, pb.Co + 4):
        y = run_conv(fm, pb, U, ep, ldc)
        assert torch.equal(bits(y), bits(pb.base.float().to(DEV))), f"{case} Cin {Ci} ldc {ldc}: not the reference's bits"
    print(f"PLANES {case:5s} Cin {Ci}: sum / q = {pb.Sq:.3g}, V shares {pb.shares['V']}, U shares {pb.shares['U']}")


# --------------------------------------------------------------------------------------------------
# prepacks
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ci,Co", [(8, 64), (16, 64), (16, 128), (24, 64), (48, 128)])
def test_prepacks(Ci, Co):
    """wino_weights against the fp64 G g G^T: bit for bit on the integer filters; on Gaussian ones within the
    four roundings of the transform (two per stage, the halvings exact), half an ulp each: gamma_4 = 2 ulp at
    the top of a binade, of the absolute-value transform |G| |g| |G|^T (the sums a + b + c cancel, so no fp32
    evaluation holds 2 ulp of the result itself).  wino_weights_split3: the plane sum, smallest first, is the
    fp32 U and the planes are the host's split; both between guards; the ops wrappers return the same images."""
    for exact in (True, False):
        pb = problem((1, 2, 2), ("reflect", 1), Ci, Co, exact)
        U, P = prepack(pb, Ci % 16 == 0)
        got = u_logical(U.t.cpu())
        if exact:
            assert torch.equal(got, pb.U)
        else:
            assert bool(((got - pb.U).abs() <= gamma(4) * u_of(pb.w.abs(), G.abs())).all())
        wp = pb.w_packed.float().to(DEV)
        uo = ops.wino_weights(wp)
        assert torch.equal(bits(uo), bits(U.t))
        if P is not None:
            up = P.t.float()  # [Ci/16][16][3][Co][16]
            s = (up[:, :, 2] + up[:, :, 1]) + up[:, :, 0]
            uu = U.t.view(Ci // 16, 2, 16, Co, 8).permute(0, 2, 3, 1, 4).reshape(Ci // 16, 16, Co, 16)
            assert torch.equal(bits(s), bits(uu))
            assert torch.equal(bits(uo.split3), bits(P.t)) and torch.equal(bits(ops.wino_weights_split3(wp)), bits(P.t))
            hp = planes(pb.U if exact else u_logical(U.t.cpu()))
            dp = P.t.double().cpu().permute(2, 3, 0, 4, 1).reshape(3, Co, Ci, 4, 4)
            for i in range(3):
                assert torch.equal(dp[i], hp[i]), f"plane {i}"


# --------------------------------------------------------------------------------------------------
# weight gradient
# --------------------------------------------------------------------------------------------------
def run_wgrad(fm, pb, ldg, with_db):
    """mhada_conv3x3_wgrad_wino through the C entry; (dw, db or None, S) after the guard checks."""
    B, H, W = pb.grid
    Ci, Co = pb.Ci, pb.Co
    S0 = _lib.load().mhada_conv3x3_wgrad_wino_splits(B, H, W, Ci, Co)
    per = 16 * Co * Ci + (Co if with_db else 0)
    extra = 128  # floats past the slabs that the call is told about and must leave alone
    wf = (per if fm["one_slab"] else S0 * per) + extra
    nchunk = B * (H // 2) * (W // 16)
    S = min(S0, wf // per)
    cps = -(-nchunk // S)
    S = -(-nchunk // cps)
    assert S == fm["S"], (S, fm["S"])
    if fm["name"].endswith("_50chunks"):
        assert nchunk - (S - 1) * cps == cps - 1  # the last split is one chunk short
    x = Guarded(F32, pb.x.shape, pb.x)
    g = Guarded(F32, (B, H, W, ldg), pb.g, cols=Co)
    dw = Guarded(F32, (Co, 9 * Ci))
    db = Guarded(F32, (Co,)) if with_db else None
    work = Guarded(F32, (wf // 64, 64))
    ops._call("mhada_conv3x3_wgrad_wino", x.t, x.t.data_ptr(), g.t.data_ptr(), dw.t.data_ptr(),
              db.t.data_ptr() if with_db else None, work.t.data_ptr(), wf, B, H, W, Ci, Co, ldg,
              _lib.PAD_ZERO if pb.zero else _lib.PAD_REFLECT)
    torch.cuda.synchronize()
    what = f"{fm['name']} ldg={ldg} db={with_db}"
    assert dw.intact() and (db is None or db.intact()) and work.intact() and x.intact() and g.intact(), what + ": guards"
    assert bool((bits(work.t.view(-1)[S * per:]) == NAN32).all()), what + ": workspace written beyond S * per"
    return dw.data(), db.data() if with_db else None


def check_wgrad(fm, exact):
    pb = wg_problem(fm["grid"], fm["zero"], fm["Ci"], fm["Co"], exact)
    if exact:
        wg_exact_premises(pb)
    worst = [0.0, 0.0]
    first = None
    for ldg in (pb.Co, pb.Co + 4):
        for with_db in (True, False):
            dw, db = run_wgrad(fm, pb, ldg, with_db)
            what = f"{fm['name']} ldg={ldg} db={with_db}"
            if first is None:
                first = dw
            assert torch.equal(bits(dw), bits(first)), what + ": dw depends on ldg / db"
            for i, (got, ref, S, n) in enumerate(((dw, pb.dw, pb.Sw, pb.n + 9), (db, pb.db, pb.Sb, pb.n))):
                if got is None:
                    continue
                if exact:
                    assert torch.equal(bits(got), bits(ref.float().to(DEV))), what + (": db" if i else ": dw")
                else:
                    ratio = ((got.double().cpu() - ref).abs() / (2 * gamma(n) * S).clamp_min(1e-300)).max().item()
                    worst[i] = max(worst[i], ratio)
                    assert ratio <= 1.0, what + f": {'db' if i else 'dw'} error / bound = {ratio:.3f}"
    return worst, first


@pytest.mark.parametrize("fm", WG_FORMS)
def test_wgrad_exact_and_canaries(fm):
    """Integer operands: dw and db bit for bit for every ldg, with and without db, guards intact."""
    check_wgrad(fm, exact=True)


@pytest.mark.parametrize("fm", WG_FORMS)
def test_wgrad_componentwise_bound(fm):
    worst, _ = check_wgrad(fm, exact=False)
    print(f"BOUND {fm['name']:36s} worst error/bound: dw {worst[0]:.4f} db {worst[1]:.4f}")


@pytest.mark.parametrize("zero", [False, True])
def test_wgrad_same_bits_for_every_split_count(zero):
    """The 50-chunk shape with S = 3 and S = 1 (integer operands: both are the fp64 bits, asserted above;
    here against each other)."""
    t = "zero" if zero else "reflect"
    fms = {p.values[0]["name"]: p.values[0] for p in WG_FORMS}
    _, a = check_wgrad(fms[f"wg_{t}_50chunks"], exact=True)
    _, b = check_wgrad(fms[f"wg_{t}_50chunks_1slab"], exact=True)
    assert torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------
# rejections
# --------------------------------------------------------------------------------------------------
def test_conv_rejections_leave_y_untouched():
    B, H, W, Ci, Co = 1, 4, 4, 16, 64
    x = torch.ones(B * H * W * Ci + 8, device=DEV)
    u = torch.ones(Ci * 16 * Co + 8, device=DEV)
    up = torch.ones(Ci * 48 * Co + 8, device=DEV, dtype=BF16)
    y = Guarded(F32, (B, H + 2, W + 2, Co))
    R, Z = _lib.PAD_REFLECT, _lib.PAD_ZERO

    def rejected(match, entry="mhada_conv3x3_wino", **over):
        a = dict(x=x.data_ptr(), u=u.data_ptr(), up=up.data_ptr(), bias=None, y=y.t.data_ptr(), B=B, H=H, W=W, Ci=Ci,
                 Co=Co, ldc=Co, mode=R, pad=1, relu=0, mask=None)
        a.update(over)
        args = [a["x"], a["u"]] + ([a["up"]] if entry.endswith("split3") else []) + \
            [a[k] for k in ("bias", "y", "B", "H", "W", "Ci", "Co", "ldc", "mode", "pad", "relu", "mask")]
        with pytest.raises(ValueError, match=match):
            ops._call(entry, x, *args)
        torch.cuda.synchronize()
        assert bool((bits(y.flat) == NAN32).all()), match

    for entry in ("mhada_conv3x3_wino", "mhada_conv3x3_wino_split3"):
        rejected("mhada_conv3x3_wino: bad args", entry, H=1)
        rejected("mhada_conv3x3_wino: bad args", entry, y=None)
        rejected("needs Cin % 8 == 0 and Cout % 64 == 0", entry, Ci=12)
        rejected("needs Cin % 8 == 0 and Cout % 64 == 0", entry, Co=96)
        rejected("bad pad_mode", entry, mode=2)
        rejected("zero pad must be 1 or 2", entry, mode=Z, pad=3)
        rejected("ldc < Cout", entry, ldc=Co - 4)
        rejected("x and u must be 16-byte aligned", entry, x=x.data_ptr() + 4)
        rejected("x and u must be 16-byte aligned", entry, u=u.data_ptr() + 8)
        rejected("too large for 32-bit indexing", entry, B=2 ** 27)
    rejected("mhada_conv3x3_wino_split3: bad args", "mhada_conv3x3_wino_split3", up=None)
    rejected("up must be 16-byte aligned", "mhada_conv3x3_wino_split3", up=up.data_ptr() + 2)


def test_prepack_rejections_leave_u_untouched():
    Co = 64
    w = torch.ones(Co * 9 * 16, device=DEV)
    for entry, dtype, match, bad in (("mhada_wino_weights", F32, r"bad args \(Cin % 8 == 0\)", 12),
                                     ("mhada_wino_weights_split3", BF16, r"bad args \(Cin % 16 == 0\)", 8)):
        out = Guarded(dtype, (16 * 16 * Co * 3,))
        for args in ((w.data_ptr(), out.t.data_ptr(), Co, bad), (None, out.t.data_ptr(), Co, 16),
                     (w.data_ptr(), None, Co, 16), (w.data_ptr(), out.t.data_ptr(), 0, 16)):
            with pytest.raises(ValueError, match=entry + ": " + match):
                ops._call(entry, w, *args)
        torch.cuda.synchronize()
        assert bool((bits(out.flat) == (NAN32 if dtype == F32 else NAN16)).all())


def test_wgrad_rejections_leave_outputs_untouched():
    B, H, W, Ci, Co = 1, 2, 16, 64, 64
    x = torch.ones(B * H * W * Ci + 8, device=DEV)
    g = torch.ones(B * H * W * (Co + 4) + 8, device=DEV)
    per = 16 * Co * Ci + Co
    dw, db, work = Guarded(F32, (Co, 9 * Ci)), Guarded(F32, (Co,)), Guarded(F32, (per // 4, 4))

    def rejected(match, **over):
        a = dict(x=x.data_ptr(), g=g.data_ptr(), dw=dw.t.data_ptr(), db=db.t.data_ptr(), work=work.t.data_ptr(), wf=per,
                 B=B, H=H, W=W, Ci=Ci, Co=Co, ldg=Co, mode=_lib.PAD_REFLECT)
        a.update(over)
        with pytest.raises(ValueError, match=match):
            ops._call("mhada_conv3x3_wgrad_wino", x, *a.values())
        torch.cuda.synchronize()
        for b in (dw, db, work):
            assert bool((bits(b.flat) == NAN32).all()), match

    rejected("bad args", work=None)
    rejected("bad args", B=0)
    rejected("needs Cin % 64 == 0, Cout % 64 == 0, H even, W % 16 == 0", Ci=32)
    rejected("needs Cin % 64 == 0, Cout % 64 == 0, H even, W % 16 == 0", H=3)
    rejected("needs Cin % 64 == 0, Cout % 64 == 0, H even, W % 16 == 0", W=24)
    rejected("bad pad_mode", mode=2)
    rejected("ldg >= Cout, ldg % 4 == 0", ldg=Co - 4)
    rejected("ldg >= Cout, ldg % 4 == 0", ldg=Co + 2)
    rejected("16-byte aligned x, g, work", g=g.data_ptr() + 4)
    rejected("16-byte aligned x, g, work", work=work.t.data_ptr() + 8)
    rejected("too large for 32-bit indexing", B=2 ** 24)
    rejected("workspace smaller than", wf=per - 1)
    rejected("workspace smaller than", wf=16 * Co * Ci)  # room for the slab, not for the bias partials


def test_zz_knobs_are_back_at_their_defaults():
    """Last in the module: every tuning() context above restored its knobs."""
    for k, v in DEFAULT_KNOBS.items():
        assert _lib.get_tuning(k) == v, k
