"""mhada_gemm_half2 and its operand writers on the GPU: exact-arithmetic cases that pin every term, the
column scale and every epilogue element by element (all buffers between NaN guards), Gaussian operands
against fp64 at the bound of test_linear_split3_fp32_accuracy, the plane writers against the Python
formulas bit for bit, and the argument refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mhada_hip import ops
    DEV = "cuda"

GUARD = 64  # elements of NaN pattern on either side of every buffer
# (M, N, K0, lda): the GEMM form shapes — one K chunk, three chunks with lda > K0, and more tiles than
# workgroups (130 x 2: the persistent loop, the lazy store drain, an 8-column partial tile, a partial row tile)
SHAPES = [(300, 260, 64, 64), (300, 260, 192, 200), (33180, 264, 128, 128)]


def guarded(shape, dtype):
    """A NaN-filled (integer types: 0x7f..) tensor of `shape` inside a larger NaN-filled allocation."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=dtype)
    return flat, flat[GUARD:GUARD + n].view(*shape)


def guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def ints(shape, lim, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def split3(x):
    p0 = x.bfloat16()
    r = x - p0.float()
    p1 = r.bfloat16()
    return torch.stack([p0, p1, (r - p1.float()).bfloat16()])


def run(a_hi, a_lo, w_hi, w_lo, cs, lda, bias=None, relu=False, out="f32", pad=0):
    """mhada_gemm_half2 on explicit planes (fp64 tensors holding fp16-exact values); returns (result,
    list of guarded allocations).  out: "f32" | "bf16" | "planes"; pad: ldc = N + pad."""
    M, K0 = a_hi.shape
    N = w_hi.shape[0]
    allocs = []

    def buf(shape, dtype):
        flat, v = guarded(shape, dtype)
        allocs.append(flat)
        return v
    a = buf((2, M, lda), torch.float16)
    a[0, :, :K0] = a_hi.to(DEV, torch.float16)
    a[1, :, :K0] = a_lo.to(DEV, torch.float16)
    w = buf((N, K0 // 64, 2, 64), torch.float16)
    w[:, :, 0] = w_hi.view(N, K0 // 64, 64).to(DEV, torch.float16)
    w[:, :, 1] = w_lo.view(N, K0 // 64, 64).to(DEV, torch.float16)
    csb = buf((N,), torch.float32)
    csb.copy_(cs)
    bb = None
    if bias is not None:
        bb = buf((N,), torch.float32)
        bb.copy_(bias)
    ldc = N + pad
    kw = dict(a=a, w=w, M=M, N=N, K=K0, compute=torch.float16, lda=lda, ldw=2 * K0, bias=bb, relu=relu, ldc=ldc,
              col_scale=csb)
    if out == "planes":
        c2 = buf((3, M, ldc), torch.bfloat16)
        ops.gemm(c=None, c2=c2, ldc2=ldc, c2_planes=True, **kw)
        res = c2
    else:
        c = buf((M, ldc), torch.float32 if out == "f32" else torch.bfloat16)
        ops.gemm(c=c, **kw)
        res = c
    torch.cuda.synchronize()
    return res, allocs


def check(res, allocs, ref32, out, pad):
    """ref32: the exact result, fp32-representable.  Element by element, padding columns and guards untouched."""
    N = ref32.shape[1]
    for f in allocs:
        assert guards_intact(f)
    if out == "planes":
        exp = split3(ref32)
        assert torch.equal(res[:, :, :N].view(torch.int16), exp.view(torch.int16))
        assert torch.isnan(res[:, :, N:]).all()
    else:
        exp = ref32 if out == "f32" else ref32.bfloat16()
        assert torch.equal(res[:, :N], exp)
        assert torch.isnan(res[:, N:]).all()


@pytest.fixture(scope="module")
def int_case():
    """Integer operands per shape, |x| <= 2048 (lo = 0), |w| <= 2: sums below 2^20; the fp64 reference."""
    cache = {}

    def get(shape):
        if shape not in cache:
            M, N, K0, _ = shape
            x, w = ints((M, K0), 2048, 1), ints((N, K0), 2, 2)
            x[0, 0], x[M - 1, K0 - 1] = 2048, -2048
            cs = torch.exp2(-(torch.arange(N) % 4).double())          # 1, 1/2, 1/4, 1/8 by column
            bias = ((torch.arange(N) % 13) - 6).double() / 8
            cache[shape] = (x, w, cs, bias, (x.to(DEV) @ w.to(DEV).T).cpu())
        return cache[shape]
    return get


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("out,relu,with_bias", [("f32", False, False), ("f32", False, True), ("f32", True, True),
                                                ("bf16", False, True), ("bf16", True, True), ("planes", True, True),
                                                ("planes", False, False)])
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_operands_give_the_fp64_bits(int_case, shape, out, relu, with_bias, pad):
    x, w, cs, bias, xw = int_case(shape)
    ref = xw * cs[None, :]
    if with_bias:
        ref = ref + bias[None, :]
    if relu:
        ref = torch.relu(ref)
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref)  # the fp64 reference is fp32-representable: compare bits
    zero = torch.zeros_like
    res, allocs = run(x, zero(x), w, zero(w), cs.float(), shape[3], bias.float() if with_bias else None, relu, out, pad)
    check(res, allocs, ref32.to(DEV), out, pad)


@pytest.mark.parametrize("which", ["a_lo", "w_lo"])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_dyadic_lo_planes_reach_the_accumulator(shape, which):
    """Only A (or only W) has lo != 0; lo lo = 0 by construction: exact iff lo hi (or hi lo) is summed."""
    M, N, K0, lda = shape
    hi_a, hi_w = ints((M, K0), 32, 3), ints((N, K0), 4, 4)
    lo_a, lo_w = torch.zeros(M, K0).double(), torch.zeros(N, K0).double()
    if which == "a_lo":
        lo_a = ints((M, K0), 8, 5) / 64
    else:
        lo_w = ints((N, K0), 8, 6) / 64
    ref = (hi_a + lo_a) @ (hi_w + lo_w).T
    assert not torch.equal(ref, hi_a @ hi_w.T)
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref)
    res, allocs = run(hi_a, lo_a, hi_w, lo_w, torch.ones(N), lda)
    check(res, allocs, ref32.to(DEV), "f32", 0)


def test_column_scale_is_per_column_and_before_the_bias():
    """Weight rows 2^20 apart and a zero row through half2_weight: cs[n] = 1 / t_n undoes each row's scale
    exactly; the bias is added to the rescaled column (an fp32 add, as the reference's)."""
    M, N, K0 = 300, 260, 64
    x, w = ints((M, K0), 2048, 7), ints((N, K0), 7, 8)
    w[1::2] *= 2.0 ** 20
    w[5] = 0
    w2, t = ops.half2_weight(w.float())
    assert t[5] == 1 and t.max() / t.min() >= 2.0 ** 20
    w2 = w2.view(N, K0 // 64, 2, 64).double()
    bias = (torch.arange(N) % 7).float() / 2 + 0.5
    ref32 = ((x @ w.T).float() + bias[None, :]).to(DEV)
    assert torch.equal((x @ w.T).float().double(), x @ w.T)
    res, allocs = run(x, torch.zeros_like(x), w2[:, :, 0].reshape(N, K0), w2[:, :, 1].reshape(N, K0), 1.0 / t, K0, bias)
    check(res, allocs, ref32, "f32", 0)
    assert torch.equal(res[:, 5], bias[5].to(DEV).expand(M))


RATIOS = []


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,N,K0", [(4096, 1536, 512), (1000, 2048, 512), (300, 256, 256)])
def test_gaussian_operands_fp32_accuracy(M, N, K0, relu):
    """test_linear_split3_fp32_accuracy's construction through the HALF2 operand writers: against fp64
    < 2e-6 and <= 2.5 x the fp32 MFMA GEMM's error + 1e-7 on the same operands; run-to-run bit-identical."""
    x = rnd(M, K0, seed=1) * 2
    w = rnd(N, K0, scale=K0 ** -0.5, seed=2)
    b = rnd(N, seed=3)
    g1, b0 = torch.ones(K0, device=DEV), torch.zeros(K0, device=DEV)
    y = ops.layernorm(x, g1, b0, torch.float32, 1e-6)
    h = ops.half2_prepare(g1, b0, w)
    assert h is not None
    pl = ops.layernorm_half2(x, g1, b0, 1e-6, h["s_a"])
    out = ops.linear_half2(pl, h["w2"], h["cs"], b, torch.float32, relu=relu)
    out2 = ops.linear_half2(pl, h["w2"], h["cs"], b, torch.float32, relu=relu)
    assert torch.equal(out, out2)
    ref = y.double() @ w.double().T + b.double()
    if relu:
        ref = torch.relu(ref)
    e_h2, e_f32 = rel(out, ref), rel(ops.linear(y, w, b, torch.float32, relu=relu), ref)
    RATIOS.append(e_h2 / e_f32)
    print(f"half2 {M}x{N}x{K0} relu={int(relu)}: e_h2 {e_h2:.3e} e_f32 {e_f32:.3e} ratio {e_h2 / e_f32:.2f} "
          f"(largest so far {max(RATIOS):.2f})")
    assert e_h2 < 2e-6, (e_h2, e_f32)
    assert e_h2 <= 2.5 * e_f32 + 1e-7, (e_h2, e_f32)
    # the plane output is the split of exactly that result
    pl3 = ops.linear_half2(pl, h["w2"], h["cs"], b, torch.float32, relu=relu, out_planes=True)
    assert torch.equal(pl3.view(torch.int16), split3(out).view(torch.int16))


def test_layernorm_half2_planes_are_the_python_formula():
    cols = 512
    x = rnd(1001, cols, seed=11) * 3 + 0.5
    g = rnd(cols, seed=12)
    g[17] = 1e-9  # one tiny channel: its plane values fall below the fp16 normal range
    b = rnd(cols, seed=13)
    b[17] = 0
    s_a = ops.half2_a_scale(g, b)
    y32 = ops.layernorm(x, g, b, torch.float32, 1e-6)
    hi, lo = ops._half2_planes(y32 * s_a)
    pl = ops.layernorm_half2(x, g, b, 1e-6, s_a)
    assert (pl.float().abs() <= 32768).all()
    assert torch.equal(pl[0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(pl[1].view(torch.int16), lo.view(torch.int16))
    assert (pl[:, :, 17] == 0).all() and (pl[0] != 0).any() and (pl[1] != 0).any()


def test_half2_weight_dev_equals_half2_weight():
    w = rnd(300, 512, scale=0.04, seed=21)
    w[1] = 0
    w[2] *= 1e-6
    w[3] *= 2.0 ** 20
    w[4, 1:] = 0
    w[4, 0] = 0.5
    w2d, td = ops.half2_weight_dev(w)
    w2, t = ops.half2_weight(w)
    assert torch.equal(td, t)
    assert torch.equal(w2d.view(torch.int16), w2.view(torch.int16))


def test_argument_refusals():
    a = torch.zeros(2, 64, 128, device=DEV, dtype=torch.float16)
    w = torch.zeros(64, 256, device=DEV, dtype=torch.float16)
    cs = torch.ones(64, device=DEV)
    c = torch.zeros(64, 64, device=DEV)
    kw = dict(a=a, w=w, c=c, compute=torch.float16, lda=128, ldw=256, ldc=64, col_scale=cs)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.gemm(M=64, N=64, K=96, **kw)
    with pytest.raises(ValueError, match="one problem"):
        ops.gemm(M=64, N=64, K=64, nb=(2, 1), **kw)
    big = torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="col_scale"):
        ops.gemm(M=64, N=64, K=64, **{**kw, "col_scale": big})
    with pytest.raises(ValueError, match="2\\^31 tiles"):
        ops.gemm(M=2 ** 31 - 1, N=2 ** 31 - 1, K=64, **{**kw, "col_scale": cs[:1].expand(2 ** 31 - 1)})
    ops.gemm(M=64, N=64, K=64, **kw)  # the same arguments at a supported shape run
    torch.cuda.synchronize()
    assert (c == 0).all()
