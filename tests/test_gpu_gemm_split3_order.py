"""The SPLIT3 GEMM's plane-once term order (gemm_s3_kernel, tuning gemm_s3_order): each chunk's six
cross products run as (p2,q0) (p1,q0) (p1,q1) (p0,q1) (p0,q2) (p0,q0) on separate A and W rings.

Shapes are the smallest at which the rings can go wrong: one chunk per tile (K0 = 64: chunk and tile
boundary coincide), two, and an odd count (K0 = 192: the A ring's parity differs from tile to tile);
a partial row tile; more output tiles than CUs (the rings run on across a tile boundary)."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


SHAPES = [(M, N, K0) for K0 in (64, 128, 192) for M in (257, 4100) for N in (256, 768)]
SHAPES.append((4100, 4096, 64))  # 17 x 16 = 272 tiles: more than one tile per workgroup on 256 CUs


@pytest.mark.parametrize("M,N,K0", SHAPES)
def test_split3_order_small_shapes_fp64(M, N, K0):
    """Against fp64 with the bounds of test_linear_split3_fp32_accuracy (< 2e-6 and within 2.5x of the
    fp32 MFMA GEMM's error + 1e-7): plain, with a residual (preloaded into the accumulators), with
    ReLU, and with the result written as planes; every call bit-identical when repeated."""
    assert _lib.get_tuning("gemm_s3_order") == 1
    x = rnd(M, K0, seed=1) * 2
    w = rnd(N, K0, scale=K0 ** -0.5, seed=2)
    b = rnd(N, seed=3)
    r = rnd(M, N, seed=4)
    pl = ops.split3_rows(x)
    w6 = ops.split3_weight(w)
    base = x.double() @ w.double().T + b.double()
    for relu, res in ((False, False), (False, True), (True, False)):
        rr = r if res else None
        out = ops.linear_split3(pl, w6, b, torch.float32, residual=rr, relu=relu)
        assert torch.equal(out, ops.linear_split3(pl, w6, b, torch.float32, residual=rr, relu=relu))
        ref = torch.relu(base) if relu else base
        if res:
            ref = ref + r.double()
        f32 = ops.linear(x, w, b, torch.float32, residual=rr, relu=relu)
        e_split, e_f32 = rel(out, ref), rel(f32, ref)
        print(f"M={M} N={N} K0={K0} relu={relu} res={res}: e_split={e_split:.3e} e_f32={e_f32:.3e}")
        assert e_split < 2e-6, (relu, res, e_split, e_f32)
        assert e_split <= 2.5 * e_f32 + 1e-7, (relu, res, e_split, e_f32)
        # the same result as planes: plane 0 its bf16 rounding, the sum within 2^-26, same bounds
        op = ops.linear_split3(pl, w6, b, torch.float32, residual=rr, relu=relu, out_planes=True)
        assert torch.equal(op[0], out.bfloat16())
        s = op[0].double() + op[1].double() + op[2].double()
        assert ((s - out.double()).abs() <= out.double().abs() * 2.0 ** -26).all()
        e_pl = rel(s, ref)
        print(f"    out_planes: e_planes={e_pl:.3e}")
        assert e_pl < 2e-6 and e_pl <= 2.5 * e_f32 + 1e-7, (relu, res, e_pl, e_f32)


def _signed_sparse(rows, cols, nnz, seed):
    """[rows][cols] of 0 / +-1 with `nnz` non-zeros per row at random columns."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.rand(rows, cols, generator=g).argsort(dim=1)[:, :nnz]
    sign = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.float64).scatter_(1, idx, sign)


@pytest.mark.parametrize("a_planes,w_planes", [(3, 1), (1, 3), (2, 2)])
def test_split3_order_exact_pairing(a_planes, w_planes):
    """Operands whose planes are known and whose kept cross products sum exactly in fp32, so the
    kernel must return that sum bit for bit in any order: a missing, doubled or mispaired term shows.
    x = a0 + a1 2^-10 + a2 2^-20 with a_i in {0, +-1} on 12 of the 64 columns of each row (each
    component with its own signs), w likewise: round-to-nearest bf16 splitting gives p_i = a_i 2^-10i
    (|a1 2^-10 + a2 2^-20| is under half a bf16 ulp of 1 on either side, likewise one level down), every
    product is +-2^-10(i+j), and a row pair shares at most 12 columns, so every partial sum is a
    multiple of 2^-20 below 16: 24 bits."""
    M, N, K0, nnz = 300, 256, 64, 12
    S = (1.0, 2.0 ** -10, 2.0 ** -20)

    def operand(rows, nplanes, seed):
        mask = _signed_sparse(rows, K0, nnz, seed).abs()
        planes = []
        for i in range(3):
            sg = _signed_sparse(rows, K0, K0, seed + 10 * (i + 1))  # dense signs, masked below
            planes.append(sg * mask * S[i] if i < nplanes else torch.zeros(rows, K0, dtype=torch.float64))
        return planes

    P = operand(M, a_planes, 100)
    Q = operand(N, w_planes, 200)
    x64, w64 = P[0] + P[1] + P[2], Q[0] + Q[1] + Q[2]
    assert torch.equal(x64.float().double(), x64) and torch.equal(w64.float().double(), w64)
    # the CPU check: the fp64 sum of the six kept plane products is its own fp32 rounding
    ref = sum(P[i] @ Q[j].T for i in range(3) for j in range(3) if i + j <= 2)
    assert torch.equal(ref.float().double(), ref)
    assert ref.abs().max() < 16 and torch.equal((ref * 2.0 ** 20).round(), ref * 2.0 ** 20)
    pl = ops.split3_rows(x64.float().to(DEV))
    w6 = ops.split3_weight(w64.float().to(DEV))
    for i in range(3):  # the planes are the intended ones
        assert torch.equal(pl[i].double().cpu(), P[i])
    blocks = w6.view(N, 1, 6, 64).double().cpu()
    for t, j in enumerate((1, 0, 2, 0, 1, 0)):
        assert torch.equal(blocks[:, 0, t], Q[j])
    out = ops.linear_split3(pl, w6, None, torch.float32)
    assert torch.equal(out.double().cpu(), ref)
    with _lib.tuning(gemm_s3_order=0):
        old = ops.linear_split3(pl, w6, None, torch.float32)
    assert torch.equal(old, out)


# sha256 of the fp32 output below from a library built from the parent commit (the six-K-tile walk was
# the only SPLIT3 GEMM there; profiles/r08_parent_sha.log holds that run beside the knob-off run of this
# build); inputs are seeded on the CPU and split on the device by kernels this change does not touch
PARENT_SHA256 = "045efe4eed07738aaa3bae08ae59f9034456f04469d72b33bc83cda6c722726c"


def test_split3_order_knob_off_is_the_parent():
    """gemm_s3_order = 0 runs the parent's kernel: same bits as a build of the parent on a mid-size
    shape (several chunks, partial row tile, bias and residual); knob on agrees with it within the
    fp64 bound of both."""
    M, N, K0 = 2000, 768, 256
    x = rnd(M, K0, seed=21) * 2
    w = rnd(N, K0, scale=K0 ** -0.5, seed=22)
    b = rnd(N, seed=23)
    r = rnd(M, N, seed=24)
    pl = ops.split3_rows(x)
    w6 = ops.split3_weight(w)
    with _lib.tuning(gemm_s3_order=0):
        old = ops.linear_split3(pl, w6, b, torch.float32, residual=r)
    new = ops.linear_split3(pl, w6, b, torch.float32, residual=r)
    sha = hashlib.sha256(old.cpu().numpy().tobytes()).hexdigest()
    print("knob-off sha256:", sha)
    assert sha == PARENT_SHA256
    ref = x.double() @ w.double().T + b.double() + r.double()
    assert rel(old, ref) < 2e-6 and rel(new, ref) < 2e-6
    assert rel(new, old) < 4e-6


def test_split3_order_headline_mlp1_planes_repeatable():
    """The headline's MLP1 (M = 32768, N = 2048, K0 = 512, ReLU, plane output): 1024 output tiles, four
    per workgroup, so every tile boundary but the last leaves the previous tile's plane stores in flight
    at the next tile's first wait — a size the small shapes do not reach.  Each term order returns the
    same bits on every repeat, plane 0 is the bf16 rounding of the fp32-output call's result, and the
    plane sum meets the SPLIT3 bounds against fp64."""
    M, N, K0 = 32768, 2048, 512
    x = rnd(M, K0, seed=31) * 2
    w = rnd(N, K0, scale=K0 ** -0.5, seed=32)
    b = rnd(N, seed=33)
    pl = ops.split3_rows(x)
    w6 = ops.split3_weight(w)
    ref = torch.relu(x.double() @ w.double().T + b.double())
    e_f32 = rel(ops.linear(x, w, b, torch.float32, relu=True), ref)
    for knob in (1, 0):
        with _lib.tuning(gemm_s3_order=knob):
            first = ops.linear_split3(pl, w6, b, torch.float32, relu=True, out_planes=True)
            for _ in range(3):
                assert torch.equal(first, ops.linear_split3(pl, w6, b, torch.float32, relu=True, out_planes=True))
            full = ops.linear_split3(pl, w6, b, torch.float32, relu=True)
            assert torch.equal(full, ops.linear_split3(pl, w6, b, torch.float32, relu=True))
        assert torch.equal(first[0], full.bfloat16())
        e = rel(first[0].double() + first[1].double() + first[2].double(), ref)
        print(f"gemm_s3_order={knob}: e_planes={e:.3e} e_full={rel(full, ref):.3e} e_f32={e_f32:.3e}")
        assert e < 2e-6 and e <= 2.5 * e_f32 + 1e-7, (knob, e, e_f32)
