"""CPU checks of the SPLIT3 out-projection: the three-plane split the producers write, the split weight
reproducing an fp64 512 x 512 projection, and the routing predicate."""
import torch

from mhada_hip import engine, ops


def split3(x):
    """The round-to-nearest three-plane split (mhada_split3_rows and the plane epilogues)."""
    p0 = x.bfloat16()
    r = x - p0.float()
    p1 = r.bfloat16()
    p2 = (r - p1.float()).bfloat16()
    return p0, p1, p2


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_three_plane_split_is_exact_to_2pow25():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    p0, p1, p2 = split3(x)
    assert torch.equal(p0, x.bfloat16())
    assert torch.equal(p1, (x - p0.float()).bfloat16())
    s = p0.double() + p1.double() + p2.double()
    # 8 + 8 + 8 mantissa bits and three signs: the sum is x to 2^-25 relative (most values exactly)
    assert ((s - x.double()).abs() <= x.double().abs() * 2.0 ** -25).all()
    # x - p0 and (x - p0) - p1 are exact in fp32 (Sterbenz-like: a residual of a rounding fits)
    assert torch.equal((x - p0.float()).double(), x.double() - p0.double())


def test_split3_weight_reproduces_fp64_projection():
    """The six kept cross products of the plane operands, summed in fp64, against the fp64 projection: the
    dropped terms (i + j > 2) stay under the SPLIT3 GEMM's bound (< 2e-6, and within 2.5x an fp32
    matmul's error + 1e-7 on the same operands)."""
    g = torch.Generator().manual_seed(1)
    M, C = 300, 512
    x = torch.randn(M, C, generator=g) * 2
    w = torch.randn(C, C, generator=g) * C ** -0.5
    w6 = ops.split3_weight(w)
    assert w6.shape == (C, 6 * C) and w6.dtype == torch.bfloat16
    q = split3(w)
    blocks = w6.view(C, C // 64, 6, 64)
    for t, j in enumerate((1, 0, 2, 0, 1, 0)):
        assert torch.equal(blocks[:, :, t].reshape(C, C), q[j])
    p = split3(x)
    # one A plane per W term q1 q0 q2 q0 q1 q0 of a 64-column chunk, so that the six pairs are those with i + j <= 2
    a_of_t = (1, 2, 0, 1, 0, 0)
    out = torch.zeros(M, C, dtype=torch.float64)
    for t in range(6):
        out += p[a_of_t[t]].double() @ blocks[:, :, t].reshape(C, C).double().T
    ref = x.double() @ w.double().T
    e, e_f32 = rel(out, ref), rel(x @ w.T, ref)
    print(f"e_split={e:.3e} e_f32={e_f32:.3e}")
    assert e < 2e-6 and e <= 2.5 * e_f32 + 1e-7


def test_routing_predicate(monkeypatch):
    """_split3_fills on a 256-CU device: the 512^2 B8 projection (32768 x 512: 256 tiles) fills it, B = 1 at
    512^2 (4096 x 512: 32 tiles) does not; ops.F32_SPLIT off disables it."""
    dev = torch.device("cuda", 0)
    monkeypatch.setitem(engine._NUM_CUS, 0, 256)
    assert ops.F32_SPLIT_OUTPROJ is True
    assert engine._split3_fills(32768, 512, dev)
    assert not engine._split3_fills(4096, 512, dev)
    assert engine._split3_fills(135 * 240, 512, dev)  # the 1080p frame, B = 1
    monkeypatch.setattr(ops, "F32_SPLIT", False)
    assert not engine._split3_fills(32768, 512, dev)
