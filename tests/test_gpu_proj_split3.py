"""The fp32 forward's two 512 x 512 out-projections as SPLIT3 GEMMs (ops.F32_SPLIT_OUTPROJ): the producers
write the A operand's bf16 planes themselves — the ViT's batch-axis attention (mhada_vit_batch_attn_split3)
and the SPLIT3 MHAda attention's epilogue (mhada_attn_split3_planes) — and the projection runs on
gemm_s3_kernel (ops.linear_split3).

Shapes are the smallest at which each form can go wrong: every L path of the batch attention (the L = 1
copy, its unaligned fall-back, 2, 5, 8), (token, head) pairs that do not fill a workgroup, several
workgroups; attention query blocks that are partial for both wave counts, a ragged last key tile and the
exact late-jump recompute; a partial and a whole number of 256-row GEMM tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import network
    from mhada_hip import _lib, engine, ops
    from mhada_hip.recipe import load_recipe, seeded_image
    DEV = "cuda"

GUARD = 4096  # bf16 elements of NaN pattern on either side of a plane buffer
PATTERN = 0x7FA5  # a bf16 NaN no kernel writes


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def guarded(n, head=GUARD):
    """A bf16 buffer of n elements inside NaN-pattern guards: (whole buffer as int16, the n-element view)."""
    buf = torch.full((head + n + GUARD,), PATTERN, dtype=torch.int16, device=DEV)
    return buf, buf[head:head + n].view(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_guards(buf, n, head=GUARD):
    assert (buf[:head] == PATTERN).all() and (buf[head + n:] == PATTERN).all()


# ---------------------------------------------------------------------------------------
# batch-axis attention planes
# ---------------------------------------------------------------------------------------
def _batch_attn_planes(qkv, L, ntok, heads, pad, head=GUARD):
    C = heads * 64
    n = L * ntok * C
    ps = n + pad
    buf, view = guarded(2 * ps + n, head)
    ops._call("mhada_vit_batch_attn_split3", qkv, qkv.data_ptr(), view.data_ptr(), ps, L, ntok, heads, 64)
    planes = torch.stack([view[p * ps:p * ps + n] for p in range(3)]).view(3, L * ntok, C)
    gaps = [bits(view[p * ps + n:(p + 1) * ps]) for p in range(2)]
    return buf, planes, gaps, 2 * ps + n


@pytest.mark.parametrize("pad", [0, 192])
@pytest.mark.parametrize("ntok,heads", [(5, 3), (33, 8)])
@pytest.mark.parametrize("L", [1, 2, 5, 8])
def test_batch_attn_planes_equal_split_of_fp32_output(L, ntok, heads, pad):
    """mhada_vit_batch_attn_split3 against split3_rows of mhada_vit_batch_attn's fp32 output, bit for bit:
    ntok * heads = 15 (not a multiple of the 4 pairs per workgroup) and 264 (66 workgroups); plane stride
    equal to and larger than rows * C, nothing written outside the three planes; repeatable."""
    C = heads * 64
    qkv = rnd(L, ntok, 3 * C, seed=7 + L)
    want = ops.split3_rows(ops.vit_batch_attn(qkv, L, ntok, heads).view(L * ntok, C))
    buf, planes, gaps, n = _batch_attn_planes(qkv, L, ntok, heads, pad)
    assert torch.equal(bits(planes), bits(want))
    assert_guards(buf, n)
    for g in gaps:
        assert (g == PATTERN).all()
    _, again, _, _ = _batch_attn_planes(qkv, L, ntok, heads, pad)
    assert torch.equal(bits(again), bits(planes))
    assert torch.equal(bits(ops.vit_batch_attn_split3(qkv, L, ntok, heads)), bits(want))


@pytest.mark.parametrize("pad,head", [(2, GUARD), (0, GUARD + 4)])
def test_batch_attn_planes_one_image_unaligned(pad, head):
    """L = 1 with a plane stride that is no multiple of 4 elements, or planes that are not 16-byte aligned:
    the per-lane kernel instead of the vector copy of V, same bits."""
    ntok, heads = 7, 3
    C = heads * 64
    qkv = rnd(1, ntok, 3 * C, seed=3)
    want = ops.split3_rows(ops.vit_batch_attn(qkv, 1, ntok, heads).view(ntok, C))
    assert torch.equal(want[0], qkv[0, :, 2 * C:].bfloat16())
    buf, planes, gaps, n = _batch_attn_planes(qkv, 1, ntok, heads, pad, head)
    assert torch.equal(bits(planes), bits(want))
    assert_guards(buf, n, head)
    for g in gaps:
        assert (g == PATTERN).all()


def test_batch_attn_planes_refused_shapes():
    """Every refused shape's error: L > 8, head widths 32 and 128, a plane stride below this call's output;
    nothing is written."""
    ntok, heads = 4, 2
    for L, hd, short in ((9, 64, 0), (2, 32, 0), (2, 128, 0), (2, 64, 1)):
        C = heads * hd
        qkv = rnd(L, ntok, 3 * C, seed=1)
        n = L * ntok * C
        buf, view = guarded(3 * n)
        with pytest.raises(ValueError):
            ops._call("mhada_vit_batch_attn_split3", qkv, qkv.data_ptr(), view.data_ptr(), n - short, L, ntok, heads, hd)
        torch.cuda.synchronize()
        assert (buf == PATTERN).all()
    with pytest.raises(ValueError):
        ops.vit_batch_attn_split3(rnd(9, ntok, 3 * 128, seed=1), 9, ntok, 2)
    with pytest.raises(ValueError):
        ops.vit_batch_attn_split3(rnd(2, ntok, 3 * 128, seed=1).bfloat16(), 2, ntok, 2)


# ---------------------------------------------------------------------------------------
# SPLIT3 MHAda attention planes
# ---------------------------------------------------------------------------------------
def _attn_planes(q, img, Ns, fcs, mu, rs, vmu):
    B, H, Nc, _ = q.shape
    n = 3 * B * Nc * H * 64
    buf, view = guarded(n)
    ops._call("mhada_attn_split3_planes", q, q.data_ptr(), img.data_ptr(), fcs.data_ptr(), mu.data_ptr(), rs.data_ptr(),
              vmu.data_ptr(), view.data_ptr(), B, H, Nc, Ns)
    return buf, view.view(3, B * Nc, H * 64), n


def _check_attn_planes(q, kv, fcs, mu, rs, vmu):
    """Both wave counts: the planes are split3_rows of mhada_attn_split3's output bit for bit (so rows >= Nc
    of a partial query block, which would land in the next batch or plane, stay unwritten), guards intact."""
    B, H, Nc, _ = q.shape
    Ns = kv.shape[2]
    img = ops.split3_kv(kv, ops.transpose_v(kv))
    saved = _lib.get_tuning("attn_waves")
    for nw in (4, 8):
        with _lib.tuning(attn_waves=nw):
            y = ops.attn_split3(q, img, Ns, fcs, mu, rs, vmu)
            buf, planes, n = _attn_planes(q, img, Ns, fcs, mu, rs, vmu)
            via_ops = ops.attn_split3_planes(q, img, Ns, fcs, mu, rs, vmu)
        assert torch.isfinite(y).all()
        want = ops.split3_rows(y.view(B * Nc, H * 64))
        assert torch.equal(bits(planes), bits(want)), nw
        assert torch.equal(bits(via_ops), bits(want)), nw
        assert_guards(buf, n)
    assert _lib.get_tuning("attn_waves") == saved  # _lib.tuning restored the knob


@pytest.mark.parametrize("Nc,Ns", [(70, 50), (33, 129), (256, 64)])
def test_attn_planes_equal_split_of_fp32_output(Nc, Ns):
    B, H = 2, 2
    q = rnd(B, H, Nc, 64, seed=31) * 0.5
    kv = rnd(B, H, Ns, 128, seed=32) * 0.5
    fcs = rnd(B, Nc, H * 64, seed=33)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, H * 64, seed=34)
    _check_attn_planes(q, kv, fcs, mu, rs, vmu)


def test_attn_planes_late_max_jump():
    """Operands of test_attn_split3_late_max_jump (a key ~120 log2 units above the first tile's scores): the
    exact recompute (attn_exact_q3) ends in the same epilogue and must write the same planes."""
    B, H, Nc, Ns = 1, 8, 97, 384
    q = rnd(B, H, Nc, 64, seed=11)
    q = q / q.norm(dim=-1, keepdim=True) * 4.0
    kv = rnd(B, H, Ns, 128, scale=0.1, seed=12)
    late = Ns - 5
    kv[:, :, late, :64] = 30.0 * q[:, :, : min(Nc, 1), :].mean(dim=2)
    kv[:, :, late - 1, :64] = -kv[:, :, late, :64]
    fcs = rnd(B, Nc, 512, seed=13)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, 512, seed=14)
    _check_attn_planes(q, kv, fcs, mu, rs, vmu)


# ---------------------------------------------------------------------------------------
# the projection from producer-written planes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [300, 512])
def test_out_projection_from_producer_planes_fp64(M):
    """N = K0 = 512 at a partial and a whole number of 256-row tiles, with and without residual: the SPLIT3
    GEMM on planes written by each producer against fp64 of the producer's fp32 output, held to the
    kernel's bounds (test_gpu_gemm_split3_order: < 2e-6 and within 2.5x the fp32 MFMA GEMM's error + 1e-7,
    the fp32 GEMM on the same operands being the path replaced)."""
    C, heads = 512, 8
    w = rnd(C, C, scale=C ** -0.5, seed=2)
    b = rnd(C, seed=3)
    r = rnd(M, C, seed=4)
    w6 = ops.split3_weight(w)
    # ViT: L = 4 images of M / 4 tokens
    L, ntok = 4, M // 4
    qkv = rnd(L, ntok, 3 * C, seed=5)
    x_vit = ops.vit_batch_attn(qkv, L, ntok, heads).view(M, C)
    p_vit = ops.vit_batch_attn_split3(qkv, L, ntok, heads)
    # MHAda: B = 2 images of M / 2 queries, 100 keys
    B, Nc, Ns = 2, M // 2, 100
    q = rnd(B, heads, Nc, 64, seed=6) * 0.5
    kv = rnd(B, heads, Ns, 128, seed=7) * 0.5
    fcs = rnd(B, Nc, C, seed=8)
    mu, rs = ops.instnorm_stats(fcs)
    vmu = rnd(B, C, seed=9)
    img = ops.split3_kv(kv, ops.transpose_v(kv))
    x_ada = ops.attn_split3(q, img, Ns, fcs, mu, rs, vmu).view(M, C)
    p_ada = ops.attn_split3_planes(q, img, Ns, fcs, mu, rs, vmu)
    for name, x, pl in (("vit", x_vit, p_vit), ("mhada", x_ada, p_ada)):
        for res in (None, r):
            ref = x.double() @ w.double().T + b.double()
            if res is not None:
                ref = ref + res.double()
            out = ops.linear_split3(pl, w6, b, torch.float32, residual=res)
            assert torch.equal(out, ops.linear_split3(pl, w6, b, torch.float32, residual=res))
            f32 = ops.linear(x, w, b, torch.float32, residual=res)
            e, e_f32 = rel(out, ref), rel(f32, ref)
            print(f"{name} M={M} res={res is not None}: e_split={e:.3e} e_f32={e_f32:.3e}")
            assert e < 2e-6, (name, e, e_f32)
            assert e <= 2.5 * e_f32 + 1e-7, (name, e, e_f32)


# ---------------------------------------------------------------------------------------
# engine routing at 64^2 B2
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    vc = load_recipe(network.VisionTransformer(pos_embedding=True), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = torch.float32
    return vc, vs, ada


def _run(nets, c, s):
    vc, vs, ada = nets
    ada.__dict__.pop("_mhada_style", None)  # no style cache carried over from another run
    with torch.no_grad():
        fcs, cs = ada(vc(c), vs(s))
    return fcs.clone(), cs.clone()


def _record(monkeypatch):
    """Recording wrappers: (fp32 mhada_gemm calls as (M, N, K), linear_split3 calls as (M, N, K0))."""
    f32, s3 = [], []
    gemm0, ls0 = ops.gemm, ops.linear_split3

    def gemm(**kw):
        if kw["compute"] == torch.float32 and kw.get("a_mode", ops.A_ROWS) != ops.A_SPLIT3 and kw.get("nb", (1, 1)) == (1, 1):
            f32.append((kw["M"], kw["N"], kw["K"]))
        return gemm0(**kw)

    def linear_split3(planes, w6, *a, **kw):
        s3.append((planes.shape[1], w6.shape[0], planes.shape[2]))
        return ls0(planes, w6, *a, **kw)

    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "linear_split3", linear_split3)
    return f32, s3


def test_engine_routes_both_out_projections_to_split3(nets, monkeypatch):
    B, res = 2, 64
    c = seeded_image(B, res, res, 1).to(DEV)
    s = seeded_image(B, res, res, 2).to(DEV)
    M = B * (res // 8) ** 2
    proj = (M, 512, 512)
    vit_layers = len(nets[0].encoder) + len(nets[1].encoder)
    blocks = len(nets[2].adaAttnHead)
    monkeypatch.setattr(engine, "_split3_fills", lambda M, N, dev: True)
    assert ops.F32_SPLIT_OUTPROJ is True
    f32, s3 = _record(monkeypatch)
    on = _run(nets, c, s)
    assert proj not in f32
    assert s3.count(proj) == vit_layers + blocks
    # the switch off: today's routing, the projections back on the fp32 GEMM
    f32.clear(), s3.clear()
    monkeypatch.setattr(ops, "F32_SPLIT_OUTPROJ", False)
    off = _run(nets, c, s)
    assert f32.count(proj) == vit_layers + blocks and proj not in s3
    # today's routing spelled out: the fp32 attention outputs through ops.linear / ops.gemm
    monkeypatch.setattr(ops, "vit_batch_attn_split3", None)
    monkeypatch.setattr(ops, "attn_split3_planes", None)
    ref = _run(nets, c, s)
    for a, b in zip(off, ref):
        assert torch.equal(a, b)
    # both forms are fp32-accurate: they differ by rounding only
    assert rel(on[1], off[1]) < 1e-5 and rel(on[0], off[0]) < 1e-5


def test_engine_cached_style_equals_uncached(nets, monkeypatch):
    """The cached-style (video) call takes the same routing: bit-equal to the uncached call."""
    B, res = 2, 64
    vc, vs, ada = nets
    c = seeded_image(B, res, res, 3).to(DEV)
    s = seeded_image(B, res, res, 4).to(DEV)
    monkeypatch.setattr(engine, "_split3_fills", lambda M, N, dev: True)
    f32, s3 = _record(monkeypatch)
    ada.__dict__.pop("_mhada_style", None)
    with torch.no_grad():
        fc, fs = vc(c), vs(s)
        s3.clear()  # the ViTs' own SPLIT3 GEMMs
        first = [t.clone() for t in ada(fc, fs)]
        assert engine.style_cache(ada, fs[:ada.num_layers], torch.float32)[1]  # the next call hits
        n_first = s3.count((B * 64, 512, 512))
        s3.clear()
        second = [t.clone() for t in ada(fc, fs)]  # the same fs objects: the style cache hits
    assert "img" in ada.__dict__["_mhada_style"]["sides"][0]
    assert s3.count((B * 64, 512, 512)) == n_first == len(ada.adaAttnHead)
    assert (B * 64, 512, 512) not in f32
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    ada.__dict__.pop("_mhada_style", None)
