"""Training at head widths 32 and 128 (16- and 4-head models): the D = 32 | 128 kernels of
csrc/attn_train.hip through MHAdaAttnFn, the grouped head projection at d = 32 | 128, the fused block and one Trainer step.

Bounds are those of test_gpu_train_attn.py (its docstring): fp32 MFMA against fp64, outputs
< max(2e-4, 2 err32) and gradients < max(2e-4, 4 err32) of the tensor's max magnitude, err32 the
reference formula's own fp32 autograd on the device with A materialised.  The scales keep the logit
std (scale^2 sqrt(D)) at or below 8; above 12 every fp32 form scatters around the yardstick by seed
(tools/train_attn_hd_ab.py --errsweep, profiles/r11_train_attn_hd_err.log)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from mhada_hip import _lib, autograd_path, ops, train_fns
from mhada_hip.recipe import load_recipe
from mhada_hip.train import Trainer
from test_train_heads_cpu import build_heads, check_against_golden_heads

WIDTHS = (32, 128)
NAN32 = 0x7FC12345  # guard bit pattern (a quiet NaN), as test_gpu_gemm_forms.py


def _ref(q, k, v, x):
    """adaDecoder.py:186-198 on centred v (v passed already centred)."""
    a = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    m = a @ v
    e2 = a @ (v * v)
    s = torch.sqrt((e2 - m * m).clamp(min=1e-6))
    return s * x + m


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def _inputs(BH, Nc, Ns, D, scale, seed, vscale=3.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(BH, Nc, D, generator=g) * scale
    k = torch.randn(BH, Ns, D, generator=g) * scale
    v = torch.randn(BH, Ns, D, generator=g) * vscale
    v = v - v.mean(dim=1, keepdim=True)
    x = torch.randn(BH, Nc, D, generator=g)
    dout = torch.randn(BH, Nc, D, generator=g)
    return q, k, v, x, dout


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("BH,Nc,Ns,scale", [(2, 128, 64, 0.4), (3, 100, 70, 0.4), (1, 37, 300, 0.5),
                                            (2, 33, 4, 0.5), (2, 200, 160, 0.7)])
def test_attn_train_hd_fwd_bwd_vs_fp64(D, BH, Nc, Ns, scale):
    """Forward + backward through MHAdaAttnFn: full and ragged query / key tiles, Ns below one tile,
    several workgroups per (b, h) (Nc = 200, Ns = 160)."""
    q, k, v, x, dout = _inputs(BH, Nc, Ns, D, scale, seed=Nc * 7 + Ns + D)
    ts = [t.double().requires_grad_() for t in (q, k, v, x)]
    ref = _ref(*ts)
    ref.backward(dout.double())
    gs = [t.cuda().contiguous().requires_grad_() for t in (q, k, v, x)]
    out = autograd_path.MHAdaAttnFn.apply(*gs)
    out.backward(dout.cuda())
    # yardstick: the reference's own fp32 autograd (materialised A) on the same device
    fs = [t.cuda().contiguous().requires_grad_() for t in (q, k, v, x)]
    out32 = _ref(*fs)
    out32.backward(dout.cuda())
    torch.cuda.synchronize()
    err, err32 = _rel(out.double().cpu(), ref.detach()), _rel(out32.double().cpu(), ref.detach())
    print(f"out: err {err:.3e} err32 {err32:.3e}")
    assert err < max(2e-4, 2 * err32)
    for name, a, b, c in zip("qkvx", gs, ts, fs):
        err = _rel(a.grad.double().cpu(), b.grad)
        err32 = _rel(c.grad.double().cpu(), b.grad)
        print(f"d{name}: err {err:.3e} err32 {err32:.3e}")
        assert err < max(2e-4, 4 * err32), (name, err, err32)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("BH,Nc,Ns,scale", [(2, 300, 700, 0.5), (3, 97, 33, 1.0)])
def test_attn_train_hd_fwd_outputs_vs_fp64(D, BH, Nc, Ns, scale):
    """lse2 and the [M' | E2'] halves of ops.attn_train_fwd_hd against fp64, to the bounds of
    test_attn_train_fwd_kernels_vs_fp64."""
    q, k, v, x, _ = _inputs(BH, Nc, Ns, D, scale, seed=BH * 100 + Ns + D, vscale=2.0)
    out, mo, lse = ops.attn_train_fwd_hd(*(t.cuda().contiguous() for t in (q, k, v, x)))
    assert mo.shape == (BH, Nc, 2 * D) and lse.shape == (BH, Nc)
    qd, kd, vd = q.double(), k.double(), v.double()
    s = qd @ kd.transpose(1, 2)
    a = torch.softmax(s, -1)
    assert torch.allclose(lse.double().cpu(), torch.logsumexp(s, -1) / math.log(2.0), atol=2e-4, rtol=1e-5)
    a32 = torch.softmax(q @ k.transpose(1, 2), -1)
    for sl, ref64, ref32 in ((slice(0, D), a @ vd, a32 @ v), (slice(D, 2 * D), a @ vd ** 2, a32 @ (v * v))):
        err, err32 = _rel(mo[..., sl].double().cpu(), ref64), _rel(ref32.double(), ref64)
        print(f"mo[{sl.start}:{sl.stop}]: err {err:.3e} err32 {err32:.3e}")
        assert err < max(2e-5, 2 * err32)
    ref = _ref(qd, kd, vd, x.double())
    assert _rel(out.double().cpu(), ref) < max(2e-4, 4 * _rel(_ref(q, k, v, x).double(), ref))


@pytest.mark.parametrize("D", WIDTHS)
def test_attn_train_hd_bwd_with_clamped_variance(D):
    """Channels whose attention-weighted variance is below the 1e-6 clamp (constant V' there): the
    clamp's gradient is zero in those channels (mhada_attn_train_bwd_prep_hd), as in fp64 autograd."""
    BH, Nc, Ns = 2, 128, 96
    q, k, v, x, dout = _inputs(BH, Nc, Ns, D, 0.4, seed=5 + D)
    v[:, :, :5] = 0.0  # var = 0 < 1e-6: the clamp is active in channels 0-4
    ts = [t.double().requires_grad_() for t in (q, k, v, x)]
    _ref(*ts).backward(dout.double())
    gs = [t.cuda().contiguous().requires_grad_() for t in (q, k, v, x)]
    autograd_path.MHAdaAttnFn.apply(*gs).backward(dout.cuda())
    for name, a, b in zip("qkvx", gs, ts):
        assert _rel(a.grad.double().cpu(), b.grad) < 2e-4, name


class Guarded:
    """[BH][rows][cols] slices inside one flat NaN-pattern buffer with one guard row before the first
    slice and after every slice (the padding scheme of test_gpu_gemm_forms.py, GUARD = 1): slice(i) is
    the dense [rows][cols] payload of (b, h) = i."""

    def __init__(self, BH, rows, cols):
        self.BH, self.rows, self.cols = BH, rows, cols
        self.flat = torch.full(((BH * (rows + 1) + 1) * cols,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)

    def slice(self, i):
        o = (1 + i * (self.rows + 1)) * self.cols
        return self.flat[o:o + self.rows * self.cols].view(self.rows, self.cols)

    def check(self):
        iv = self.flat.view(torch.int32).view(-1, self.cols)
        guard = torch.zeros(iv.shape[0], dtype=torch.bool, device="cuda")
        guard[0] = True
        guard[self.rows + 1::self.rows + 1] = True
        assert int(guard.sum()) == self.BH + 1
        assert bool((iv[guard] == NAN32).all()), "a guard row was written"
        assert bool(torch.isfinite(self.flat.view(-1, self.cols)[~guard]).all()), "a payload element was not written"


@pytest.mark.parametrize("D", WIDTHS)
def test_attn_train_hd_leaves_guard_rows_intact(D):
    """Nc = 37 (a ragged 32-query tile), Ns = 5 (below one key tile): every output of the three entries
    sits between NaN-pattern guard rows at each (b, h) boundary — the entries are called per slice on
    pointers into the guarded buffers — which must hold their pattern while every payload element is
    written."""
    BH, Nc, Ns = 3, 37, 5
    q, k, v, x, dout = (t.cuda().contiguous() for t in _inputs(BH, Nc, Ns, D, 0.5, seed=37 + D))
    out, mo, lse = Guarded(BH, Nc, D), Guarded(BH, Nc, 2 * D), Guarded(BH, Nc, 1)
    dx, dmo, dd = Guarded(BH, Nc, D), Guarded(BH, Nc, 2 * D), Guarded(BH, Nc, 1)
    dq, dk, dv = Guarded(BH, Nc, D), Guarded(BH, Ns, D), Guarded(BH, Ns, D)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for i in range(BH):
        p = lambda t: t.data_ptr()  # noqa: E731
        rc = lib.mhada_attn_train_fwd_hd(p(q[i]), p(k[i]), p(v[i]), p(x[i]), p(out.slice(i)), p(mo.slice(i)),
                                         p(lse.slice(i)), 1, D, Nc, Ns, st)
        assert rc == 0, lib.mhada_last_error()
        rc = lib.mhada_attn_train_bwd_prep_hd(p(dout[i]), p(x[i]), p(mo.slice(i)), p(dx.slice(i)), p(dmo.slice(i)),
                                              p(dd.slice(i)), Nc, D, st)
        assert rc == 0, lib.mhada_last_error()
        rc = lib.mhada_attn_train_bwd_hd(p(q[i]), p(k[i]), p(v[i]), p(lse.slice(i)), p(dmo.slice(i)), p(dd.slice(i)),
                                         p(dq.slice(i)), p(dk.slice(i)), p(dv.slice(i)), 1, D, Nc, Ns, st)
        assert rc == 0, lib.mhada_last_error()
    torch.cuda.synchronize()
    for t in (out, mo, lse, dx, dmo, dd, dq, dk, dv):
        t.check()
    # the per-slice calls return what the batched ops return
    o2, mo2, lse2 = ops.attn_train_fwd_hd(q, k, v, x)
    dx2, dmo2, dd2 = ops.attn_train_bwd_prep_hd(dout, x, mo2)
    dq2, dk2, dv2 = ops.attn_train_bwd_hd(q, k, v, lse2, dmo2, dd2)
    for i in range(BH):
        for a, b in ((out, o2), (mo, mo2), (dx, dx2), (dmo, dmo2), (dq, dq2), (dk, dk2), (dv, dv2)):
            assert torch.equal(a.slice(i), b[i])
        assert torch.equal(lse.slice(i).view(-1), lse2[i]) and torch.equal(dd.slice(i).view(-1), dd2[i])


@pytest.mark.parametrize("D", WIDTHS)
def test_attn_train_hd_bwd_is_deterministic(D):
    """No atomics: two backward calls return equal bits, and BWD_PATH_COUNTS (the 64-wide spill /
    recompute record) is not touched."""
    BH, Nc, Ns = 2, 200, 160
    q, k, v, x, _ = (t.cuda().contiguous() for t in _inputs(BH, Nc, Ns, D, 0.5, seed=9 + D))
    out, mo, lse = ops.attn_train_fwd_hd(q, k, v, x)
    dmo = torch.randn(BH, Nc, 2 * D, generator=torch.Generator().manual_seed(3)).cuda()
    dd = (dmo * mo).sum(-1).contiguous()
    before = dict(ops.BWD_PATH_COUNTS)
    a = ops.attn_train_bwd_hd(q, k, v, lse, dmo, dd)
    b = ops.attn_train_bwd_hd(q, k, v, lse, dmo, dd)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert ops.BWD_PATH_COUNTS == before


def _count_fwd_hd_calls(monkeypatch):
    """Wrap ops.attn_train_fwd_hd: the returned list receives the row width of every call."""
    calls, real = [], ops.attn_train_fwd_hd

    def counted(q, k, v, x):
        calls.append(q.shape[-1])
        return real(q, k, v, x)

    monkeypatch.setattr(ops, "attn_train_fwd_hd", counted)
    return calls


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


@pytest.mark.parametrize("H,d", [(16, 32), (4, 128)])
def test_head_proj_grouped_gemm_hd_vs_fp64(H, d):
    """train_fns.HeadProjFn at d = 32 | 128 against fp64 autograd of the per-head products, to the
    tolerance test_head_proj_grouped_gemm_vs_fp64 applies at 64: y, dX, dW, db."""
    T = 70
    x, w, b, gy = _rnd(T, d * H, seed=11), _rnd(H, d, d, scale=0.125, seed=12), _rnd(H, d, seed=13), _rnd(H, T, d, seed=14)
    xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
    y = train_fns.head_proj(xs, ws, bs)
    y.backward(gy)
    xd, wd, bd = (t.double().clone().requires_grad_() for t in (x, w, b))
    yd = torch.stack([xd[:, d * h:d * h + d] @ wd[h].T + bd[h] for h in range(H)])
    yd.backward(gy.double())
    assert _rel(y.double(), yd) < 2e-6
    for a, r in ((xs.grad, xd.grad), (ws.grad, wd.grad), (bs.grad, bd.grad)):
        assert _rel(a.double(), r) < 2e-6


def test_head_proj_at_64_is_the_same_gemm_call():
    """d = 64: HeadProjFn's forward equals, in bits, a direct ops.gemm call with the arguments it has
    always passed (strides 64 and 4096)."""
    T, H = 70, 8
    x, w, b = _rnd(T, 64 * H, seed=11), _rnd(H, 64, 64, scale=0.125, seed=12), _rnd(H, 64, seed=13)
    y = train_fns.head_proj(x, w, b)
    ref = torch.empty(H, T, 64, device="cuda")
    ops.gemm(a=x, w=w, c=ref, M=T, N=64, K=64, compute=torch.float32, lda=64 * H, sa=(64, 0), nb=(H, 1), ldw=64,
             sw=(4096, 0), bias=b, sb=(64, 0), ldc=64, sc=(T * 64, 0))
    assert torch.equal(y, ref)


@pytest.mark.parametrize("heads", [4, 16])
def test_fused_block_grads_match_autograd_block_heads(monkeypatch, heads):
    """autograd_path.block_forward with TRAIN_ATTN "hip" (the fused block on the D-wide kernels) against
    "torch" (the per-head aten loop) on a 4- and a 16-head block, to the tolerance of
    test_fused_block_grads_match_autograd_block; "hip" must reach ops.attn_train_fwd_hd."""
    calls = _count_fwd_hd_calls(monkeypatch)
    torch.manual_seed(0)
    blk = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads), "ada").cuda().adaAttnHead[0]
    fc = (torch.randn(2, 512, 12, 10, device="cuda") * 2).requires_grad_()
    fs = (torch.randn(2, 512, 9, 11, device="cuda") * 2).requires_grad_()
    fcs = (torch.randn(2, 512, 12, 10, device="cuda") * 2).requires_grad_()
    dout = torch.randn(2, 512, 12, 10, device="cuda")
    results = []
    for mode in ("hip", "torch"):
        monkeypatch.setattr(autograd_path, "TRAIN_ATTN", mode)
        for t in (fc, fs, fcs, *blk.parameters()):
            t.grad = None
        y = autograd_path.block_forward(blk, fc, fs, fcs)
        y.backward(dout)
        results.append([y.detach().clone()] + [t.grad.clone() for t in (fc, fs, fcs, *blk.parameters())])
        assert calls == [512 // heads]  # one call, by "hip" only
    # K-bias gradients are zero in exact arithmetic (a per-query constant logit shift): those
    # are held to an absolute floor of 1e-5 of the largest gradient
    gmax = max(b.abs().max().item() for b in results[1])
    for i, (a, b) in enumerate(zip(*results)):
        err = (a.double() - b.double()).abs().max().item()
        assert err <= max(1e-3 * b.abs().max().item(), 1e-5 * gmax), (i, err)


def test_attn_train_hd_never_stores_the_attention_matrix():
    """The feature's point: forward + backward at BH = 16, D = 32, Nc = Ns = 4096 allocate less than ONE
    Nc x Ns fp32 matrix per (b, h) (4 BH Nc Ns = 1 GiB) above what was live before the call; the op's own
    tensors are about 15 x 8 MiB.  The aten path keeps A and its gradients: several GiB."""
    BH, D, N = 16, 32, 4096
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, x = (torch.randn(BH, N, D, device="cuda", generator=g) * 0.5 for _ in range(4))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_(), x.requires_grad_()
    dout = torch.randn(BH, N, D, device="cuda", generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    autograd_path.MHAdaAttnFn.apply(q, k, v, x).backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak / 2 ** 20:.1f} MiB")
    assert peak < 4 * BH * N * N
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v, x))


@pytest.mark.parametrize("heads", [4, 16])
def test_gpu_train_step_matches_reference_golden_heads(monkeypatch, heads):
    """One Trainer.backward step of a 4- / 16-head model against the reference's golden, with every
    MHAda attention of the step (six blocks, the three AdaFormer calls batched into one) on the
    D-wide kernels."""
    calls = _count_fwd_hd_calls(monkeypatch)
    tr = Trainer(*build_heads(heads, "cuda"))
    check_against_golden_heads(tr, "cuda", heads)
    n_blocks = len(tr.ada.adaAttnHead)
    assert calls and set(calls) == {512 // heads} and len(calls) % n_blocks == 0
