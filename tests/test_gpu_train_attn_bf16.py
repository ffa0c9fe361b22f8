"""The opt-in bf16 training attention (csrc/attn_train_bf16.hip, autograd_path.MHAdaAttnBf16Fn,
Trainer(attn_precision="bf16")) against fp64 autograd of the reference formula.

Yardstick: what the reference's own code yields under torch.autocast(bfloat16), restated in
``_yard`` and evaluated in the test on the same inputs: q, k, v cast to bf16, bmm in bf16, softmax on
the float of that, A cast to bf16 for A v and A v^2 (v^2 squared in fp32, then cast), the rest in
fp32, gradients by autograd through it.  Error = max|delta| / max|ref| per tensor; every assertion
is error <= 2 x the yardstick's error on that tensor.

Measured on an MI355X (worst error / yardstick ratio per tensor over the nine cases of (a)): out' 0.62,
dq 0.68, dk 0.91, dv 0.60, dx 0.83; the block of (f) 1.45 at worst.  With bf16(V'^2) beside bf16(V') and
single-plane dM', dE2' in dV', dv was 2.4 - 16.6 x the yardstick at logit std 8: the
kernels take the exact hi + lo planes of (bf16 V')^2 and hi + lo dM', dE2' in dV' for that reason."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import network
from conftest import load_golden
from mhada_hip import _lib, autograd_path, ops
from mhada_hip.recipe import load_recipe, seeded_image
from mhada_hip.train import Trainer
from test_train_cpu import build

NAN32 = 0x7FC12345  # guard bit pattern (a quiet NaN)
LOG2E = 1.4426950408889634


def _ref(q, k, v, x):
    """adaDecoder.py:186-198 on centred v (v passed already centred)."""
    a = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    m = a @ v
    e2 = a @ (v * v)
    s = torch.sqrt((e2 - m * m).clamp(min=1e-6))
    return s * x + m


def _yard(q, k, v, x):
    """_ref as torch.autocast(bfloat16) evaluates it."""
    s = torch.bmm(q.bfloat16(), k.bfloat16().transpose(1, 2))
    a = torch.softmax(s.float(), dim=-1).bfloat16()
    m = torch.bmm(a, v.bfloat16()).float()
    e2 = torch.bmm(a, (v * v).bfloat16()).float()
    return torch.sqrt((e2 - m * m).clamp(min=1e-6)) * x.float() + m


class _YardFn:
    """Stands in for autograd_path.MHAdaAttnFn: the yardstick through plain autograd."""
    apply = staticmethod(_yard)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def _inputs(BH, Nc, Ns, scale, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(BH, Nc, 64, generator=g) * scale
    k = torch.randn(BH, Ns, 64, generator=g) * scale
    v = torch.randn(BH, Ns, 64, generator=g) * 3
    v = v - v.mean(dim=1, keepdim=True)
    x = torch.randn(BH, Nc, 64, generator=g)
    dout = torch.randn(BH, Nc, 64, generator=g)
    return q, k, v, x, dout


def _three_ways(q, k, v, x, dout):
    """[out, dq, dk, dv, dx] of fp64 autograd, of MHAdaAttnBf16Fn and of the yardstick (fp64, on the CPU)."""
    ts = [t.double().requires_grad_() for t in (q, k, v, x)]
    ref = _ref(*ts)
    ref.backward(dout.double())
    res = [[ref.detach()] + [t.grad for t in ts]]
    for fn in (autograd_path.MHAdaAttnBf16Fn.apply, _yard):
        gs = [t.cuda().contiguous().requires_grad_() for t in (q, k, v, x)]
        out = fn(*gs)
        out.backward(dout.cuda())
        res.append([out.detach().double().cpu()] + [t.grad.double().cpu() for t in gs])
    return res


def _assert_within_twice_the_yardstick(ref, got, yard, label):
    bad = []
    for name, r, a, y in zip(("out", "dq", "dk", "dv", "dx"), ref, got, yard):
        err, erry = _rel(a, r), _rel(y, r)
        print(f"{label} {name}: err {err:.3e} yardstick {erry:.3e} ratio {err / erry:.2f}")
        assert np.isfinite(erry) and erry > 0  # the bound is never vacuous
        if not err <= 2 * erry:
            bad.append((name, err, erry))
    assert not bad, bad


@pytest.mark.parametrize("BH,Nc,Ns,scale", [(2, 128, 64, 0.4), (3, 100, 70, 0.4), (1, 37, 300, 0.6), (2, 33, 4, 0.5),
                                            (2, 256, 129, 1.0)])
def test_attn_train_bf16_fwd_bwd_vs_fp64(BH, Nc, Ns, scale):
    """(a) A ragged query tail, a ragged key tail, fewer keys than one tile, more than one key tile per
    block and more than one workgroup per (b, h); logit std 8 scale^2 <= 8."""
    ref, got, yard = _three_ways(*_inputs(BH, Nc, Ns, scale, seed=Nc * 7 + Ns))
    _assert_within_twice_the_yardstick(ref, got, yard, f"({BH},{Nc},{Ns},{scale})")


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_attn_train_bf16_fwd_bwd_vs_fp64_seeds(seed):
    """(a) (2, 200, 160) at logit std 8 over four seeds."""
    ref, got, yard = _three_ways(*_inputs(2, 200, 160, 1.0, seed=seed))
    _assert_within_twice_the_yardstick(ref, got, yard, f"seed {seed}")


class Guarded:
    """[rows][cols] inside a NaN-pattern buffer with one guard row before and after."""

    def __init__(self, rows, cols):
        self.rows, self.cols = rows, cols
        self.flat = torch.full(((rows + 2) * cols,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.flat[cols:(rows + 1) * cols].view(rows, cols)

    def check(self):
        iv = self.flat.view(torch.int32).view(-1, self.cols)
        assert bool((iv[0] == NAN32).all()) and bool((iv[-1] == NAN32).all()), "a guard row was written"
        assert bool(torch.isfinite(self.t).all()), "a payload element was not written"


@pytest.mark.parametrize("Nc,Ns", [(37, 300), (33, 4)])
def test_attn_train_bf16_leaves_guard_rows_intact(Nc, Ns):
    """(b) out, mo, lse, dq, dk, dv of every (b, h) sit between poisoned rows (the entries are called
    per slice on pointers into the guarded buffers) and equal what the batched ops return."""
    BH = 2
    q, k, v, x, dout = (t.cuda().contiguous() for t in _inputs(BH, Nc, Ns, 0.5, seed=Nc + Ns))
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    o2, mo2, lse2 = ops.attn_train_fwd_bf16(q, k, v, x)
    dx2, dmo2, _ = ops.attn_train_bwd_prep(dout, x, mo2)
    dq2, dk2, dv2 = ops.attn_train_bwd_bf16(q, k, v, lse2, dmo2, mo2)
    p = lambda t: t.data_ptr()  # noqa: E731
    for i in range(BH):
        out, mo, lse = Guarded(Nc, 64), Guarded(Nc, 128), Guarded(Nc, 1)
        dq, dk, dv = Guarded(Nc, 64), Guarded(Ns, 64), Guarded(Ns, 64)
        ws = torch.empty(max(lib.mhada_attn_train_bf16_workspace(1, Nc, Ns, b) for b in (0, 1)), dtype=torch.uint8,
                         device="cuda")
        rc = lib.mhada_attn_train_fwd_bf16(p(q[i]), p(k[i]), p(v[i]), p(x[i]), p(out.t), p(mo.t), p(lse.t), p(ws),
                                           ws.numel(), 1, Nc, Ns, st)
        assert rc == 0, lib.mhada_last_error()
        rc = lib.mhada_attn_train_bwd_bf16(p(q[i]), p(k[i]), p(v[i]), p(lse.t), p(dmo2[i]), p(mo.t), p(dq.t), p(dk.t),
                                           p(dv.t), p(ws), ws.numel(), 1, Nc, Ns, 3, st)
        assert rc == 0, lib.mhada_last_error()
        torch.cuda.synchronize()
        for t in (out, mo, lse, dq, dk, dv):
            t.check()
        for a, b in ((out, o2), (mo, mo2), (dq, dq2), (dk, dk2), (dv, dv2)):
            assert torch.equal(a.t, b[i])
        assert torch.equal(lse.t.view(-1), lse2[i])


def test_attn_train_bf16_bwd_with_clamped_variance():
    """(c) v[:, :, :5] = 0: the clamp is active in channels 0-4; gradients there are fp64's exact zeros
    where fp64 has them, the rest within bound (a)."""
    q, k, v, x, dout = _inputs(2, 128, 96, 0.4, seed=5)
    v[:, :, :5] = 0.0
    ref, got, yard = _three_ways(q, k, v, x, dout)
    for r, a in zip(ref[1:], got[1:]):
        zero = r == 0
        assert bool((a[zero] == 0).all())
    _assert_within_twice_the_yardstick(ref, got, yard, "clamped")


def test_attn_train_bf16_is_deterministic():
    """(d) No atomics: two forward + backward calls on the same inputs return the same bits."""
    q, k, v, x, dout = (t.cuda().contiguous() for t in _inputs(2, 200, 160, 0.5, seed=9))
    res = []
    for _ in range(2):
        before = dict(ops.BF16_TRAIN_COUNTS)
        out, mo, lse = ops.attn_train_fwd_bf16(q, k, v, x)
        dx, dmo, _ = ops.attn_train_bwd_prep(dout, x, mo)
        dq, dk, dv = ops.attn_train_bwd_bf16(q, k, v, lse, dmo, mo)
        assert ops.BF16_TRAIN_COUNTS == {"fwd": before["fwd"] + 1, "bwd": before["bwd"] + 1}
        res.append((out, mo, lse, dq, dk, dv, dx))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_attn_train_bf16_recomputed_rows_sum_to_one():
    """(e) From the forward's lse2 and the test's own restatement of the logits (bf16 q, k; fp32 products
    and sum; times log2 e), sum_j exp2(S_ij - lse2_i) is within 1e-3 of 1 in every row."""
    q, k, v, x, _ = (t.cuda().contiguous() for t in _inputs(2, 128, 64, 0.4, seed=128 * 7 + 64))
    _, _, lse = ops.attn_train_fwd_bf16(q, k, v, x)
    s2 = (q.bfloat16().double() @ k.bfloat16().double().transpose(1, 2)) * LOG2E
    rows = torch.exp2(s2 - lse.double().unsqueeze(-1)).sum(-1)
    print(f"row sums: {rows.min().item():.6f} .. {rows.max().item():.6f}")
    assert bool(((rows - 1).abs() < 1e-3).all())


def _block_run(blk, fc, fs, fcs, dout):
    for t in (fc, fs, fcs, *blk.parameters()):
        t.grad = None
    y = autograd_path.block_forward(blk, fc, fs, fcs)
    y.backward(dout)
    return [y.detach().double().cpu()] + [t.grad.double().cpu() for t in (fc, fs, fcs, *blk.parameters())]


def _block_inputs(dtype=torch.float32, device="cuda"):
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: (torch.randn(*s, generator=g) * 2).to(device=device, dtype=dtype).requires_grad_()  # noqa: E731
    fc, fs, fcs = mk(2, 512, 4, 4), mk(2, 512, 3, 5), mk(2, 512, 4, 4)
    dout = torch.randn(2, 512, 4, 4, generator=g).to(device=device, dtype=dtype)
    return fc, fs, fcs, dout


def test_block_bf16_within_twice_the_yardstick(monkeypatch):
    """(f) block_forward on one 8-head block (B = 2, 4x4 content, 3x5 style) with TRAIN_ATTN "bf16": the
    counter rises; output and every gradient within 2x the yardstick block's error against the fp64
    aten block (the yardstick block: MHAdaAttnFn replaced by the autocast restatement under "hip")."""
    torch.manual_seed(0)
    blk = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").cuda().adaAttnHead[0]
    blk64 = load_recipe(network.AdaAttnTransformerMultiHead(), "ada").adaAttnHead[0].double()
    ref = _block_run(blk64, *_block_inputs(torch.float64, "cpu"))
    args = _block_inputs()
    before = dict(ops.BF16_TRAIN_COUNTS)
    monkeypatch.setattr(autograd_path, "TRAIN_ATTN", "bf16")
    got = _block_run(blk, *args)
    assert ops.BF16_TRAIN_COUNTS == {"fwd": before["fwd"] + 1, "bwd": before["bwd"] + 1}
    monkeypatch.setattr(autograd_path, "TRAIN_ATTN", "hip")
    monkeypatch.setattr(autograd_path, "MHAdaAttnFn", _YardFn)
    yard = _block_run(blk, *args)
    assert ops.BF16_TRAIN_COUNTS == {"fwd": before["fwd"] + 1, "bwd": before["bwd"] + 1}
    bad = []
    for i, (r, a, y) in enumerate(zip(ref, got, yard)):
        # max|delta| of both sides: the ratio does not depend on the common scale max|ref|
        err, erry = (a - r).abs().max().item(), (y - r).abs().max().item()
        print(f"block tensor {i}: err {err:.3e} yardstick {erry:.3e}")
        if not err <= 2 * erry:
            bad.append((i, err, erry))
    assert not bad, bad


def test_block_bf16_mode_leaves_16_heads_on_the_fp32_kernels(monkeypatch):
    """(f) A 16-head block (head width 32) under TRAIN_ATTN "bf16" runs the _hd fp32 kernels."""
    calls, real = [], ops.attn_train_fwd_hd
    monkeypatch.setattr(ops, "attn_train_fwd_hd", lambda *a: (calls.append(a[0].shape[-1]), real(*a))[1])
    blk = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=16), "ada").cuda().adaAttnHead[0]
    before = dict(ops.BF16_TRAIN_COUNTS)
    monkeypatch.setattr(autograd_path, "TRAIN_ATTN", "bf16")
    _block_run(blk, *_block_inputs())
    assert calls == [32] and ops.BF16_TRAIN_COUNTS == before


def _trainer_run(tr, c, s):
    out = tr.backward(c, s)
    losses = np.array([float(out[k].detach()) for k in ("loss_gs", "loss_lf", "loss_id1", "loss_id2", "loss")])
    grads = torch.cat([p.grad.flatten() for _, p in sorted(tr.ada.named_parameters())]).clone()
    return losses, grads


def test_trainer_step_bf16_within_twice_the_yardstick(monkeypatch):
    """(g) Trainer.backward on the train_64_b2 golden's inputs and weights: default, attn_precision
    "bf16", the yardstick (MHAdaAttnFn replaced by the autocast restatement), and default again."""
    g = load_golden("train_64_b2")
    c = seeded_image(2, 64, 64, int(g["content_seed"])).cuda()
    s = seeded_image(2, 64, 64, int(g["style_seed"])).cuda()
    l0, g0 = _trainer_run(Trainer(*build("cuda")), c, s)
    before = dict(ops.BF16_TRAIN_COUNTS)
    tb = Trainer(*build("cuda"), attn_precision="bf16")
    lb, gb = _trainer_run(tb, c, s)
    n_calls = 1 if tb.batch_adaformer else 3  # AdaFormer calls per step (the three batched into one)
    assert ops.BF16_TRAIN_COUNTS["fwd"] - before["fwd"] == 6 * n_calls == len(tb.ada.adaAttnHead) * n_calls
    assert ops.BF16_TRAIN_COUNTS["bwd"] - before["bwd"] == 6 * n_calls
    assert autograd_path.TRAIN_ATTN == "hip"
    with monkeypatch.context() as mp:
        mp.setattr(autograd_path, "MHAdaAttnFn", _YardFn)
        ly, gy = _trainer_run(Trainer(*build("cuda")), c, s)
    dev = lambda l: float(np.abs(l / g["losses"] - 1).max())  # noqa: E731
    dist = lambda a: float((a.double() - g0.double()).norm() / g0.double().norm())  # noqa: E731
    print(f"loss deviation from the golden: default {dev(l0):.3e} bf16 {dev(lb):.3e} yardstick {dev(ly):.3e}")
    print(f"AdaFormer gradient distance from the default run: bf16 {dist(gb):.3e} yardstick {dist(gy):.3e}")
    assert dev(lb) <= 2 * dev(ly)
    assert dist(gb) <= 2 * dist(gy)
    # the switch leaks no state: a default run after the bf16 run repeats the first one bit for bit
    counts = dict(ops.BF16_TRAIN_COUNTS)
    l1, g1 = _trainer_run(Trainer(*build("cuda")), c, s)
    assert ops.BF16_TRAIN_COUNTS == counts
    assert np.array_equal(l0, l1) and torch.equal(g0, g1)


def test_attn_train_bf16_never_stores_the_attention_matrix():
    """(h) One 8-head block's attention, forward + backward at B = 1 (BH = 8), Nc = Ns = 1024: the peak
    above what was live before the call stays below one fp32 attention matrix (4 BH Nc Ns bytes)."""
    BH, N = 8, 1024
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, x = (torch.randn(BH, N, 64, device="cuda", generator=g) * 0.5 for _ in range(4))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_(), x.requires_grad_()
    dout = torch.randn(BH, N, 64, device="cuda", generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    autograd_path.MHAdaAttnBf16Fn.apply(q, k, v, x).backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak / 2 ** 20:.1f} MiB of {4 * BH * N * N / 2 ** 20:.0f}")
    assert peak < 4 * BH * N * N
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v, x))
