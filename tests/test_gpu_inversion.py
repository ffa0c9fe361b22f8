"""Feature inversion on the HIP training kernels: an image that requires grad through the frozen
content ViT (visual_vit.py:88-112) and through the ViT plus the six MHAda blocks with no-grad style
features (visual_mhada.py:111-127), against the same modules evaluated by autograd_path in fp64 on the
CPU and against the reference's own golden (tests/golden/make_inversion_goldens.py).

Criterion for an image gradient g against the fp64 gradient g64: |g - g64| <= 1e-4 |g64| (L2), that of
test_vit_training_forward_matches_aten_autograd.  Measured on the MI355X: see
profiles/r13_inversion_accuracy.log."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import network
from mhada_hip import autograd_path, ops
from mhada_hip.inversion import invert_features
from mhada_hip.recipe import load_recipe, seeded_image
from conftest import load_golden

DEV = "cuda"
TOL = 1e-4


def frozen(m, dev=None, double=False):
    m = m.double() if double else m
    m = m.to(dev) if dev else m
    return m.eval().requires_grad_(False)


def vit(tag, heads=8):
    return load_recipe(network.VisionTransformer(pos_embedding=tag == "vit_c", num_heads=heads), tag)


def rel_l2(g, g64):
    g, g64 = g.detach().double().cpu(), g64.detach().double().cpu()
    return ((g - g64).norm() / g64.norm()).item()


def twice(t):
    return torch.cat([t, t])


def vit_loss(fwd, model, img, target):
    return sum(F.mse_loss(f, t) for f, t in zip(fwd(model, img), target))


def blocks(ada, fc, fs):
    """adaformer_forward without the decoder: the six blocks in the reference's order."""
    fcs = fc[0]
    for i in range(ada.num_layers):
        fcs = ada.adaAttnHead[2 * i](fc[i], fs[i], fcs)
        fcs = ada.adaAttnHead[2 * i + 1](fcs, fs[i], fcs)
    return fcs


@pytest.fixture(scope="module")
def vit_pair():
    return frozen(vit("vit_c"), DEV), frozen(vit("vit_c"), double=True)


def _vit_case(vit_pair, content, init):
    """(HIP image gradient, fp64 CPU image gradient, HIP loss, fp64 loss) of the ViT inversion loss."""
    v32, v64 = vit_pair
    with torch.no_grad():
        target = v32(content.to(DEV))
        target64 = autograd_path.vit_forward(v64, content.double())
    x = init.to(DEV).requires_grad_(True)
    loss = vit_loss(lambda m, i: m(i), v32, x, target)
    (g,) = torch.autograd.grad(loss, x)
    x64 = init.double().requires_grad_(True)
    loss64 = vit_loss(autograd_path.vit_forward, v64, x64, target64)
    (g64,) = torch.autograd.grad(loss64, x64)
    return g, g64, loss.item(), loss64.item()


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 64, 48)])
def test_frozen_vit_image_gradient_vs_fp64(vit_pair, B, H, W):
    content = seeded_image(B, H, W, 101)
    init = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(7))
    g, g64, loss, loss64 = _vit_case(vit_pair, content, init)
    e = rel_l2(g, g64)
    print(f"ViT inversion ({B}, {H}, {W}): loss {loss:.6g} fp64 {loss64:.6g}; |g64| {g64.norm().item():.4g}; "
          f"HIP rel L2 {e:.3e}")
    assert g.shape == init.shape and torch.isfinite(g).all()
    assert abs(loss - loss64) <= 1e-4 * abs(loss64)
    assert e <= TOL
    assert all(p.grad is None for p in vit_pair[0].parameters())


def test_routing_reaches_the_kernel_once_and_the_switch_restores_aten(vit_pair, monkeypatch):
    v32, _ = vit_pair
    calls = []
    real = ops.patch_embed_dgrad
    monkeypatch.setattr(ops, "patch_embed_dgrad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    content = seeded_image(1, 64, 64, 101)
    init = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        target = v32(content.to(DEV))

    def grad():
        x = init.to(DEV).requires_grad_(True)
        (g,) = torch.autograd.grad(vit_loss(lambda m, i: m(i), v32, x, target), x)
        return g

    assert autograd_path.VIT_INPUT_GRAD == "hip"
    g_hip = grad()
    assert len(calls) == 1
    with autograd_path.vit_input_grad("torch"):
        g_aten = grad()
    assert len(calls) == 1  # the aten route never reaches the kernel
    assert autograd_path.VIT_INPUT_GRAD == "hip"
    assert rel_l2(g_hip, g_aten) <= TOL
    with pytest.raises(ValueError):
        with autograd_path.vit_input_grad("aten"):
            pass


def _mhada_case(heads):
    vc, vs, ada = (frozen(vit("vit_c", heads), DEV), frozen(vit("vit_s", heads), DEV),
                   frozen(load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads), "ada"), DEV))
    vc64, vs64, ada64 = (frozen(vit("vit_c", heads), double=True), frozen(vit("vit_s", heads), double=True),
                         frozen(load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads), "ada"), double=True))
    content, style = seeded_image(1, 64, 64, 101), seeded_image(1, 64, 64, 102)
    init = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        fs = vs(style.to(DEV))
        target = blocks(ada, vc(content.to(DEV)), fs)
        fs64 = autograd_path.vit_forward(vs64, style.double())
        target64 = blocks(ada64, autograd_path.vit_forward(vc64, content.double()), fs64)
    before = dict(ops.BWD_PATH_COUNTS), dict(ops.DQ_ONLY_COUNTS)
    x = init.to(DEV).requires_grad_(True)
    loss = F.mse_loss(blocks(ada, vc(x), fs), target)
    (g,) = torch.autograd.grad(loss, x)
    after = dict(ops.BWD_PATH_COUNTS), dict(ops.DQ_ONLY_COUNTS)
    # the fp64 reference runs the image stacked twice along the batch axis: aten's CPU instance_norm
    # backward is wrong at B = 1 for a non-contiguous incoming gradient (make_inversion_goldens.py);
    # two identical samples give the same features and loss, and their two gradients sum in the leaf
    # to exactly the B = 1 gradient
    x64 = init.double().requires_grad_(True)
    loss64 = F.mse_loss(blocks(ada64, autograd_path.vit_forward(vc64, twice(x64)), [twice(f) for f in fs64]),
                        twice(target64))
    (g64,) = torch.autograd.grad(loss64, x64)
    assert all(p.grad is None for m in (vc, vs, ada) for p in m.parameters())
    return g, g64, loss.item(), loss64.item(), before, after


@pytest.mark.parametrize("heads", [8, 4, 16])
def test_vit_plus_mhada_blocks_image_gradient_vs_fp64(heads):
    g, g64, loss, loss64, before, after = _mhada_case(heads)
    e = rel_l2(g, g64)
    print(f"ViT + MHAda inversion, {heads} heads: loss {loss:.6g} fp64 {loss64:.6g}; |g64| {g64.norm().item():.4g}; "
          f"HIP rel L2 {e:.3e}")
    assert after[1]["dq_only"] - before[1]["dq_only"] == 6  # one dQ-only backward per block
    assert after[0] == before[0]  # neither the spill nor the recompute backward ran
    assert e <= TOL


def _attn_operands(BH, Nc, Ns, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(BH, Nc, D, generator=g) * 0.4
    k = torch.randn(BH, Ns, D, generator=g) * 0.4
    v = torch.randn(BH, Ns, D, generator=g) * 3.0
    v = v - v.mean(dim=1, keepdim=True)
    x = torch.randn(BH, Nc, D, generator=g)
    dout = torch.randn(BH, Nc, D, generator=g)
    return [t.to(DEV).contiguous() for t in (q, k, v, x, dout)]


@pytest.mark.parametrize("BH,Nc,Ns", [(2, 100, 70), (1, 64, 257)])
@pytest.mark.parametrize("D", [64, 32, 128])
def test_dq_only_ops_are_bit_identical_to_the_full_backward(D, BH, Nc, Ns):
    q, k, v, x, dout = _attn_operands(BH, Nc, Ns, D, seed=D + Nc)
    if D == 64:
        _, mo, lse = ops.attn_train_fwd(q, k, v, x)
        _, dmo, dd = ops.attn_train_bwd_prep(dout, x, mo)
        dq_full = ops.attn_train_bwd(q, k, v, lse, dmo, dd, spill=False)[0]
        dq = ops.attn_train_dq(q, k, v, lse, dmo, dd)
    else:
        _, mo, lse = ops.attn_train_fwd_hd(q, k, v, x)
        _, dmo, dd = ops.attn_train_bwd_prep_hd(dout, x, mo)
        dq_full = ops.attn_train_bwd_hd(q, k, v, lse, dmo, dd)[0]
        dq = ops.attn_train_dq_hd(q, k, v, lse, dmo, dd)
    assert torch.isfinite(dq).all() and dq.abs().max() > 0
    assert torch.equal(dq, dq_full)


def test_attn_fn_keeps_the_full_backward_when_keys_need_gradients():
    """k requires grad: the backward is today's (the counters of the 64-wide paths move, dq-only does not)."""
    q, k, v, x, dout = _attn_operands(2, 100, 70, 64, seed=3)
    q.requires_grad_(True)
    k.requires_grad_(True)
    before = dict(ops.BWD_PATH_COUNTS), dict(ops.DQ_ONLY_COUNTS)
    autograd_path.MHAdaAttnFn.apply(q, k, v, x).backward(dout)
    assert ops.DQ_ONLY_COUNTS == before[1]
    assert sum(ops.BWD_PATH_COUNTS.values()) == sum(before[0].values()) + 1
    assert k.grad is not None and q.grad is not None


def test_invert_features_loss_history_vs_fp64(vit_pair):
    """Ten Adam steps at 64 x 64, lr 0.5: the loss history against the same loop in fp64 on the CPU, step by
    step (fp64: 22006.35 falling to 20621.62)."""
    v32, v64 = vit_pair
    content = seeded_image(1, 64, 64, 101)
    init = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        target = v32(content.to(DEV))
        target64 = autograd_path.vit_forward(v64, content.double())
    img, hist = invert_features(v32, target, init.to(DEV), steps=10, lr=0.5)
    img64, hist64 = invert_features(lambda x: autograd_path.vit_forward(v64, x), target64, init.double(), steps=10, lr=0.5)
    print("HIP  ", " ".join(f"{h:.4f}" for h in hist))
    print("fp64 ", " ".join(f"{h:.4f}" for h in hist64))
    assert img.is_cuda and img.shape == init.shape and not img.requires_grad
    assert len(hist) == 10 and hist64[-1] < hist64[0]
    for a, b in zip(hist, hist64):
        assert abs(a - b) <= 1e-4 * abs(b)


def test_hip_path_matches_the_reference_golden(vit_pair):
    """The reference's own losses and image gradients (inversion_64.npz) at the criterion above."""
    gold = load_golden("inversion_64")
    g, _, loss, _ = _vit_case(vit_pair, seeded_image(1, 64, 64, 101),
                              torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(7)))
    e = rel_l2(g, torch.from_numpy(gold["grad_vit"]))
    print(f"ViT inversion vs reference golden: rel L2 {e:.3e}")
    assert abs(loss - gold["losses"][0]) <= 1e-4 * gold["losses"][0]
    assert e <= TOL
    g, _, loss, _, _, _ = _mhada_case(8)
    e = rel_l2(g, torch.from_numpy(gold["grad_ada"]))
    print(f"ViT + MHAda inversion vs reference golden: rel L2 {e:.3e}")
    assert abs(loss - gold["losses"][1]) <= 1e-4 * gold["losses"][1]
    assert e <= TOL
