"""The fused temporal losses on the GPU (csrc/temporal.hip; video.TemporalLossFn and the two public
*_hip functions): the reference's goldens, an fp64 restatement of mhada_hip.losses, the resize
prologue against aten, no host synchronisation, determinism, guard rows, the all-zero mask and one
VideoTrainer.backward with the flag on and off.

Tolerances against fp64 (test_fused_route_is_as_close_to_fp64_as_the_aten_route): none is a fixed
number.  Per tensor kind (loss, dx2, dx1) the error of the aten device route (the mhada_hip.losses
expressions around video.warp, on the same inputs) against the fp64 CPU evaluation of the same
expressions is measured over all the cases below, as max|x - ref| / max|ref|; the fused route must
stay within twice the largest of them in every case.  The fused path sums in fp64; the factor 2
covers the atomics' ordering in dx1.  Measured on an MI355X (profiles/r31_temporal_loss_accuracy.log):
the aten route's largest errors are 1.13e-7 (loss), 1.11e-6 (dx2) and 8.79e-7 (dx1); the fused route's
are 0.48x, 1.03x and 1.00x of them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import load_golden
from mhada_hip import losses as L
from mhada_hip import ops
from mhada_hip.video import TemporalLossFn, feature_level_temporal_loss_hip, output_level_temporal_loss_hip

MSE = torch.nn.MSELoss(reduction="none")


# ---- the losses.py expressions on explicit (flow, mask): lossfn.py:50-66 with c1 / c2, else lossfn.py:81-86 ----
def losses_expr(x1, x2, flow, m, c1, c2):
    if c1 is not None:
        return L.output_level_temporal_loss(c1, c2, x1, x2, flow, m, MSE)
    warped = L._warp(x1, flow)
    fm = m.unsqueeze(1).expand(-1, x1.shape[1], -1, -1)
    loss = torch.sum(fm * MSE(x2, warped))
    return loss * (1 / torch.nonzero(fm).shape[0])


def with_grads(fn, x1, x2, *rest):
    x1, x2 = x1.detach().requires_grad_(True), x2.detach().requires_grad_(True)
    loss = fn(x1, x2, *rest)
    g1, g2 = torch.autograd.grad(loss, (x1, x2))
    return loss.detach(), g2, g1


def fused(x1, x2, flow, m, c1, c2):
    return TemporalLossFn.apply(x1, x2, flow, m, c1, c2)


def as_layout(t, layout):
    """[B,C,H,W] values in contiguous NCHW storage or as a channels_last view of [B,H,W,C] storage."""
    if layout == "nchw":
        return t.contiguous()
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def sample_pos(flow):
    """The warp's fp32 sample positions (csrc/warp_tap.h, utilities.py:112-113 + grid_sampler_unnormalize)."""
    B, _, H, W = flow.shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gx = 2.0 * (xx + flow[:, 0]) / max(W - 1, 1) - 1.0
    gy = 2.0 * (yy + flow[:, 1]) / max(H - 1, 1) - 1.0
    return ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0


def make_flow(B, H, W, seed):
    """Displacements up to the frame size, so taps fall outside all four borders; a few pixels sample the
    centre (x + fx = (W - 1) / 2, whose position W / 2 - 1/2 is an integer for odd W, and equal weights
    for even W; likewise y); one pixel has zero flow."""
    g = torch.Generator().manual_seed(seed)
    flow = torch.randn(B, 2, H, W, generator=g) * torch.tensor([W / 2.0, H / 2.0]).view(1, 2, 1, 1)
    for y, x in ((0, 0), (H - 1, W - 1), (H // 2, W // 3), (1, W - 2)):
        flow[:, 0, y, x] = (W - 1) / 2.0 - x
        flow[:, 1, y, x] = (H - 1) / 2.0 - y
    flow[:, :, H // 3, W // 2] = 0.0
    ix, iy = sample_pos(flow)
    assert ix.min() < -1 and ix.max() > W and iy.min() < -1 and iy.max() > H  # beyond all four borders
    assert W % 2 == 0 or int((ix == ix.round()).sum()) >= 4 * B  # exactly on integer positions
    assert H % 2 == 0 or int((iy == iy.round()).sum()) >= 4 * B
    return flow


def make_mask(kind, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ones":
        return torch.ones(B, H, W)
    if kind == "band":
        m = torch.ones(B, H, W)
        m[:, H // 4:H // 2 + 1] = 0.0
        return m
    m = torch.rand(B, H, W, generator=g) * 1.5  # non-binary weights, some exact zeros
    m[torch.rand(B, H, W, generator=g) < 0.25] = 0.0
    return m


# name: (B, C, H, W, layout, with the luminance target, fed by mhada_flow_mask_resize from 32 x 48)
SHAPES = {
    "c3_13x17_nchw_t": (2, 3, 13, 17, "nchw", True, False),       # PIX, one channel group
    "c3_13x17_cl_t": (2, 3, 13, 17, "cl", True, False),           # CH, one channel per lane, with t
    "c512_4x6_cl_resized": (2, 512, 4, 6, "cl", False, True),     # CH, 16 B per lane, two passes of 256 channels
    "c512_4x6_nchw_resized": (2, 512, 4, 6, "nchw", False, True),  # PIX, 32 channel groups
    "c5_9x8_nchw": (1, 5, 9, 8, "nchw", False, False),            # PIX, one block
    "c5_9x8_cl": (1, 5, 9, 8, "cl", False, False),                # CH, C % 4 != 0
}
MASKS = ("ones", "band", "weights")
CASES = [(s, m) for s in SHAPES for m in MASKS]


def make_case(shape, mask_kind):
    B, C, H, W, layout, with_t, resized = SHAPES[shape]
    seed = sorted(SHAPES).index(shape) * 10 + MASKS.index(mask_kind)
    g = torch.Generator().manual_seed(1000 + seed)
    x1, x2 = (as_layout(torch.randn(B, C, H, W, generator=g), layout) for _ in range(2))
    c1 = c2 = None
    if with_t:
        c1, c2 = torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)
    if resized:
        flow, m = ops.flow_mask_resize(make_flow(B, 32, 48, seed).cuda(), make_mask(mask_kind, B, 32, 48, seed).cuda(),
                                       (H, W))
        flow, m = flow.cpu(), m.cpu()
    else:
        flow, m = make_flow(B, H, W, seed), make_mask(mask_kind, B, H, W, seed)
    return x1, x2, flow, m, c1, c2


def rel_err(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def measured():
    """Every case once: the fp64 CPU reference, the aten device route and the fused route, as
    (loss, dx2, dx1) errors against the reference."""
    out = {}
    for shape, mask_kind in CASES:
        case = make_case(shape, mask_kind)
        ref = with_grads(losses_expr, *(None if t is None else t.double() for t in case))
        dev = [None if t is None else t.cuda() for t in case]
        assert dev[0].stride() == case[0].stride()  # the layout under test reaches the kernel
        aten = with_grads(losses_expr, *dev)
        ours = with_grads(fused, *dev)
        assert ours[0].dim() == 0 and ours[0].is_cuda and ours[1].shape == dev[1].shape
        out[shape, mask_kind] = ([rel_err(a, r) for a, r in zip(aten, ref)], [rel_err(a, r) for a, r in zip(ours, ref)])
    aten_max = [max(v[0][i] for v in out.values()) for i in range(3)]
    ours_max = [max(v[1][i] for v in out.values()) for i in range(3)]
    for k, (a, o) in out.items():
        print(f"temporal fp64 {k[0]:>22s} {k[1]:>7s}: aten loss/dx2/dx1 {a[0]:.2e} {a[1]:.2e} {a[2]:.2e}  "
              f"fused {o[0]:.2e} {o[1]:.2e} {o[2]:.2e}")
    print("temporal fp64 largest: aten " + " ".join(f"{v:.3e}" for v in aten_max) + "  fused "
          + " ".join(f"{v:.3e}" for v in ours_max) + "  ratio " + " ".join(f"{o / a:.3f}" for o, a in zip(ours_max, aten_max)))
    return out, aten_max


@pytest.mark.parametrize("shape,mask_kind", CASES)
def test_fused_route_is_as_close_to_fp64_as_the_aten_route(measured, shape, mask_kind):
    out, aten_max = measured
    _, ours = out[shape, mask_kind]
    for name, e, bound in zip(("loss", "dx2", "dx1"), ours, aten_max):
        assert e <= 2 * bound, (name, e, bound)


def test_fused_losses_match_the_reference_goldens():
    """The inputs of test_oracle_golden.test_temporal_losses_match_reference on the device, at the rtol
    that test grants the aten restatement."""
    g = load_golden("video_warp")
    t = {k: torch.from_numpy(g[k]).cuda() for k in ("c1", "c2", "cs1", "cs2", "flow", "mask", "f1", "f2")}
    m = t["mask"].unsqueeze(0)
    out = output_level_temporal_loss_hip(t["c1"], t["c2"], t["cs1"] * 255, t["cs2"] * 255, t["flow"][:1], m)
    assert out.dim() == 0 and out.is_cuda
    np.testing.assert_allclose(float(out), float(g["out_temporal"]), rtol=1e-5)
    feat = feature_level_temporal_loss_hip(t["f1"], t["f2"], t["flow"][:1], m)
    assert feat.dim() == 0 and feat.is_cuda
    np.testing.assert_allclose(float(feat), float(g["feat_temporal"]), rtol=1e-5)


def resize_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    flow = 4 * torch.randn(B, 2, H, W, generator=g)
    mask = (torch.rand(B, H, W, generator=g) > 0.6).float()
    mask[:, H // 3:H // 3 + H // 3] = 0.0  # a band wide enough to give all-zero neighbourhoods
    return flow, mask


def aten_resize(flow, mask, size):
    """lossfn.py:71-80"""
    ff = F.interpolate(flow, size=size, mode="bilinear")
    ff[:, 0] *= float(size[1]) / flow.shape[3]
    ff[:, 1] *= float(size[0]) / flow.shape[2]
    fm = F.interpolate(mask.unsqueeze(1), size=size, mode="bilinear").squeeze(1)
    return ff, (fm > 0).float(), fm


@pytest.fixture(scope="module")
def resize_measured():
    """Both grids once: aten on the CPU, aten on the device and the kernel."""
    out = {}
    for size, (H, W) in (((4, 6), (32, 48)), ((3, 5), (20, 37))):
        flow, mask = resize_inputs(2, H, W, 7 * H + W)
        ff_cpu, fm_cpu, raw = aten_resize(flow, mask, size)
        # the mask's interpolated values are exact zeros or far from rounding to one
        assert bool(((raw == 0) | (raw > 1e-3)).all()) and 0 < int((raw == 0).sum()) < raw.numel()
        ff_dev, fm_dev, _ = aten_resize(flow.cuda(), mask.cuda(), size)
        ff, fm = ops.flow_mask_resize(flow.cuda(), mask.cuda(), size)
        ulp = float(torch.finfo(torch.float32).eps * ff_cpu.abs().max())
        out[size] = dict(fm=fm, fm_dev=fm_dev, fm_cpu=fm_cpu, aten=float((ff_dev.cpu() - ff_cpu).abs().max()) / ulp,
                         ours=float((ff - ff_dev).abs().max()) / ulp)
        print(f"flow_mask_resize {size} from {(H, W)}: aten device vs aten CPU {out[size]['aten']:.3f} ulp of the "
              f"largest flow; kernel vs aten device {out[size]['ours']:.3f} ulp")
    return out


@pytest.mark.parametrize("size", [(4, 6), (3, 5)])
def test_flow_mask_resize_matches_aten(resize_measured, size):
    """The mask exactly; the flow as close to aten on the device as aten on the device is to aten on the
    CPU (the largest of the two grids' measured distances, in ulp of the largest flow value)."""
    r = resize_measured[size]
    assert torch.equal(r["fm"], r["fm_dev"]) and torch.equal(r["fm"].cpu(), r["fm_cpu"])
    assert r["ours"] <= max(v["aten"] for v in resize_measured.values())


def test_fused_losses_do_not_synchronise_with_the_host():
    """Under sync debug mode "error" both fused losses and their backward run clean; the losses.py route
    raises on its torch.nonzero."""
    g = torch.Generator().manual_seed(5)
    B, H, W, C, h, w = 2, 16, 24, 64, 4, 6
    c1, c2, cs2 = (torch.randn(B, 3, H, W, generator=g).cuda() for _ in range(3))
    cs1 = torch.randn(B, 3, H, W, generator=g).cuda().requires_grad_(True)
    f1 = as_layout(torch.randn(B, C, h, w, generator=g), "cl").cuda().requires_grad_(True)
    f2 = as_layout(torch.randn(B, C, h, w, generator=g), "cl").cuda().requires_grad_(True)
    flow = make_flow(B, H, W, 5).cuda()
    mask = make_mask("weights", B, H, W, 5).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            L.output_level_temporal_loss(c1, c2, cs1, cs2, flow, mask, MSE)
        with pytest.raises(RuntimeError):
            L.feature_level_temporal_loss(f1, f2, flow, mask, MSE)
        ot = output_level_temporal_loss_hip(c1, c2, cs1, cs2, flow, mask)
        ft = feature_level_temporal_loss_hip(f1, f2, flow, mask)
        (2.0 * ot + 2.0 * ft).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ot.dim() == 0 and ft.dim() == 0 and ot.is_cuda and ft.is_cuda
    assert cs1.grad is not None and f1.grad is not None and f2.grad is not None
    assert bool(torch.isfinite(ot)) and bool(torch.isfinite(ft)) and float(f2.grad.abs().max()) > 0


@pytest.mark.parametrize("shape", ["c3_13x17_nchw_t", "c512_4x6_cl_resized", "c512_4x6_nchw_resized", "c5_9x8_cl"])
def test_forward_and_dx2_are_bit_identical_over_five_runs(shape):
    dev = [None if t is None else t.cuda() for t in make_case(shape, "weights")]
    runs = [with_grads(fused, *dev) for _ in range(5)]
    for loss, dx2, _ in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(dx2, runs[0][1])


@pytest.mark.parametrize("shape", ["c3_13x17_nchw_t", "c512_4x6_cl_resized", "c5_9x8_cl", "c5_9x8_nchw"])
def test_padded_gradients_leave_their_guard_rows_untouched(shape):
    """dx1 / dx2 as views into larger allocations filled with NaN: the kernel writes the views only."""
    x1, x2, flow, m, c1, c2 = (None if t is None else t.cuda() for t in make_case(shape, "weights"))
    B, C, H, W = x1.shape
    loss, work = ops.temporal_loss_fwd(x1, x2, flow, m, c1, c2)
    g = torch.full((), 0.75, device="cuda")
    want1, want2 = ops.temporal_loss_bwd(x1, x2, flow, m, c1, c2, work, g)
    bigs, views = [], []
    for _ in range(2):
        if SHAPES[shape][4] == "nchw":
            big = torch.full((B, C + 2, H + 4, W + 3), float("nan"), device="cuda")
            view = big[:, 1:1 + C, 2:2 + H, 1:1 + W]
        else:
            big = torch.full((B, H + 4, W + 3, C + 4), float("nan"), device="cuda")
            view = big[:, 2:2 + H, 1:1 + W, 4:4 + C].permute(0, 3, 1, 2)
        bigs.append(big)
        views.append(view)
    inside = []
    for big, view in zip(bigs, views):
        view.zero_()
        inside.append(~torch.isnan(big))
        assert int(inside[-1].sum()) == view.numel()
    ops.temporal_loss_bwd(x1, x2, flow, m, c1, c2, work, g, dx1=views[0], dx2=views[1])
    torch.cuda.synchronize()
    for big, ins in zip(bigs, inside):
        assert bool(torch.isnan(big[~ins]).all())
    assert torch.equal(views[1], want2)
    torch.testing.assert_close(views[0], want1, rtol=1e-5, atol=1e-6 * float(want1.abs().max()))
    # either gradient alone
    only1, none2 = ops.temporal_loss_bwd(x1, x2, flow, m, c1, c2, work, g, need_dx2=False)
    none1, only2 = ops.temporal_loss_bwd(x1, x2, flow, m, c1, c2, work, g, need_dx1=False)
    assert none1 is None and none2 is None and torch.equal(only2, want2)
    torch.testing.assert_close(only1, want1, rtol=1e-5, atol=1e-6 * float(want1.abs().max()))


def test_all_zero_mask_gives_nan_without_a_fault():
    x1, x2, flow, m, c1, c2 = (None if t is None else t.cuda() for t in make_case("c3_13x17_nchw_t", "ones"))
    loss, dx2, dx1 = with_grads(fused, x1, x2, flow, torch.zeros_like(m), c1, c2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)) and dx2.shape == x2.shape and dx1.shape == x1.shape
    f = feature_level_temporal_loss_hip(as_layout(torch.randn(1, 8, 2, 3), "cl").cuda(), torch.randn(1, 8, 2, 3).cuda(),
                                        flow[:1], torch.zeros_like(m[:1]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(f))


def test_video_trainer_backward_with_and_without_the_fused_temporal_losses():
    """One VideoTrainer.backward on the train_video_64x128_s64_b2 golden's inputs with the flag on and off:
    every loss entry within rtol 1e-5.  The AdaFormer gradient of the fused step is as far from the aten
    step's as two aten steps are from each other (atomic scatters in both), plus a margin of 1e-5 of the
    gradient's norm: 1/50 of the fp32 noise of these gradients against fp64 (4.9e-4,
    test_train_cpu.test_video_golden_fp32_noise_yardstick), for the last-bit differences of the loss
    gradients that the whole backward pass then carries."""
    from mhada_hip.recipe import seeded_image
    from mhada_hip.train import VideoTrainer
    from test_train_cpu import build
    g = load_golden("train_video_64x128_s64_b2")
    fh, fw = (int(x) for x in g["frame_shape"])
    sh, sw = (int(x) for x in g["style_shape"])
    style = seeded_image(2, sh, sw, int(g["seeds"][0])).cuda()
    c1, c2 = (seeded_image(2, fh, fw, int(x)).cuda() for x in g["seeds"][1:])
    flow, mask = torch.from_numpy(g["flow"]).cuda(), torch.from_numpy(g["mask"]).cuda()
    tr = VideoTrainer(*build("cuda"))
    assert tr.fused_temporal_losses is True
    keys = ("loss_gs", "loss_lf", "loss_ot", "loss_ft", "loss_id1", "loss_id2", "loss")
    runs = []
    for flag in (True, False, False):
        tr.fused_temporal_losses = flag
        out = tr.backward(style, c1, c2, flow, mask)
        runs.append((np.array([float(out[k].detach()) for k in keys]),
                     torch.cat([p.grad.double().flatten() for p in tr.ada.parameters() if p.grad is not None])))
    np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=1e-5)
    norm = float(runs[1][1].norm())
    d_on_off = float((runs[0][1] - runs[1][1]).norm()) / norm
    d_off_off = float((runs[2][1] - runs[1][1]).norm()) / norm
    print(f"VideoTrainer AdaFormer gradient distance / norm: fused vs aten {d_on_off:.3e}, aten vs aten {d_off_off:.3e}")
    assert d_on_off <= d_off_off + 1e-5
