"""Every form of mhada_conv2d and the two Inception pools, element by element (csrc/conv2d.hip).

fp64 F.conv2d on the same fp32 operands is the only oracle.  Each case is one geometry of the InceptionV3
trunk (kernel, stride, padding as torchvision sets them), B = 2 on a 9 x 11 or a 10 x 8 map, with random-sign
scale and shift (so negative ones occur) and the ReLU, and is run twice: dense, and into channels
c_off .. c_off + Cout of a wider buffer (the concat write).  Checked:

  bound    every element within 2 gamma_n (|scale| S + |shift|) of fp64, S = sum |x| |w| of that element
           (computed by the same fp64 conv on the absolute values), gamma_n = n u / (1 - n u), u = 2^-24,
           n = KH KW Cin + 2 (one fp32 FMA per term of the K walk in whatever order, one rounding for the
           scale, one for the shift); the factor 2 is the GEMM suite's headroom.  ReLU is 1-Lipschitz.
  canary   x, w and y sit inside larger allocations whose guards hold a quiet-NaN bit pattern, as do the
           channels of the concat buffer outside the slice: y's guards and neighbouring channels must keep
           their bits, a read that strays into a guard turns the output into NaN, and the concat run must
           return the dense run's bits.

The 64-thread 32 x 64 tile serves every small case; the two `big` cases have enough 128 x 64 tiles to take
the 256-thread form on a device of up to 256 CUs, with M no multiple of 128 and Cout no multiple of 64.
Cin = 3 in this table goes through the general kernel: ops.inception_input pads the image to 4 channels,
conv2d_pack_weight the filter.  The trunk's own first layer is the direct fp64 kernel mhada_conv2d_stem
(test_conv2d_stem): it is held to ONE fp32 rounding of the fp64 value, |got - ref| <= 2^-24 |ref| plus
2^-50 (|scale| S + |shift|) for the fp64 chain of up to 77 terms, on every geometry and both strides, with and
without the fused 2 x - 1, on an image like the reference's (within 0.008 of a constant), dense and as a
concat write with guards.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"
else:
    DEV = "cpu"

NAN32 = 0x7FC12345
GUARD = 64  # floats before and after every tensor
UR = 2.0 ** -24

# (KH, KW), padding as the trunk uses the geometry (3 x 3 occurs with and without padding)
GEOMETRIES = [((1, 1), (0, 0)), ((3, 3), (0, 0)), ((3, 3), (1, 1)), ((5, 5), (2, 2)), ((1, 7), (0, 3)), ((7, 1), (3, 0)),
              ((1, 3), (0, 1)), ((3, 1), (1, 0))]
MAPS = [(2, 9, 11), (2, 10, 8)]


def gamma(n):
    return n * UR / (1 - n * UR)


def case(k, pad, stride, grid, ci, co):
    B, H, W = grid
    name = f"k{k[0]}x{k[1]}_p{pad[0]}{pad[1]}_s{stride}_b{B}_{H}x{W}_{ci}to{co}"
    return pytest.param(dict(k=k, pad=pad, stride=stride, grid=grid, ci=ci, co=co, name=name), id=name)


def _cases():
    c = []
    for k, pad in GEOMETRIES:  # every geometry, both strides, an odd and an even map; ragged K (48) and N (80)
        for stride in (1, 2):
            for grid in MAPS:
                c.append(case(k, pad, stride, grid, 48, 80))
    for ci in (3, 32, 80, 160, 448):  # 48 is above; 3 = the stem
        c.append(case((3, 3), (1, 1), 1, MAPS[0], ci, 80))
    c.append(case((3, 3), (0, 0), 2, MAPS[0], 3, 32))  # Conv2d_1a_3x3
    for co in (32, 192, 320):  # 80 is above
        c.append(case((1, 1), (0, 0), 1, MAPS[1], 32, co))
        c.append(case((3, 3), (1, 1), 2, MAPS[0], 32, co))
    c.append(case((1, 1), (0, 0), 1, (2, 60, 57), 48, 320))  # big: 54 x 5 tiles of 128 x 64, M = 6840
    c.append(case((3, 3), (0, 0), 2, (2, 121, 117), 32, 320))  # big, stride 2 on odd sizes: 60 x 58 outputs
    return c


CASES = _cases()


def guarded(t):
    """t copied into the middle of a NaN-filled device allocation: (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), NAN32, dtype=torch.int32, device=DEV).view(F32)
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_intact(buf, n):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == NAN32).all() and (b[GUARD + n:] == NAN32).all())


@functools.lru_cache(maxsize=None)
def problem(name):
    fm = next(p.values[0] for p in CASES if p.values[0]["name"] == name)
    B, H, W = fm["grid"]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randn(B, fm["ci"], H, W, generator=g)
    w = torch.randn(fm["co"], fm["ci"], *fm["k"], generator=g) / (fm["ci"] * fm["k"][0] * fm["k"][1]) ** 0.5
    scale = (0.5 + torch.rand(fm["co"], generator=g)) * (1 - 2 * (torch.rand(fm["co"], generator=g) < 0.5).float())
    shift = 0.5 * torch.randn(fm["co"], generator=g)
    conv = F.conv2d(x.double(), w.double(), None, fm["stride"], fm["pad"])
    s_abs = F.conv2d(x.double().abs(), w.double().abs(), None, fm["stride"], fm["pad"])
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    ref = torch.relu(conv * sc + sh).permute(0, 2, 3, 1).contiguous()
    n = fm["k"][0] * fm["k"][1] * fm["ci"] + 2
    bound = (2 * gamma(n) * (sc.abs() * s_abs + sh.abs())).permute(0, 2, 3, 1).contiguous()
    assert (ref > 0).any() and (ref == 0).any()  # the ReLU cuts some and passes some
    assert (scale < 0).any() and (shift < 0).any()
    return dict(fm=fm, x=x, w=w, scale=scale, shift=shift, ref=ref, bound=bound)


def device_operands(p):
    fm = p["fm"]
    if fm["ci"] == 3:  # the stem form: the 4-padded image, made by the device kernel
        xd = ops.inception_input(p["x"].to(DEV), normalize=False)
        assert torch.equal(xd[..., :3].cpu(), p["x"].permute(0, 2, 3, 1)) and bool((xd[..., 3] == 0).all())
        xd, xbuf = guarded(xd)
    else:
        xd, xbuf = guarded(p["x"].permute(0, 2, 3, 1).contiguous())
    wd, wbuf = guarded(ops.conv2d_pack_weight(p["w"]))
    return xd, wd, p["scale"].to(DEV), p["shift"].to(DEV)


@pytest.mark.parametrize("fm", CASES)
def test_conv2d_form(fm):
    p = problem(fm["name"])
    xd, wd, scale, shift = device_operands(p)
    ref, bound = p["ref"], p["bound"]
    B, Ho, Wo, Co = ref.shape
    y, ybuf = guarded(torch.zeros(B, Ho, Wo, Co))
    ybuf.view(torch.int32).fill_(NAN32)
    ops.conv2d(xd, wd, scale, shift, stride=fm["stride"], padding=fm["pad"], out=y)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, y.numel())
    got = y.cpu()
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"{fm['name']}: largest error / bound {worst:.4f}")
    assert worst <= 1.0

    # the concat write: channels c_off .. c_off + Co of rows ldc apart; everything else keeps its bits
    c_off, ldc = 12, Co + 12 + 7
    z, zbuf = guarded(torch.zeros(B, Ho, Wo, ldc))
    zbuf.view(torch.int32).fill_(NAN32)
    ops.conv2d(xd, wd, scale, shift, stride=fm["stride"], padding=fm["pad"], out=z, c_off=c_off)
    torch.cuda.synchronize()
    assert guards_intact(zbuf, z.numel())
    zi = z.view(torch.int32)
    assert bool((zi[..., :c_off] == NAN32).all()) and bool((zi[..., c_off + Co:] == NAN32).all())
    assert torch.equal(z[..., c_off:c_off + Co].contiguous().view(torch.int32).cpu(), got.view(torch.int32))


def test_conv2d_no_relu_and_repeat():
    p = problem(CASES[0].values[0]["name"])
    fm = p["fm"]
    xd, wd, scale, shift = device_operands(p)
    a = ops.conv2d(xd, wd, scale, shift, stride=fm["stride"], padding=fm["pad"], relu=False)
    b = ops.conv2d(xd, wd, scale, shift, stride=fm["stride"], padding=fm["pad"], relu=False)
    r = ops.conv2d(xd, wd, scale, shift, stride=fm["stride"], padding=fm["pad"], relu=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool((a < 0).any()) and torch.equal(torch.relu(a), r)


@pytest.mark.parametrize("grid,C", [((2, 9, 11), 64), ((2, 10, 8), 288), ((1, 3, 3), 4), ((2, 35, 33), 192)])
def test_maxpool3s2(grid, C):
    B, H, W = grid
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + H))
    ref = F.max_pool2d(x, 3, 2).permute(0, 2, 3, 1).contiguous()
    xd, _ = guarded(x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.maxpool3s2(xd).cpu(), ref)
    c_off, ldc = 8, C + 8 + 4
    z, zbuf = guarded(torch.zeros(*ref.shape[:3], ldc))
    zbuf.view(torch.int32).fill_(NAN32)
    ops.maxpool3s2(xd, z, c_off)
    torch.cuda.synchronize()
    assert guards_intact(zbuf, z.numel())
    zi = z.view(torch.int32)
    assert bool((zi[..., :c_off] == NAN32).all()) and bool((zi[..., c_off + C:] == NAN32).all())
    assert torch.equal(z[..., c_off:c_off + C].cpu(), ref)


@pytest.mark.parametrize("grid,C", [((2, 9, 11), 64), ((2, 10, 8), 288), ((1, 1, 1), 4), ((1, 2, 5), 8), ((2, 35, 33), 192)])
def test_avgpool3(grid, C):
    B, H, W = grid
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + W)) + 1.0
    ref = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=True).permute(0, 2, 3, 1)
    s_abs = F.avg_pool2d(x.double().abs(), 3, 1, 1, count_include_pad=True).permute(0, 2, 3, 1)
    xd, _ = guarded(x.permute(0, 2, 3, 1).contiguous())
    got = ops.avgpool3(xd).cpu()
    # eight additions and the division: 9 roundings of magnitudes below sum |x| / 9 ... sum |x|
    assert bool(((got.double() - ref).abs() <= gamma(9) * 9 * s_abs).all())
    # the divisor is 9 at the border too: a corner holds the sum of its (up to) four in-range taps / 9
    corner = x[:, :, :2, :2].double().sum(dim=(2, 3)) / 9.0
    assert torch.allclose(got[:, 0, 0, :].double(), corner, rtol=1e-6, atol=1e-6)


def test_rejected_arguments_launch_nothing():
    lib = _lib.load()
    x = torch.randn(1, 6, 6, 8, device=DEV)
    w = torch.randn(16, 3, 3, 8, device=DEV)
    sc = torch.ones(16, device=DEV)
    y = torch.full((1, 4, 4, 16), NAN32, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def conv(xp=None, B=1, H=6, W=6, ci=8, co=16, kh=3, kw=3, stride=1, ph=0, pw=0, ldc=16, c_off=0, relu=1):
        return lib.mhada_conv2d(x.data_ptr() if xp is None else xp, w.data_ptr(), sc.data_ptr(), sc.data_ptr(),
                                y.data_ptr(), B, H, W, ci, co, kh, kw, stride, ph, pw, ldc, c_off, relu, st)

    bad = [dict(kh=2, kw=2), dict(kh=7, kw=7), dict(kh=3, kw=5), dict(stride=3), dict(stride=0), dict(ci=6), dict(ci=3),
           dict(ldc=15), dict(c_off=1), dict(c_off=-1, ldc=32), dict(ph=3), dict(pw=-1), dict(kh=1, kw=1, ph=1), dict(B=0),
           dict(H=2), dict(xp=0), dict(xp=x.data_ptr() + 4), dict(relu=2)]
    for kw in bad:
        assert conv(**kw) == 1, kw
        assert lib.mhada_last_error()
    assert lib.mhada_maxpool3s2(x.data_ptr(), y.data_ptr(), 1, 2, 6, 8, 8, 0, st) == 1
    assert lib.mhada_maxpool3s2(x.data_ptr(), y.data_ptr(), 1, 6, 6, 6, 8, 0, st) == 1
    assert lib.mhada_maxpool3s2(x.data_ptr(), y.data_ptr(), 1, 6, 6, 8, 8, 4, st) == 1
    assert lib.mhada_avgpool3(x.data_ptr(), 0, 1, 6, 6, 8, st) == 1
    assert lib.mhada_inception_input(0, y.data_ptr(), 1, 6, 6, 1, st) == 1
    torch.cuda.synchronize()
    assert bool((y == NAN32).all())
    assert conv() == 0  # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.view(F32)).all())
    with pytest.raises(RuntimeError):
        ops.conv2d(x.cpu(), w.cpu(), sc.cpu(), sc.cpu())


STEM_CASES = [(k, pad, stride, grid) for k, pad in GEOMETRIES for stride in (1, 2) for grid in ((2, 9, 11), (1, 10, 8))] + \
             [((3, 3), (0, 0), 2, (2, 139, 123))]  # Conv2d_1a_3x3 on the golden's size: several workgroups


@pytest.mark.parametrize("k,pad,stride,grid", STEM_CASES,
                         ids=[f"k{k[0]}x{k[1]}_p{p[0]}{p[1]}_s{s}_b{g[0]}_{g[1]}x{g[2]}" for k, p, s, g in STEM_CASES])
@pytest.mark.parametrize("normalize", (True, False), ids=["norm", "plain"])
def test_conv2d_stem(k, pad, stride, grid, normalize):
    B, H, W = grid
    Co = 32
    g = torch.Generator().manual_seed(zlib.crc32(f"stem{k}{pad}{stride}{grid}".encode()))
    # the reference's input scale: levels v / 255 / 255 (2 x - 1 within 0.008 of -1); plain: Gaussian
    x = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255 / 255) if normalize else torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(Co, 3, *k, generator=g) / (3 * k[0] * k[1]) ** 0.5
    scale = ((0.5 + torch.rand(Co, generator=g)) * (1 - 2 * (torch.rand(Co, generator=g) < 0.5).float())).double() * 30
    xin = 2 * x.double() - 1 if normalize else x.double()
    conv = F.conv2d(xin, w.double(), None, stride, pad)
    # a BatchNorm that removes the constant, as the trunk's first one does: shift = beta - mean * scale
    shift = 0.1 * torch.randn(Co, generator=g).double() - conv.mean(dim=(0, 2, 3)) * scale
    s_abs = F.conv2d(xin.abs(), w.double().abs(), None, stride, pad)
    sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    ref = torch.relu(conv * sc + sh).permute(0, 2, 3, 1).contiguous()
    bound = (UR * ref.abs() + 2.0 ** -50 * (sc.abs() * s_abs + sh.abs()).permute(0, 2, 3, 1))
    assert (ref > 0).any() and (ref == 0).any()
    xd, _ = guarded(x)
    wd, _ = guarded(ops.conv2d_pack_weight(w))
    assert wd.shape[3] == 4
    wd[..., 3] = float("nan")  # the fourth channel is not read
    y, ybuf = guarded(torch.zeros(*ref.shape))
    ybuf.view(torch.int32).fill_(NAN32)
    ops.conv2d_stem(xd, wd, scale.to(DEV), shift.to(DEV), stride=stride, padding=pad, normalize=normalize, out=y)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, y.numel())
    got = y.cpu()
    assert torch.isfinite(got).all()
    worst = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"stem k{k} s{stride} {grid} normalize {normalize}: largest error / bound {worst:.3f}")
    assert bool(((got.double() - ref).abs() <= bound).all())
    c_off, ldc = 5, Co + 5 + 3
    z, zbuf = guarded(torch.zeros(*ref.shape[:3], ldc))
    zbuf.view(torch.int32).fill_(NAN32)
    ops.conv2d_stem(xd, wd, scale.to(DEV), shift.to(DEV), stride=stride, padding=pad, normalize=normalize, out=z, c_off=c_off)
    torch.cuda.synchronize()
    assert guards_intact(zbuf, z.numel())
    zi = z.view(torch.int32)
    assert bool((zi[..., :c_off] == NAN32).all()) and bool((zi[..., c_off + Co:] == NAN32).all())
    assert torch.equal(z[..., c_off:c_off + Co].contiguous().view(torch.int32).cpu(), got.view(torch.int32))


def test_stem_rejected_arguments_launch_nothing():
    lib = _lib.load()
    x = torch.rand(1, 3, 6, 6, device=DEV)
    w = torch.randn(16, 3, 3, 4, device=DEV)
    sc = torch.ones(16, device=DEV, dtype=F64)
    y = torch.full((1, 4, 4, 16), NAN32, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def stem(xp=None, B=1, H=6, W=6, co=16, kh=3, kw=3, stride=1, ph=0, pw=0, ldc=16, c_off=0, relu=1, norm=1):
        return lib.mhada_conv2d_stem(x.data_ptr() if xp is None else xp, w.data_ptr(), sc.data_ptr(), sc.data_ptr(),
                                     y.data_ptr(), B, H, W, co, kh, kw, stride, ph, pw, ldc, c_off, relu, norm, st)

    for kw in (dict(kh=2, kw=2), dict(stride=3), dict(ldc=15), dict(c_off=-1, ldc=32), dict(ph=3), dict(B=0), dict(H=2),
               dict(xp=0), dict(relu=2), dict(norm=2)):
        assert stem(**kw) == 1, kw
        assert lib.mhada_last_error()
    torch.cuda.synchronize()
    assert bool((y == NAN32).all())
    assert stem() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.view(F32)).all())
