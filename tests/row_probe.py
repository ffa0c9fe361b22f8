"""Probes, fp64 references and element-wise bounds for the bandwidth-bound row kernels (csrc/small_ops.hip,
csrc/train_ops.hip): LayerNorm, the ViT's batch-axis attention, the positional-embedding resize, the
InstanceNorm statistics, the weight fold, the cosine row normalisation and their training adjoints.

A plain helper module: it imports without a GPU (tests/test_row_forms_cpu.py checks it there,
tests/test_gpu_row_forms.py runs the kernels on it).  Everything is computed on the CPU in fp64; the
"f32" functions evaluate the same formulas with plain fp32 torch ops and fix the two constants below.

Notation: u = 2^-24, gamma(n) = n u / (1 - n u) (the error of n chained fp32 roundings).

LayerNorm (cols terms, any summation order):
  em   = gamma(cols + 1) mean|x|                      error of the computed mean: it scales with mean|x|, not |y|
  rel  = gamma(cols + 6) + C_RSQRT u + (em rstd)^2    relative error of rstd (the centred squares see em only
                                                      in second order: sum (x - mean) = 0)
  |y - ref| <= em rstd |g| (1 + rel) + |xh g| (rel + gamma(4)) + u |ref|   (+ 2^-8 |ref| for a bf16 store)
  stats: |mean - ref| <= em, |rstd - ref| <= rel rstd.
LayerNorm backward (stats handed over in fp32: dmean <= u |mean|, drstd <= u rstd):
  exh = u |mean| rstd + 3 u |xh|, gd = dy g, m1 = mean gd, m2 = mean gd xh,
  em1 = gamma(cols + 2) mean|gd|, em2 = gamma(cols + 3) mean|gd xh| + mean(|gd| exh),
  |dx - ref| <= rstd (u |gd| + em1 + |xh| em2 + exh |m2| + gamma(6) (|gd| + |m1| + |xh m2|));  dgamma, dbeta: gamma(rows + 4) sum|dy xh| + sum|dy| exh, gamma(rows + 4) sum|dy|.
Batch-axis attention (L keys, head width D, scale = 1 / sqrt(D)):
  es_ij = gamma(D + 2) scale sum_d |q_id k_jd|        error of a score
  re_ij = 2 es_ij + (C_EXP + 3 |s_ij - max_j s_ij|) u relative error of exp(s_ij - m): the score, the rounded
                                                      difference, and __expf (x log2 e rounds once per unit of |x|)
  RP_ij = re_ij + sum_k P_ik re_ik + gamma(L + 2)     relative error of P_ij
  |out_id - ref| <= sum_j P_ij |v_jd| (RP_ij + gamma(4 L + 8))   (the online kernels rescale at every key)
  backward: attn_bwd_bound, the same terms pushed through dP = dout v^T, dS = P (dP - sum P dP), dq, dk, dv.
Positional embedding: W is the dense fp64 resize matrix (F.interpolate of the identity basis);
  forward  |out - W p|   <= gamma(4 + 3) |W| |p| + ey Ly + ex Lx: the forward is PyTorch's fp32 resize, whose source
           coordinate fl(fl(fl(n / m) (o + 0.5)) - 0.5) carries e <= gamma(3) (s + 0.5); L is the largest neighbour
           difference of pos over the cells a coordinate within e of s can lie in (pos_fwd_bound),
  adjoint  |gpos - W^T g| <= gamma(n + 3) |W|^T |g|, n the nonzero weights of the column; a zero column is +0.0.
InstanceNorm (fp64 sums inside the kernel, N terms):
  |mu - ref| <= (u + 2^-50 N) |mean|,  |rstd - ref| <= rstd (u + 2^-51 (N + 4) E[x^2] / (var + eps))
  backward: m1, m2 fp64 means of fp32 terms (dy y rounds once), dx = (dy - m1 - y m2) rstd.
Fold: wq = wf rstd_c (one rounding), K half = wg rstd_s kscale (two), V half = wh, bkv = bg kscale (one),
  v_mu = bh + wh mu_s (65 terms).  Cosine prep: v / sqrt(sum v^2): gamma(32 + 2) + C_RSQRT u relative.
Backward prep: evar = gamma(2) (m^2 + |var|), esd = evar / (2 sd) + (1 + C_RSQRT) u sd, and so on in prep_bound.

The two intrinsic allowances cannot be derived here and are not written in the project:
  C_RSQRT  units of u allowed to rsqrtf / sqrtf beyond a correctly rounded result,
  C_EXP    units of u allowed to __expf at argument 0 (the |x| u growth is in re_ij).
They were fixed as attn_probe.C_BOUND was: evaluate the same formulas in fp32 torch on the test's own operands
(ln_f32, attn_f32, ...; never from the kernels) and choose the constants so that this evaluation stays within
half of every bound that holds one of them; test_row_forms_cpu.py asserts that (measured worst fp32-torch error /
bound with C_RSQRT = 4 and C_EXP = 8: LayerNorm 0.35, attention 0.024, its backward 0.009).
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_RSQRT = 4.0
C_EXP = 8.0
F64 = torch.float64


def gamma(n):
    return n * U / (1.0 - n * U)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, seed):
    """Gaussian fp64 values that are exactly representable in fp32."""
    return torch.randn(*shape, generator=gen(seed), dtype=F64).float().double()


# --------------------------------------------------------------------------------------------------
# plane splits (the documented ones, in torch)
# --------------------------------------------------------------------------------------------------
def split3(y):
    """[3][...] bf16 planes of an fp32 tensor: p0 = bf16(y), p1 = bf16(y - p0), p2 = bf16(y - p0 - p1)."""
    y = y.float()
    p0 = y.bfloat16()
    r1 = y - p0.float()
    p1 = r1.bfloat16()
    return torch.stack([p0, p1, (r1 - p1.float()).bfloat16()])


def half2_plane(v):
    q = v.half()
    return torch.where(q.float().abs() < 6.103515625e-05, torch.zeros_like(q), q)


def half2(y, scale):
    """[2][...] fp16 planes hi = fp16(s y), lo = fp16(s y - hi), subnormal plane values flushed to zero."""
    v = y.float() * scale
    hi = half2_plane(v)
    return torch.stack([hi, half2_plane(v - hi.float())])


# --------------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def ln_gauss(rows, cols, offset=0.0, seed=0):
    x = randn(rows, cols, seed=100 + seed) * 1.5 + randn(rows, 1, seed=200 + seed)
    if offset:
        x = (x + offset).float().double()
    return x, randn(cols, seed=300 + seed), randn(cols, seed=400 + seed)


def ln_exact(rows, cols):
    """x = m0 +- 2^k per row (as many of each sign: every partial sum is exact in any order), integer gamma and
    beta, distinct per column.  Returns x, g, b, m0, k."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(cols).view(1, -1)
    m0 = (r % 7 - 3).double()
    k = (r % 6 - 2).double()
    sign = torch.where((7 * c + 3 * r) % cols < cols // 2, 1.0, -1.0).double()
    x = m0 + sign * torch.pow(2.0, k)
    g = (1 + torch.arange(cols) % 7).double()
    b = (torch.arange(cols) - cols // 2).double()
    return x, g, b, m0.view(-1), k.view(-1)


def ln_ref(x, g, b, eps=LN_EPS, dt=F64):
    x, g, b = x.to(dt), g.to(dt), b.to(dt)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    return dict(y=d * rstd * g + b, xh=d * rstd, mean=mean.view(-1), rstd=rstd.view(-1))


def ln_f32(x, g, b, eps=LN_EPS):
    return ln_ref(x, g, b, eps, torch.float32)


def ln_bound(x, g, r, bf16_out=False):
    cols = x.shape[-1]
    rstd = r["rstd"].view(-1, 1)
    em = gamma(cols + 1) * x.abs().mean(-1, keepdim=True)
    rel = gamma(cols + 6) + C_RSQRT * U + (em * rstd) ** 2
    by = em * rstd * g.abs() * (1 + rel) + (r["xh"] * g).abs() * (rel + gamma(4)) + U * r["y"].abs()
    if bf16_out:
        by = by + 2.0 ** -8 * r["y"].abs()
    return dict(y=by, mean=em.view(-1), rstd=(rel * rstd).view(-1))


def ln_bwd_ref(x, dy, g, eps=LN_EPS):
    """fp64 autograd of the fp64 forward."""
    x = x.clone().requires_grad_(True)
    g = g.clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    ln_ref(x, g, b, eps)["y"].backward(dy)
    return dict(dx=x.grad, dgamma=g.grad, dbeta=b.grad)


def ln_bwd_bound(x, dy, g, r):
    rows, cols = x.shape
    rstd, mean, xh = r["rstd"].view(-1, 1), r["mean"].view(-1, 1), r["xh"]
    exh = U * mean.abs() * rstd + 3 * U * xh.abs()
    gd = dy * g
    m1, m2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    em1 = gamma(cols + 2) * gd.abs().mean(-1, keepdim=True)
    em2 = gamma(cols + 3) * (gd * xh).abs().mean(-1, keepdim=True) + (gd.abs() * exh).mean(-1, keepdim=True)
    dx = rstd * (U * gd.abs() + em1 + xh.abs() * em2 + exh * m2.abs()
                 + gamma(6) * (gd.abs() + m1.abs() + (xh * m2).abs()))
    dgamma = gamma(rows + 4) * (dy * xh).abs().sum(0) + (dy.abs() * exh).sum(0)
    dbeta = gamma(rows + 4) * dy.abs().sum(0)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


# --------------------------------------------------------------------------------------------------
# batch-axis attention: qkv [L][ntok][3][heads][D], out [L][ntok][heads D]
# --------------------------------------------------------------------------------------------------
def attn_gauss(L, ntok, heads, D, seed=0):
    qkv = randn(L, ntok, 3, heads, D, seed=500 + seed)
    qkv[:, :, 0] *= 3.0  # a moderately peaked softmax
    return qkv.float().double()


def select_map(L, ntok, heads):
    """sel[i][token][head]: the key query i selects; cyclic shifts (bijective) on two pairs of three, a
    two-to-one map on the third (so some key is selected twice and some never)."""
    i = torch.arange(L).view(L, 1, 1)
    p = (torch.arange(ntok).view(1, ntok, 1) * heads + torch.arange(heads).view(1, 1, heads))
    return torch.where(p % 3 == 2, (i // 2 + p) % L, (i + 1 + p) % L)


def attn_select(L, ntok, heads, D, bf16=False):
    """q_i = 64 e_i, k_j = 32 on the coordinates of the queries that select j: q_i . k_j = 2048 [sel(i) == j], so
    the scaled scores differ by 256 (D = 64), 181 (128) or 362 (32) >= 128 and exp underflows to exactly 0 off
    the selected key.  v: distinct integers per (i, token, head, d) (fp32); bf16: integers in [-254, 254] from the
    same index mod 509 (every one representable, neighbours in every direction distinct)."""
    assert L <= D
    sel = select_map(L, ntok, heads)
    qkv = torch.zeros(L, ntok, 3, heads, D, dtype=F64)
    i = torch.arange(L)
    qkv[i, :, 0, :, i] = 64.0
    onehot = F.one_hot(sel, L).double()           # [i][n][h][j]
    qkv[:, :, 1, :, :L] = 32.0 * onehot.permute(3, 1, 2, 0)  # k_j[d = i] = 32 [sel(i) == j]
    idx = torch.arange(L * ntok * heads * D).view(L, ntok, heads, D)
    qkv[:, :, 2] = ((idx * 37) % 509 - 254).double() if bf16 else (idx + 1).double()
    return qkv, sel


def attn_uniform(L, ntok, heads, D):
    """q = 0: every weight is exactly 1 / L (L a power of two); k and v small integers."""
    assert L in (2, 4, 8)
    idx = torch.arange(L * ntok * heads * D).view(L, ntok, heads, D)
    qkv = torch.zeros(L, ntok, 3, heads, D, dtype=F64)
    qkv[:, :, 1] = ((idx * 5) % 3 - 1).double()
    qkv[:, :, 2] = ((idx * 11) % 17 - 8).double()
    return qkv


def int_dout(L, ntok, heads, D):
    idx = torch.arange(L * ntok * heads * D).view(L, ntok, heads * D)
    return ((idx * 13) % 5 - 2).double()


def select_bwd_exact(sel, dout, heads, D):
    """dqkv of the select probe: dq = dk = 0, dv[r] = the sum of the dout rows whose query selected r."""
    L, ntok = sel.shape[:2]
    g = dout.view(L, ntok, heads, D)
    dv = torch.zeros(L, ntok, heads, D, dtype=F64)
    dv.scatter_add_(0, sel[..., None].expand(L, ntok, heads, D), g)
    z = torch.zeros_like(dv)
    return torch.stack([z, z, dv], 2)


def attn_parts(qkv, dt=F64):
    L, ntok, _, heads, D = qkv.shape
    q, k, v = (qkv[:, :, t].to(dt).permute(1, 2, 0, 3) for t in range(3))  # [n][h][L][D]
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    p = torch.softmax(s, -1)
    return q, k, v, s, p


def attn_ref(qkv, dt=F64):
    """out [L][ntok][heads D]."""
    L, ntok, _, heads, D = qkv.shape
    q, k, v, s, p = attn_parts(qkv, dt)
    return (p @ v).permute(2, 0, 1, 3).reshape(L, ntok, heads * D)


def attn_f32(qkv):
    return attn_ref(qkv, torch.float32)


def _attn_rp(q, k, s, p, L, D):
    scale = 1.0 / math.sqrt(D)
    es = gamma(D + 2) * scale * (q.abs() @ k.abs().transpose(-1, -2))
    re = 2 * es + (C_EXP + 3 * (s - s.amax(-1, keepdim=True)).abs()) * U
    return re + (p * re).sum(-1, keepdim=True) + gamma(L + 2)


def attn_bound(qkv, bf16_out=False):
    L, ntok, _, heads, D = qkv.shape
    q, k, v, s, p = attn_parts(qkv)
    rp = _attn_rp(q, k, s, p, L, D)
    b = ((p * (rp + gamma(4 * L + 8))) @ v.abs()).permute(2, 0, 1, 3).reshape(L, ntok, heads * D)
    if bf16_out:
        b = b + 2.0 ** -8 * attn_ref(qkv).abs()
    return b


def attn_bwd_ref(qkv, dout):
    """fp64 autograd of the fp64 forward: dqkv like qkv."""
    x = qkv.clone().requires_grad_(True)
    attn_ref(x).backward(dout)
    return x.grad


def attn_bwd_bound(qkv, dout):
    L, ntok, _, heads, D = qkv.shape
    scale = 1.0 / math.sqrt(D)
    q, k, v, s, p = attn_parts(qkv)
    g = dout.view(L, ntok, heads, D).permute(1, 2, 0, 3)
    rp = _attn_rp(q, k, s, p, L, D)
    dp = g @ v.transpose(-1, -2)
    edp = gamma(D + 1) * (g.abs() @ v.abs().transpose(-1, -2))
    a = (p * dp.abs()).sum(-1, keepdim=True)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    eds = p * (rp * (dp.abs() + a) + edp + (p * (edp + rp * dp.abs())).sum(-1, keepdim=True)
               + gamma(L + 4) * (dp.abs() + a))
    bq = scale * (eds @ k.abs() + gamma(L + 3) * (ds.abs() @ k.abs()))
    bk = scale * (eds.transpose(-1, -2) @ q.abs() + gamma(L + 3) * (ds.abs().transpose(-1, -2) @ q.abs()))
    bv = (p * (rp + gamma(L + 3))).transpose(-1, -2) @ g.abs()
    return torch.stack([t.permute(2, 0, 1, 3) for t in (bq, bk, bv)], 2)  # [L][ntok][3][heads][D]


# --------------------------------------------------------------------------------------------------
# positional embedding: pos [C][bh][bw] -> out [oh ow][C]; adjoint g [oh ow][C] -> gpos [C][bh][bw]
# --------------------------------------------------------------------------------------------------
POS_SIZES = [((4, 6), (4, 6)), ((5, 3), (11, 7)), ((8, 8), (3, 5)), ((1, 4), (6, 9)), ((4, 4), (1, 1)), ((3, 2), (2, 9))]


def resize_matrix(bh, bw, oh, ow, dt=F64):
    """W [oh ow][bh bw]: the resize of the identity basis."""
    eye = torch.eye(bh * bw, dtype=dt).view(bh * bw, 1, bh, bw)
    if (bh, bw) == (oh, ow):
        return eye.view(bh * bw, bh * bw).clone()
    w = F.interpolate(eye, size=(oh, ow), mode="bilinear", align_corners=False)
    return w.view(bh * bw, oh * ow).t().contiguous()


def pos_fwd(pos, W):
    C = pos.shape[0]
    return W @ pos.reshape(C, -1).t().to(W.dtype)                # [oh ow][C]


def pos_coord(n, m):
    """Per target index of an n -> m resize: the exact source coordinate s = max(((2 o + 1) n - m) / (2 m), 0),
    its floor i0, and the bound gamma(3) (s + 0.5) on the error of the fp32 coordinate fl(fl(fl(n / m) (o + 0.5))
    - 0.5): the quotient, the product and the difference round once each."""
    o = torch.arange(m, dtype=F64)
    s = torch.clamp(((2 * o + 1) * n - m) / (2.0 * m), min=0.0)
    return s, torch.clamp(s.floor().long(), max=n - 1), gamma(3) * (s + 0.5)


def _cells(s, i0, e):
    """The cells [j, j + 1] a coordinate within e of s can lie in: its own, and a neighbour's where s is within e
    of an integer (there the fp32 floor may fall on either side)."""
    return [i0] + ([i0 - 1] if s - i0 <= e else []) + ([i0 + 1] if i0 + 1 - s <= e else [])


def _lipschitz(p, ca, cb, axis):
    """max |p[j + 1] - p[j]| along `axis` over the cells the perturbed coordinate can lie in (ca, cb: (s, i0, e)
    of the axis and of the other axis, whose pixels j, j + 1 of each cell count).  p [C][bh][bw] -> [oa][ob][C]."""
    d = p.diff(dim=axis).abs()                                       # differences along the axis
    if axis == 2:
        d = d.transpose(1, 2)                                        # [C][along][across]
    C, na, nb = d.shape
    (sa, ia, ea), (sb, ib, eb) = ca, cb
    out = torch.zeros(len(ia), len(ib), C, dtype=F64)
    for a in range(len(ia)):
        ja = [j for j in _cells(sa[a].item(), ia[a].item(), ea[a].item()) if 0 <= j < na]
        for b in range(len(ib)):
            cells = _cells(sb[b].item(), ib[b].item(), eb[b].item())
            jb = sorted({j for c in cells for j in (c, c + 1) if 0 <= j < nb})
            if ja:
                out[a, b] = d[:, ja][:, :, jb].amax((1, 2))
    return out


def pos_fwd_bound(pos, W, dst):
    """gamma(4 + 3) |W| |p| for the four products and sums and the weights' own roundings, plus the error of the
    fp32 source coordinates, which the operation has by definition (PyTorch's fp32 bilinear resize, which
    tests/test_gpu_kernels.py::test_pos_embed pins to 1e-6): the bilinear interpolant is continuous and piecewise
    linear in each coordinate, so a coordinate error e moves it by at most e times the largest neighbour
    difference of the cells it can lie in (a floor that flips at an integer coordinate included)."""
    C, bh, bw = pos.shape
    oh, ow = dst
    b = gamma(4 + 3) * (W.abs() @ pos.reshape(C, -1).t().abs())
    if (bh, bw) == (oh, ow):
        return b
    cy, cx = pos_coord(bh, oh), pos_coord(bw, ow)
    ly = _lipschitz(pos, cy, cx, 1)                                  # [oh][ow][C]
    lx = _lipschitz(pos, cx, cy, 2).transpose(0, 1)                  # [oh][ow][C]
    return b + (cy[2].view(-1, 1, 1) * ly + cx[2].view(1, -1, 1) * lx).reshape(oh * ow, C)


def pos_bwd(g, W):
    return (W.t() @ g.to(W.dtype)).t().contiguous()              # [C][bh bw]


def pos_bwd_bound(g, W):
    n = (W != 0).sum(0).double().view(-1, 1)                     # nonzero weights per source pixel
    return (gamma(n + 3) * (W.abs().t() @ g.abs())).t().contiguous()


# --------------------------------------------------------------------------------------------------
# InstanceNorm statistics and backward: x [B][N][C]
# --------------------------------------------------------------------------------------------------
IN_EPS = 1e-5


def in_ref(x, eps=IN_EPS):
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)   # two-pass: well conditioned at any offset
    return dict(mu=mean, rstd=torch.rsqrt(var + eps), var=var)


def in_bound(x, r, eps=IN_EPS):
    N = x.shape[1]
    return dict(mu=(U + 2.0 ** -50 * N) * r["mu"].abs(),
                rstd=r["rstd"] * (U + 2.0 ** -51 * (N + 4) * (x * x).mean(1) / (r["var"] + eps)))


def in_bwd_ref(dy, y, rstd):
    """dx = (dy - mean_N dy - y mean_N(dy y)) rstd: the fp64 autograd of (x - mu) rstd with y its output."""
    m1, m2 = dy.mean(1, keepdim=True), (dy * y).mean(1, keepdim=True)
    return (dy - m1 - y * m2) * rstd[:, None]


def in_bwd_bound(dy, y, rstd):
    m1, m2 = dy.mean(1, keepdim=True), (dy * y).mean(1, keepdim=True)
    e1 = 2 * U * m1.abs()
    e2 = U * (dy * y).abs().mean(1, keepdim=True) + 2 * U * m2.abs()
    return rstd[:, None] * (e1 + y.abs() * e2 + gamma(5) * (dy.abs() + m1.abs() + (y * m2).abs()))


# --------------------------------------------------------------------------------------------------
# weight fold (head width 64)
# --------------------------------------------------------------------------------------------------
def fold_operands(B, H, exact, seed=0):
    D = 64
    o = dict(wf=randn(H, D, D, seed=600 + seed), wg=randn(H, D, D, seed=601 + seed), wh=randn(H, D, D, seed=602 + seed),
             bg=randn(H * D, seed=603 + seed), bh=randn(H * D, seed=604 + seed), mu_s=randn(B, H * D, seed=605 + seed))
    if exact:  # powers of two
        c = torch.arange(B * H * D).view(B, H * D)
        o["rstd_c"] = torch.pow(2.0, (c % 5 - 2).double())
        o["rstd_s"] = torch.pow(2.0, ((c // 3) % 4 - 1).double())
    else:
        o["rstd_c"] = (randn(B, H * D, seed=606 + seed).abs() + 0.25).float().double()
        o["rstd_s"] = (randn(B, H * D, seed=607 + seed).abs() + 0.25).float().double()
    return o


def fold_ref(o, kscale, B, H):
    D = 64
    rc, rs, ms = (o[n].view(B, H, 1, D) for n in ("rstd_c", "rstd_s", "mu_s"))
    wq = o["wf"][None] * rc
    wk = o["wg"][None] * rs * kscale
    wkv = torch.cat([wk, o["wh"][None].expand(B, H, D, D)], 2)          # [B][H][2 D][D]
    bkv = torch.cat([(o["bg"] * kscale).view(H, D), torch.zeros(H, D, dtype=F64)], 1).reshape(-1)
    acc = (o["wh"][None] * ms).sum(-1)                                  # [B][H][D]
    mag = (o["wh"][None] * ms).abs().sum(-1) + o["bh"].view(1, H, D).abs()
    v_mu = (acc + o["bh"].view(1, H, D)).reshape(B, H * D)
    return dict(wq=wq, wkv=wkv, bkv=bkv, v_mu=v_mu, v_mu_mag=mag.reshape(B, H * D))


def fold_bound(r, bf16):
    extra = 2.0 ** -8 if bf16 else 0.0
    return dict(wq=(U + extra) * r["wq"].abs(), wkv=(gamma(2) + extra) * r["wkv"].abs(), bkv=U * r["bkv"].abs(),
                v_mu=gamma(65) * r["v_mu_mag"])


# --------------------------------------------------------------------------------------------------
# cosine prep: rows of 64 normalised in place
# --------------------------------------------------------------------------------------------------
def rownorm_ref(x):
    return x / x.pow(2).sum(-1, keepdim=True).sqrt()


def rownorm_bound(ref, bf16):
    return (gamma(32 + 2) + C_RSQRT * U + (2.0 ** -8 if bf16 else 0.0)) * ref.abs()


# --------------------------------------------------------------------------------------------------
# attention backward prep: rows of D channels, mo = [m | e2]
# --------------------------------------------------------------------------------------------------
CLAMP = torch.tensor(1e-6, dtype=torch.float32)                       # 1e-6f
CLAMP_BELOW = torch.nextafter(CLAMP, torch.tensor(0.0))               # the fp32 value just below
CLAMP_ABOVE = torch.nextafter(CLAMP, torch.tensor(1.0))               # the fp32 value just above
# with m = 2^-3 (m^2 = 2^-6 exact, contracted or not): e2 = 2^-6 + k 2^-29, var = k 2^-29 exactly
VAR_GRID_BELOW = 536 * 2.0 ** -29   # 9.98e-7 < 1e-6f
VAR_GRID_ABOVE = 537 * 2.0 ** -29   # 1.0002e-6 > 1e-6f


def prep_gauss(rows, D, seed=0):
    m = randn(rows, D, seed=700 + seed)
    e2 = (m * m + randn(rows, D, seed=701 + seed).abs() + 0.1).float().double()
    return randn(rows, D, seed=702 + seed), randn(rows, D, seed=703 + seed), m, e2


def prep_clamp_rows(D):
    """Five rows whose var sits just below, exactly at and just above 1e-6f (m = 0, var = e2), and just below /
    above on the 2^-29 grid (m = 1/8).  Returns dout, x, m, e2, active (True: the clamp is active, dvar = 0)."""
    m = torch.zeros(5, D, dtype=F64)
    m[3:] = 0.125
    e2 = torch.empty(5, D, dtype=F64)
    e2[0], e2[1], e2[2] = CLAMP_BELOW.double(), CLAMP.double(), CLAMP_ABOVE.double()
    e2[3], e2[4] = 2.0 ** -6 + VAR_GRID_BELOW, 2.0 ** -6 + VAR_GRID_ABOVE
    c = torch.arange(D).double()
    dout = (1 + c % 3).expand(5, D).contiguous()
    x = (1 + c % 5).expand(5, D).contiguous()
    return dout, x, m, e2, torch.tensor([True, False, False, True, False])


def prep_ref(dout, x, m, e2, dt=F64):
    dout, x, m, e2 = (t.to(dt) for t in (dout, x, m, e2))
    var = e2 - m * m
    sd = torch.sqrt(torch.clamp(var, min=float(CLAMP)))
    on = var >= float(CLAMP)
    dvar = torch.where(on, dout * x * 0.5 / sd, torch.zeros_like(sd))
    dm = dout - 2.0 * m * dvar
    return dict(dx=dout * sd, dm=dm, dvar=dvar, dd=(dm * m + dvar * e2).sum(-1), var=var, sd=sd)


def prep_bound(dout, x, m, e2, r):
    D = m.shape[-1]
    evar = gamma(2) * (m * m + r["var"].abs())  # the product and the difference round once each; not attributed term by term
    esd = evar / (2 * r["sd"]) + (1 + C_RSQRT) * U * r["sd"]
    edvar = r["dvar"].abs() * (gamma(4) + esd / r["sd"])
    edm = 2 * m.abs() * edvar + gamma(3) * (dout.abs() + 2 * (m * r["dvar"]).abs())
    edd = (m.abs() * edm + e2.abs() * edvar).sum(-1) + gamma(D + 2) * ((r["dm"] * m).abs() + (r["dvar"] * e2).abs()).sum(-1)
    return dict(dx=dout.abs() * esd + U * r["dx"].abs(), dm=edm, dvar=edvar, dd=edd)
