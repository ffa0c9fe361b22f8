"""Every inference attention kernel form, element by element (csrc/attn.hip, attn_split3.hip, cosine.hip,
attn_hd.hip, loss_attn.hip).

FORMS is a table of rows, each naming the kernel it is meant to reach, the dispatch condition that sends it
there and the knobs that pin it (DESIGN.md "Attention forms under test" holds the same table;
profiles/r12_attn_forms_kernels.txt is the kernel trace of this file).  Every row runs every shape of
attn_probe.SHAPES its dispatch condition admits (H = 8), and at each shape every probe of tests/attn_probe.py
(softmax: the three key maps x the three level schedules, the query map rotating; cosine: key maps x query
maps).  The probes make every attention weight a power of two (or 0, 1, 2) and every V' an integer, so one
mis-addressed, dropped or twice-counted key moves an element far outside the bound
(tests/test_attn_probe_cpu.py shows that on the CPU).  Each probe is checked four ways:

  bound   every output element within attn_probe.bound of the fp64 reference (C_BOUND = 10, fixed on the
          CPU from an fp32 torch evaluation, not from the kernels).  bf16 kernels are held to the SAME
          bound plus the 2^-8 |ref| rounding of their output: their operands, P and V'^2 are exact in bf16.
  canary  the C entry called on pointers into flat buffers filled with NaN bit patterns: GUARD rows before
          and after the [B Nc][C] output must hold the pattern, every payload element must be written and
          finite; q, kv, the vt / img / mom image and fcs sit inside larger NaN-filled buffers of their own
          (a read past a tensor poisons the output); the output must equal the ops wrapper's bit for bit.
  repeat  a second call returns identical bits.
  side    mhada_transpose_v positions Ns .. ldt - 1 are zero, mhada_split3_kv rows / positions past Ns are
          zero, mom[..., 64, 128] == Ns, and each image's guards hold.

Largest error / bound per form (profiles/r12_attn_forms_bounds.log): fp32 outputs 0.14 (loss_attn_w1_cosine) to
0.53 (loss_attn_w1_nch2_softmax); bf16 outputs 0.996 (the 2^-8 |ref| term is the bf16 rounding itself).
The file found one defect: loss_attn_kernel rounded s log2 e before subtracting the running max, 1.10 to
5.41 times the bound (at C = 8) on the "l8" probes at Ns = 1024 and 4096; it now forms
exp2(fma(s, log2 e, -m2)) as loss_attn_lds_kernel does.
"""

import pytest
import torch

import attn_probe as P

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
if torch.cuda.is_available():
    from mhada_hip import _lib, ops
    DEV = "cuda"
    CUS = torch.cuda.get_device_properties(0).multi_processor_count
else:  # collection without a GPU: the table is still built (every test here is marked gpu)
    DEV, CUS = "cpu", 256

DEFAULT_KNOBS = dict(attn_fixed_shift=1, attn_waves=0, attn_tk=128)
NAN32, NAN16 = 0x7FC12345, 0x7FC1  # guard bit patterns (quiet NaNs), as test_gpu_gemm_forms.py
GUARD = 3                          # guard rows before and after the output
PAD = 256                          # NaN elements before and after every operand
H = 8
SOFTMAX, COSINE = 0, 1


# --------------------------------------------------------------------------------------------------
# the form table
# --------------------------------------------------------------------------------------------------
def ragged(B, Nc, Ns):
    return Ns % 128 != 0


def whole(B, Nc, Ns):
    return Ns % 128 == 0


def form(name, kernel, cond, *, kind, dt, act, D=64, Dv=None, knobs=None, ok=None, shapes=None, splits=0):
    return dict(name=name, kernel=kernel, cond=cond, kind=kind, dt=dt, act=act, D=D, Dv=Dv or D, knobs=knobs or {},
                ok=ok, shapes=shapes, splits=splits)


def _forms():
    f = []
    acts = (("softmax", SOFTMAX), ("cosine", COSINE))
    # ---- mhada_attn: launch_attn<NW> in csrc/attn.hip -------------------------------------------------
    for an, a in acts:
        for nw in (4, 8):
            f.append(form(f"attn_f32_{an}_w{nw}", f"attn_f32_kernel<{an}, {nw}>", f"fp32, attn_waves = {nw}", kind="attn",
                          dt=F32, act=a, knobs=dict(attn_waves=nw)))
        for nw, tk, tile in ((8, 128, 128), (8, 64, 64), (4, 128, 64)):
            f.append(form(f"attn_bf16_{an}_w{nw}_tk{tile}", f"attn_bf16_kernel<{an}, {nw}, {tile}>",
                          f"bf16, attn_fixed_shift = 0, attn_waves = {nw}" + (f", attn_tk = {tk}" if nw == 8 else
                                                                              " (4 waves: always 64-key tiles)"),
                          kind="attn", dt=BF16, act=a, knobs=dict(attn_fixed_shift=0, attn_waves=nw, attn_tk=tk)))
    f.append(form("attn_bf16_fs_w8", "attn_bf16_fs_kernel<8, 128>", "bf16 softmax, fixed shift, 8 waves, Ns % 128 != 0",
                  kind="attn", dt=BF16, act=SOFTMAX, knobs=dict(attn_fixed_shift=1, attn_waves=8), ok=ragged))
    for nw in (4, 8):
        f.append(form(f"attn_bf16_fsq_w{nw}", f"attn_bf16_fsq_kernel<{nw}>",
                      f"bf16 softmax, fixed shift, {nw} waves, Ns % 128 == 0", kind="attn", dt=BF16, act=SOFTMAX,
                      knobs=dict(attn_fixed_shift=1, attn_waves=nw), ok=whole))
    f.append(form("attn_bf16_fs_w4_ragged", "attn_bf16_kernel<softmax, 4, 64>",
                  "bf16 softmax, fixed shift, 4 waves, Ns % 128 != 0: falls back to the online kernel", kind="attn",
                  dt=BF16, act=SOFTMAX, knobs=dict(attn_fixed_shift=1, attn_waves=4), ok=ragged))
    # attn_waves = 0: 4 waves while B H ceil(Nc / 256) < CUs, else 8
    n8 = -(-CUS // (2 * H))  # 256-query blocks per (b, h) at B = 2 that reach the CU count
    f.append(form("attn_bf16_auto_below", "attn_bf16_fsq_kernel<4> | attn_bf16_kernel<softmax, 4, 64>",
                  "attn_waves = 0, B H ceil(Nc / 256) < CUs (every table shape, and one block below the switch)",
                  kind="attn", dt=BF16, act=SOFTMAX, knobs=dict(attn_fixed_shift=1, attn_waves=0),
                  shapes=P.SHAPES + [(2, 256 * (n8 - 1), 128)]))
    f.append(form("attn_bf16_auto_above", "attn_bf16_fs_kernel<8, 128> | attn_bf16_fsq_kernel<8>",
                  "attn_waves = 0, B H ceil(Nc / 256) >= CUs", kind="attn", dt=BF16, act=SOFTMAX,
                  knobs=dict(attn_fixed_shift=1, attn_waves=0), shapes=[(2, 256 * n8 - 37, Ns) for Ns in (33, 128, 384)]))
    # ---- the other entry points ---------------------------------------------------------------------------
    for nw in (4, 8):
        f.append(form(f"attn_split3_w{nw}", f"attn_s3_kernel<{nw}>", f"mhada_attn_split3, attn_waves = {nw}", kind="split3",
                      dt=F32, act=SOFTMAX, knobs=dict(attn_waves=nw)))
    for dt, dn in ((F32, "f32"), (BF16, "bf16")):
        f.append(form(f"cosine_linear_{dn}", f"cosine_mom_kernel<{dn}> + cosine_mom_finish_kernel + cosine_attn_kernel<{dn}>",
                      "mhada_cosine_moments at the wrapper's split count min(ceil(Ns / 64), ceil(512 / (B H))), "
                      "mhada_cosine_attn", kind="cosmom", dt=dt, act=COSINE))
        f.append(form(f"cosine_linear_{dn}_split1", f"cosine_mom_kernel<{dn}> + cosine_attn_kernel<{dn}>",
                      "mhada_cosine_moments with splits = 1 (no finish kernel)", kind="cosmom", dt=dt, act=COSINE, splits=1))
    for D in (32, 128):
        for dt, dn in ((F32, "f32"), (BF16, "bf16")):
            for an, a in acts:
                f.append(form(f"attn_hd{D}_{dn}_{an}", f"attn_hd_{dn}_kernel<{D}, {an}>", f"mhada_attn_hd, D = {D}",
                              kind="hd", dt=dt, act=a, D=D))
    # mhada_loss_attn: W = d_v / 64 waves, dsl = ceil(d_qk / 8 W) 8; the LDS form at W = 4 and dsl <= 112;
    # nch = ceil(dsl / 128) Q chunks per wave
    for an, a in acts:
        f.append(form(f"loss_attn_lds_{an}", f"loss_attn_lds_kernel<{an}>", "d_v = 256, d_qk = 64 (dsl = 8 <= 112)",
                      kind="loss", dt=F32, act=a, D=64, Dv=256))
        for W, dqk in ((1, 64), (2, 64), (4, 452), (8, 64)):
            f.append(form(f"loss_attn_w{W}_{an}", f"loss_attn_kernel<{an}, {W}>",
                          f"d_v = {64 * W}, d_qk = {dqk}" + (" (dsl = 120 > 112: not the LDS form)" if W == 4 else ""),
                          kind="loss", dt=F32, act=a, D=dqk, Dv=64 * W))
        f.append(form(f"loss_attn_w1_nch2_{an}", f"loss_attn_kernel<{an}, 1>", "d_v = 64, d_qk = 136 (dsl = 136: nch = 2)",
                      kind="loss", dt=F32, act=a, D=136, Dv=64))
    return f


FORMS = _forms()


def _cases():
    """(form, shape), shape-major so that the references of one shape are shared by every row."""
    shapes = list(P.SHAPES)
    for fm in FORMS:
        for s in fm["shapes"] or ():
            if s not in shapes:
                shapes.append(s)
    out = []
    for s in shapes:
        for fm in FORMS:
            if s in (fm["shapes"] or P.SHAPES) and (fm["ok"] is None or fm["ok"](*s)):
                out.append(pytest.param(fm, s, id=f"{fm['name']}-{'x'.join(map(str, s))}"))
    return out


CASES = _cases()


def test_every_row_runs_at_least_three_shapes():
    for fm in FORMS:
        n = sum(1 for c in CASES if c.values[0] is fm)
        assert n >= 3, fm["name"]


# --------------------------------------------------------------------------------------------------
# probes, references (shared per shape) and NaN-filled buffers
# --------------------------------------------------------------------------------------------------
_cache = {"shape": None, "probe": {}}


def probe_and_reference(shape, fm, spec):
    """(probe rounded to the form's operand type, fp64 evaluation, bound), computed once per shape."""
    if _cache["shape"] != shape:
        _cache["shape"], _cache["probe"] = shape, {}
        if DEV == "cuda":
            torch.cuda.empty_cache()
    loss = fm["kind"] == "loss"
    key = (fm["D"], fm["Dv"], fm["act"], loss, fm["dt"], spec)
    if key not in _cache["probe"]:
        B, Nc, Ns = shape
        km, qm, lv = spec
        p = P.Probe(B, 1 if loss else H, Nc, Ns, fm["D"], fm["Dv"], "softmax" if fm["act"] == SOFTMAX else "cosine",
                    km, qm, lv, natural=loss, device=DEV).rounded(fm["dt"])
        if loss:  # mhada_loss_attn takes V itself, not a centred V': no v_mu is added back
            p.v_mu = torch.zeros_like(p.v_mu)
        r = P.evaluate(p)
        _cache["probe"][key] = (p, r["out"], P.bound(p, r, bf16_out=fm["dt"] == BF16))
    return _cache["probe"][key]


def nan_fill(n, dtype):
    if dtype == F32:
        return torch.full((n,), NAN32, dtype=torch.int32, device=DEV).view(F32)
    return torch.full((n,), NAN16, dtype=torch.int16, device=DEV).view(BF16)


class NanBuf:
    """A tensor of `shape` inside a flat NaN-pattern buffer, `pad` pattern elements before and after it."""

    def __init__(self, dtype, shape, src=None, pad=PAD):
        self.dtype, self.shape, self.pad = dtype, tuple(shape), pad
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.flat = nan_fill(self.n + 2 * pad, dtype)
        if src is not None:
            self.t.copy_(src.reshape(self.shape))

    @property
    def t(self):
        return self.flat[self.pad:self.pad + self.n].view(self.shape)

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.pad * self.flat.element_size()

    def guards_intact(self):
        iv = self.flat.view(torch.int32 if self.dtype == F32 else torch.int16)
        pat = NAN32 if self.dtype == F32 else NAN16
        return bool((iv[:self.pad] == pat).all()) and bool((iv[self.pad + self.n:] == pat).all())


def ceil64(n):
    return -(-n // 64) * 64


def call(name, *args):
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream().cuda_stream), name)


def pad_positions(Ns, dtype):
    """Positions of the keys Ns .. ldt - 1 in a V'^T image (bf16 and SPLIT3 images swap bits 2 and 3)."""
    n = torch.arange(Ns, ceil64(Ns), device=DEV)
    return P.swap23(n) if dtype == BF16 else n


# --------------------------------------------------------------------------------------------------
# one probe through one form: the ops wrappers, then the C entries on NaN-guarded buffers
# --------------------------------------------------------------------------------------------------
def operands(fm, p):
    dt = fm["dt"]
    f32 = lambda t: t.float().contiguous()  # noqa: E731
    o = dict(fcs=f32(p.fcs), mu=f32(p.mu), rs=f32(p.rstd), vmu=f32(p.v_mu))
    if fm["kind"] == "loss":
        o.update(q=f32(p.q[:, 0]), k=f32(p.k[:, 0]), v=f32(p.v[:, 0]))
    else:
        o.update(q=p.q.to(dt).contiguous(), kv=torch.cat([p.k, p.v], -1).to(dt).contiguous())
    return o


def wrapper_splits(B, Ns):
    return max(1, min((Ns + 63) // 64, -(-512 // (B * H))))


def run_wrappers(fm, p, o):
    kind, act = fm["kind"], fm["act"]
    if kind == "attn":
        return ops.mhada_attn(o["q"], o["kv"], ops.transpose_v(o["kv"]), o["fcs"], o["mu"], o["rs"], o["vmu"], act)
    if kind == "split3":
        img = ops.split3_kv(o["kv"], ops.transpose_v(o["kv"]))
        return ops.attn_split3(o["q"], img, p.Ns, o["fcs"], o["mu"], o["rs"], o["vmu"])
    if kind == "cosmom":
        mom = ops.cosine_moments(o["kv"], ops.transpose_v(o["kv"]))
        return ops.cosine_attn(o["q"], mom, o["fcs"], o["mu"], o["rs"], o["vmu"])
    if kind == "hd":
        return ops.attn_hd(o["q"], o["kv"], o["fcs"], o["mu"], o["rs"], o["vmu"], act)
    return ops.loss_attn(o["q"], o["k"], o["v"], o["fcs"], o["mu"], o["rs"], act)


def run_guarded(fm, p, o):
    """The C entries on NaN-guarded buffers.  Returns (first output, second output) after the guard and
    side-output checks."""
    kind, act, dt = fm["kind"], fm["act"], fm["dt"]
    B, Nc, Ns, D, Dv = p.B, p.Nc, p.Ns, p.Dqk, p.Dv
    Hh = p.H
    C = Hh * Dv
    dtc = ops.dt_code(dt)
    what = fm["name"] + " " + p.name
    ldt = ceil64(Ns)
    fcs = NanBuf(F32, (B, Nc, C), o["fcs"])
    odt = F32 if kind in ("split3", "loss") else dt
    out = NanBuf(odt, (B * Nc, C), pad=GUARD * C)
    ins = [fcs]
    if kind == "loss":
        q, k, v = NanBuf(F32, o["q"].shape, o["q"]), NanBuf(F32, o["k"].shape, o["k"]), NanBuf(F32, o["v"].shape, o["v"])
        ins += [q, k, v]
    else:
        q, kv = NanBuf(dt, o["q"].shape, o["q"]), NanBuf(dt, o["kv"].shape, o["kv"])
        ins += [q, kv]
    images = []
    if kind in ("attn", "split3", "cosmom"):
        vt = NanBuf(dt, (B, Hh, 128, ldt))
        call("mhada_transpose_v", kv.ptr, vt.ptr, dtc, B, Hh, Ns)
        images.append(("vt", vt))
    if kind == "split3":
        img = NanBuf(BF16, (B, Hh, 576 * ldt))
        call("mhada_split3_kv", kv.ptr, vt.ptr, img.ptr, B, Hh, Ns)
        images.append(("img", img))
    if kind == "cosmom":
        splits = fm["splits"] or wrapper_splits(B, Ns)
        mom = NanBuf(F32, (B, Hh, 65, 132))
        work = NanBuf(F32, (splits, B * Hh * 65 * 132)) if splits > 1 else None
        call("mhada_cosine_moments", kv.ptr, vt.ptr, dtc, B, Hh, Ns, mom.ptr, work.ptr if work else None, splits)
        images.append(("mom", mom))
        if work:
            images.append(("work", work))

    def attention():
        if kind == "attn":
            call("mhada_attn", q.ptr, kv.ptr, vt.ptr, fcs.ptr, o["mu"].data_ptr(), o["rs"].data_ptr(), o["vmu"].data_ptr(),
                 out.ptr, dtc, B, Hh, Nc, Ns, act)
        elif kind == "split3":
            call("mhada_attn_split3", q.ptr, img.ptr, fcs.ptr, o["mu"].data_ptr(), o["rs"].data_ptr(), o["vmu"].data_ptr(),
                 out.ptr, B, Hh, Nc, Ns)
        elif kind == "cosmom":
            call("mhada_cosine_attn", q.ptr, mom.ptr, fcs.ptr, o["mu"].data_ptr(), o["rs"].data_ptr(), o["vmu"].data_ptr(),
                 out.ptr, dtc, B, Hh, Nc)
        elif kind == "hd":
            call("mhada_attn_hd", q.ptr, kv.ptr, fcs.ptr, o["mu"].data_ptr(), o["rs"].data_ptr(), o["vmu"].data_ptr(),
                 out.ptr, dtc, B, Hh, D, Nc, Ns, act)
        else:
            call("mhada_loss_attn", q.ptr, k.ptr, v.ptr, fcs.ptr, o["mu"].data_ptr(), o["rs"].data_ptr(), out.ptr, B, Nc, Ns,
                 D, Dv, act)
        torch.cuda.synchronize()
        assert out.guards_intact(), what + ": written outside the [B Nc][C] output"
        y = out.t.clone()
        assert bool(torch.isfinite(y.float()).all()), what + ": an output element not written, or not finite"
        return y.view(B, Nc, C)

    first = attention()
    out.flat.copy_(nan_fill(out.flat.numel(), odt))
    second = attention()
    for b in ins:
        assert b.guards_intact(), what + ": an input buffer was written"
    # side outputs
    for name, b in images:
        assert b.guards_intact(), what + f": {name} written outside its image"
        if name != "work":
            assert bool(torch.isfinite(b.t.float()).all()), what + f": {name} not fully written"
    pos = pad_positions(Ns, dt)
    if kind in ("attn", "split3", "cosmom"):
        assert bool((vt.t[..., pos] == 0).all()), what + ": vt positions Ns .. ldt - 1 not zero"
        assert torch.equal(vt.t, ops.transpose_v(o["kv"])), what + ": vt differs from the wrapper's"
    if kind == "split3":
        im = img.t.view(B, Hh, 576 * ldt)
        kpl = im[..., :3 * ldt * 64].view(B, Hh, 3, ldt, 64)
        vpl = im[..., 3 * ldt * 64:].view(B, Hh, 3, 128, ldt)
        assert bool((kpl[..., Ns:, :] == 0).all()), what + ": split3 K rows past Ns not zero"
        assert bool((vpl[..., pad_positions(Ns, BF16)] == 0).all()), what + ": split3 V' positions past Ns not zero"
    if kind == "cosmom":
        assert bool((mom.t[..., 64, 128] == Ns).all()), what + ": mom[64][128] != Ns"
        assert bool((mom.t[..., 129:] == 0).all()), what + ": mom padding columns not zero"
    return first, second


def check(fm, shape):
    probes = P.SOFTMAX_PROBES if fm["act"] == SOFTMAX else P.COSINE_PROBES
    worst = 0.0
    for spec in probes:
        p, ref, bound = probe_and_reference(shape, fm, spec)
        o = operands(fm, p)
        what = f"{fm['name']} {shape} {p.name}"
        with _lib.tuning(**fm["knobs"]):
            y = run_wrappers(fm, p, o) if not fm["splits"] else None
            first, second = run_guarded(fm, p, o)
        torch.cuda.synchronize()
        assert torch.equal(first, second), what + ": a second call returned other bits"
        if y is not None:
            assert torch.equal(y, first), what + ": the C entry on guarded buffers differs from the ops wrapper"
        ratio = ((first.double() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        print(f"RATIO {fm['name']:28s} {'x'.join(map(str, shape)):12s} {p.name:24s} {ratio:.4f}")
        assert ratio <= 1.0, what + f": error / bound = {ratio:.3f}"
    return worst


@pytest.mark.parametrize("fm,shape", CASES)
def test_form(fm, shape):
    worst = check(fm, shape)
    print(f"BOUND {fm['name']:28s} {fm['kernel']:60s} {'x'.join(map(str, shape)):12s} worst error/bound = {worst:.4f}")


def test_zz_knobs_are_back_at_their_defaults():
    """Last in the module: every tuning() context above restored its knobs."""
    for k, v in DEFAULT_KNOBS.items():
        assert _lib.get_tuning(k) == v, k
