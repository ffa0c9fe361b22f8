"""Timing of mhada_attn_hd (head widths 32 / 128, csrc/attn_hd.hip) against the D = 64, 8-head general
kernels of the same dtype in one process (same QK and PV FLOPs): interleaved rounds after a warm-up,
median per variant, the sustained-clock probe beside it; then the whole stylize call for 4, 8 and 16
heads.

    python tools/attn_hd_ab.py [--attn-only | --model-only]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

import network
from mhada_hip import _lib, ops
from mhada_hip.recipe import load_recipe, seeded_image

# (name, dtype, B, Nc = Ns): the attention shapes of the bench's two inference configs
SHAPES = [("512^2 B8 fp32", torch.float32, 8, 4096), ("1024^2 B4 bf16", torch.bfloat16, 4, 16384)]
ROUNDS, REPS = 7, 3


def operands(dt, B, H, D, n):
    sc = 0.35 * (64.0 / D) ** 0.25
    q = (torch.randn(B, H, n, D, device="cuda") * sc).to(dt)
    kv = (torch.randn(B, H, n, 2 * D, device="cuda") * sc).to(dt)
    fcs = torch.randn(B, n, 512, device="cuda")
    mu, rs = ops.instnorm_stats(fcs)
    return q, kv, fcs, mu, rs, torch.zeros(B, 512, device="cuda")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS


def attn_ab():
    torch.manual_seed(0)
    for name, dt, B, n in SHAPES:
        runs = {}
        q, kv, fcs, mu, rs, vmu = operands(dt, B, 8, 64, n)
        vt = ops.transpose_v(kv)
        # the yardstick: attn_f32_kernel (fp32) / the online-max attn_bf16_kernel (attn_fixed_shift = 0)
        runs["D64 H8 general"] = lambda a=(q, kv, vt, fcs, mu, rs, vmu): ops.mhada_attn(*a, 0)
        for H, D in ((4, 128), (16, 32)):
            a = operands(dt, B, H, D, n)
            runs[f"D{D} H{H} attn_hd"] = lambda a=a: ops.attn_hd(*a, 0)
        with _lib.tuning(attn_fixed_shift=0):
            for fn in runs.values():  # warm-up
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for k, fn in runs.items():
                    times[k].append(timed(fn))
        med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
        base = med["D64 H8 general"]
        fl = 6.0 * n * n * 512 * B
        print(f"{name}: " + "   ".join(f"{k} {t:.3f} ms ({fl / t / 1e9:.0f} TF, x{t / base:.2f})" for k, t in med.items()),
              flush=True)


def model_time():
    for name, dt, B, side in (("512^2 B8 fp32", torch.float32, 8, 512), ("1024^2 B4 bf16", torch.bfloat16, 4, 1024)):
        c = seeded_image(B, side, side, 1).cuda()
        s = seeded_image(B, side, side, 2).cuda()
        out = []
        for heads in (4, 8, 16):
            vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").cuda().eval()
            vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").cuda().eval()
            ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads), "ada").cuda().eval()
            for m in (vc, vs, ada):
                m.compute_dtype = dt
            ada.cache_style = False

            def call():
                with torch.no_grad():
                    ada(vc(c), vs(s))
            call()
            call()
            torch.cuda.synchronize()
            ts = sorted(timed(call) for _ in range(5))
            out.append(f"{heads} heads {ts[2]:.2f} ms")
        print(f"stylize {name}: " + "   ".join(out), flush=True)


def clock(launches=20, iters=150000):
    """The sustained shader clock under dense bf16 MFMA load right after the timed region
    (mhada_clock_probe, as bench.py's shader_clock)."""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    buf = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(launches):
        _lib.check(_lib.load().mhada_clock_probe(buf.data_ptr(), n, iters, st), "mhada_clock_probe")
    torch.cuda.synchronize()
    v = buf.view(n, 2).double().cpu()
    ghz = (v[:, 0] / v[:, 1].clamp(min=1) * 0.1).sort().values
    print(f"clock probe: {float(ghz[n // 2]):.3f} GHz", flush=True)


if __name__ == "__main__":
    clock()
    if "--model-only" not in sys.argv:
        attn_ab()
    clock()
    if "--attn-only" not in sys.argv:
        model_time()
