"""Frames/s of VideoStylizer.stylize_clip against the per-frame loop over stylize_u8, in one process.

    python tools/clip_throughput.py [--hw 256x512] [--style 256] [--T 1,2,4,8,16] [--rounds 7] [--dtypes fp32,bf16]
                                    [--heads 8] [--activation softmax]

Per dtype and T: `rounds` alternating rounds of (per-frame loop over T frames, the same loop again, one
stylize_clip(max_frames=T)), each timed with device events after one untimed warm-up round; prints the medians
with the min-max spread, the loop's A-against-A spread (its two timings in the same round), the ratio of the
medians, and the peak device memory of each route (above what is held before the call).  Frames are uint8
B,G,R [T][H][W][3]; the style is 256^2.  Seeded weights (mhada_hip.recipe), so the numbers are reproducible
without a checkpoint.  --heads 4 | 8 | 16 (head widths 128 / 64 / 32, the ViTs built with the same head count)
and --activation softmax | cosine choose the model family; the defaults are the 8-head softmax model.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "mhada-style-transfer_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import network  # noqa: E402
from mhada_hip.recipe import load_recipe, seeded_image  # noqa: E402
from mhada_hip.video import VideoStylizer  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", default="256x512")
    ap.add_argument("--style", type=int, default=256)
    ap.add_argument("--T", default="1,2,4,8,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--heads", type=int, default=8, choices=(4, 8, 16))
    ap.add_argument("--activation", default="softmax", choices=("softmax", "cosine"))
    ap.add_argument("--no-clip", action="store_true", help="the per-frame loop alone (a tree without stylize_clip)")
    ap.add_argument("--clip-only", action="store_true", help="the clip call alone, untimed rounds (under a kernel trace)")
    a = ap.parse_args()
    H, W = map(int, a.hw.split("x"))
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; frames {H}x{W} u8, style {a.style}^2, {a.rounds} rounds; ms per call")
    default = a.heads == 8 and a.activation == "softmax"
    if not default:
        print(f"# model: {a.heads} heads (head width {512 // a.heads}), {a.activation}")
    kw = {} if default else dict(num_heads=a.heads)
    akw = {} if default else dict(num_heads=a.heads, activation=a.activation)
    for dn in a.dtypes.split(","):
        dt = dict(fp32=torch.float32, bf16=torch.bfloat16)[dn]
        vc = load_recipe(network.VisionTransformer(pos_embedding=True, **kw), "vit_c").to(dev).eval()
        vs = load_recipe(network.VisionTransformer(pos_embedding=False, **kw), "vit_s").to(dev).eval()
        ada = load_recipe(network.AdaAttnTransformerMultiHead(**akw), "ada").to(dev).eval()
        for m in (vc, vs, ada):
            m.compute_dtype = dt
        st = VideoStylizer(vc, vs, ada)
        st.set_style(seeded_image(1, a.style, a.style, 2).to(dev))
        if not default:
            print(f"# {dn}: clip route {'on' if st._clip_route(torch.empty(0, device=dev)) else 'off (per-frame loop)'}")
        for T in map(int, a.T.split(",")):
            g = torch.Generator().manual_seed(T)
            u8 = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            f32 = [x.unsqueeze(0) for x in u8.flip(-1).permute(0, 3, 1, 2).float().contiguous()]

            def loop():
                for x in f32:
                    st.stylize_u8(x)

            def clip():
                st.stylize_clip(u8, max_frames=T)

            if a.clip_only:
                for _ in range(a.rounds):
                    clip()
                torch.cuda.synchronize()
                continue
            runs = [loop, loop] if a.no_clip else [loop, loop, clip]
            for fn in runs:
                fn()
            torch.cuda.synchronize()
            ts = [[] for _ in runs]
            for _ in range(a.rounds):
                for i, fn in enumerate(runs):
                    ts[i].append(timed(fn))
            med = [statistics.median(t) for t in ts]
            aa = max(abs(x - y) for x, y in zip(ts[0], ts[1]))
            line = (f"{dn} T={T:2d} loop {med[0]:8.2f} [{min(ts[0]):.2f}-{max(ts[0]):.2f}] = {1e3 * T / med[0]:7.1f} f/s "
                    f"(A-A spread {aa:.2f} ms, peak {peak(loop):.0f} MiB)")
            if not a.no_clip:
                line += (f" | clip {med[2]:8.2f} [{min(ts[2]):.2f}-{max(ts[2]):.2f}] = {1e3 * T / med[2]:7.1f} f/s "
                         f"(peak {peak(clip):.0f} MiB) | clip/loop frames/s x{med[0] / med[2]:.2f}")
            print(line, flush=True)


if __name__ == "__main__":
    main()
