"""The library calls the Python host path makes, case by case, and the golden file of them.

    python tools/record_host_trace.py [out.json]      (default: tests/golden/host_trace.json)

tests/test_gpu_host_trace.py replays the same cases (``CASES``) and compares.  The golden is recorded on the
commit BEFORE a change to the host code (mhada_hip/engine.py, ops.py, autograd_path.py) and committed
unchanged with it: the change then provably launches the same entry points, in the same order, with the
same scalars.

``trace(fn)`` swaps ``ops._call`` for a recorder that notes the call and passes it on.  Per call: the entry
point's name and its arguments — integers as they are, floats as ``float.hex``, the structure behind a
``ctypes.byref`` as the list of its fields.  Device addresses become "ptr" (None stays None): every integer at
or above 2^32 counts as one, and no size or stride of these cases comes near that.  So the trace pins the
order, the entry points and every scalar, not which buffer a pointer names; the numerical suites do that.

Every case runs twice and the second run is recorded: the first fills the per-module weight preparations
(engine.cached_prep and the lazily built SPLIT3 / HALF2 weights), whose launches happen once per module, so a
case's trace does not depend on which cases ran before it.  Cases reset what they depend on themselves (a new
VideoStylizer, new style features, ``cache_style``).

File format: {"calls": [unique call, ...], "cases": {name: [index into calls, ...]}} — the forwards of the 12
models repeat most calls, and the file stays small.
"""
import ctypes
import functools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "mhada-style-transfer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "host_trace.json")
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
PLANES_ROUTE = (256, 1)  # case "planes": B Nc = 192 rows count as 49152, 192 x 2 SPLIT3 tiles for 256 CUs


def _canon(v):
    if v is None:
        return None
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, int):
        return "ptr" if v >= 1 << 32 else int(v)
    obj = getattr(v, "_obj", None)  # ctypes.byref(structure)
    if isinstance(obj, ctypes.Structure):
        return {type(obj).__name__: [_canon(getattr(obj, f[0])) for f in obj._fields_]}
    if isinstance(v, ctypes.Array):
        return [_canon(x) for x in v]
    raise TypeError(f"record_host_trace: an argument of type {type(v).__name__}")


def trace(fn):
    """The calls fn() makes through ops._call, canonicalised."""
    from mhada_hip import ops
    real, calls = ops._call, []

    def recorder(name, dev_tensor, *args):
        calls.append([name] + [_canon(a) for a in args])
        return real(name, dev_tensor, *args)

    ops._call = recorder
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops._call = real
    return calls


@functools.lru_cache(maxsize=None)
def models(heads, act, dtype):
    """As tests/test_gpu_clip_forms.py builds them."""
    import network
    from mhada_hip.recipe import load_recipe
    vc = load_recipe(network.VisionTransformer(pos_embedding=True, num_heads=heads), "vit_c").to(DEV).eval()
    vs = load_recipe(network.VisionTransformer(pos_embedding=False, num_heads=heads), "vit_s").to(DEV).eval()
    ada = load_recipe(network.AdaAttnTransformerMultiHead(num_heads=heads, activation=act), "ada").to(DEV).eval()
    for m in (vc, vs, ada):
        m.compute_dtype = DTYPES[dtype]
    return vc, vs, ada


def _images(batch):
    from mhada_hip.recipe import seeded_image
    content = torch.cat([seeded_image(1, 64, 96, 11 + i) for i in range(batch)]).to(DEV)  # Nc = 96
    style = torch.cat([seeded_image(1, 40, 56, 2 + i) for i in range(batch)]).to(DEV)     # Ns = 35
    return content, style


def case_batch(heads, act, dtype):
    """(a) a matched batch of 2, the per-style cache off."""
    vc, vs, ada = models(heads, act, dtype)
    c, s = _images(2)
    ada.cache_style = False
    try:
        with torch.no_grad():
            ada(vc(c), vs(s))
    finally:
        del ada.cache_style


def case_cache(heads, act, dtype):
    """(b) the same input twice with the cache on: build, then hit."""
    vc, vs, ada = models(heads, act, dtype)
    c, s = _images(2)
    ada.__dict__.pop("_mhada_style", None)
    with torch.no_grad():
        fs = vs(s)
        ada(vc(c), fs)
        ada(vc(c), fs)


def case_clip(heads, act, dtype):
    """(c) a clip of 3 frames against one style: the shared-style entries, the grouped batch-axis attention."""
    from mhada_hip.video import VideoStylizer
    c, s = _images(3)
    st = VideoStylizer(*models(heads, act, dtype))
    st.set_style(s[:1])
    st.stylize_clip(c, u8=False, max_frames=3)


def case_planes():
    """(d) 8 heads, fp32 softmax, routed as a batch large enough for the SPLIT3 out-projections: the attention
    writes bf16 planes (mhada_attn_split3_planes) and out_conv is a SPLIT3 GEMM."""
    from mhada_hip import engine, ops
    vc, vs, ada = models(8, "softmax", "fp32")
    c, s = _images(2)
    ada.cache_style = False
    try:
        with torch.no_grad(), ops.route_as(*PLANES_ROUTE):
            assert engine._split3_fills(2 * 96, 512, c.device), "PLANES_ROUTE does not fill this device"
            ada(vc(c), vs(s))
    finally:
        del ada.cache_style


def _train_inputs(D, Ns, kv_grad, BH=4, Nc=96):
    g = torch.Generator(device="cpu").manual_seed(1000 * D + Ns)
    q, x = (torch.randn(BH, Nc, D, generator=g).to(DEV) for _ in range(2))
    k, v = (torch.randn(BH, Ns, D, generator=g).to(DEV) for _ in range(2))
    q.requires_grad_(True)
    x.requires_grad_(True)
    k.requires_grad_(kv_grad)
    v.requires_grad_(kv_grad)
    return q, k, v, x


def case_train(D, Ns, kv_grad):
    """(e) MHAdaAttnFn forward and backward; without k / v gradients the dQ-only kernels."""
    from mhada_hip import autograd_path
    autograd_path.MHAdaAttnFn.apply(*_train_inputs(D, Ns, kv_grad)).sum().backward()


def case_train_bf16():
    """(f) MHAdaAttnBf16Fn forward and backward at D = 64."""
    from mhada_hip import autograd_path
    autograd_path.MHAdaAttnBf16Fn.apply(*_train_inputs(64, 35, True)).sum().backward()


def _cases():
    out = {}
    for heads in (4, 8, 16):
        for act in ("softmax", "cosine"):
            for dtype in DTYPES:
                for kind, fn in (("batch", case_batch), ("cache", case_cache), ("clip", case_clip)):
                    out[f"h{heads}-{act}-{dtype}-{kind}"] = functools.partial(fn, heads, act, dtype)
    out["h8-softmax-fp32-planes"] = case_planes
    for D in (32, 64, 128):
        for Ns in (35, 36):  # at 64: 36 takes the dS spill, 35 the recompute
            for kv_grad in (True, False):
                out[f"train-d{D}-ns{Ns}-{'kv' if kv_grad else 'dq'}"] = functools.partial(case_train, D, Ns, kv_grad)
    out["train-bf16-d64"] = case_train_bf16
    return out


CASES = _cases()


def run_case(name):
    """The recorded trace of one case (its second run)."""
    fn = CASES[name]
    fn()
    return trace(fn)


def pack(traces):
    """{case: [call, ...]} -> the file format."""
    calls, index, cases = [], {}, {}
    for name, tr in traces.items():
        ids = []
        for call in tr:
            key = json.dumps(call)
            if key not in index:
                index[key] = len(calls)
                calls.append(call)
            ids.append(index[key])
        cases[name] = ids
    return {"calls": calls, "cases": cases}


def load_golden(path=GOLDEN):
    """The file -> {case: [call, ...]}."""
    with open(path) as f:
        packed = json.load(f)
    return {name: [packed["calls"][i] for i in ids] for name, ids in packed["cases"].items()}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    traces = {}
    for name in CASES:
        traces[name] = run_case(name)
        print(f"{name}: {len(traces[name])} calls", flush=True)
    packed = pack(traces)
    with open(out, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(packed['calls'])} distinct calls in {len(packed['cases'])} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
