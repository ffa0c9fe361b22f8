"""The library calls of the Python host path, against tests/golden/host_trace.json.

The golden was recorded by tools/record_host_trace.py on the commit before the host path's twins (head width,
shared style, plane output) were folded into single bodies, and is committed unchanged: every route below must
launch the same entry points, in the same order, with the same scalars (integers, floats by their bits, every
field of a GemmArgs), device addresses aside.  Which buffer a pointer names is what the numerical suites check.

Cases (tools/record_host_trace.py, shared with the recorder): heads 4, 8, 16 x softmax, cosine x fp32, bf16,
each as a matched batch of 2 without the style cache, the same input twice with it (build, hit) and a 3-frame
clip against one style; the planes + SPLIT3 out-projection route at 8 heads fp32 softmax under ops.route_as;
MHAdaAttnFn forward + backward at D = 32, 64, 128 x Ns = 35, 36 x with and without k / v gradients;
MHAdaAttnBf16Fn at D = 64.
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_host_trace", os.path.join(REPO, "tools", "record_host_trace.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

_GOLDEN = {}


def golden_trace(name):
    if not _GOLDEN:
        _GOLDEN.update(rec.load_golden())
    return _GOLDEN[name]


def test_golden_holds_exactly_the_cases():
    if not _GOLDEN:
        _GOLDEN.update(rec.load_golden())
    assert sorted(_GOLDEN) == sorted(rec.CASES)
    assert all(len(t) > 0 for t in _GOLDEN.values())


@pytest.mark.parametrize("name", list(rec.CASES))
def test_host_path_makes_the_recorded_calls(name):
    want = golden_trace(name)
    got = rec.run_case(name)
    if name.endswith("-planes"):  # the case must not quietly fall back to the fp32 out-projection
        assert any(c[0] == "mhada_attn_split3_planes" for c in got)
    names = [c[0] for c in got]
    assert names == [c[0] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i} ({g[0]}) differs"
    assert len(got) == len(want)
