"""The premises of tests/test_gpu_wino_forms.py, checked without a GPU on its own form tables and operand
generators, so that the GPU file cannot pass because its reference drifted:

  * every exact case: the reference is its own fp32 rounding, the operands and both transforms are integers,
    the absolute-value Winograd sum stays below 2^24, and the Winograd evaluation A^T [(G g G^T) . (B^T d B)] A
    in fp64 is the F.conv2d reference (the sum S bounds the arithmetic the kernels actually perform);
  * every SPLIT3 plane case: the budget, the plane occupancy and the zero dropped products (asserted in
    plane_problem), and an fp64 emulation of the SPLIT3 product from the three host-side planes: as specified
    it returns the reference exactly; with plane 2 dropped, plane 1 dropped, or any one of the six kept cross
    products dropped it returns something else in the case that names that plane or product;
  * the weight-gradient cases: the same budget and rounding premises, and the split counts of the table.
"""
import pytest
import torch

import test_gpu_wino_forms as WF

PROBLEMS = sorted({(fm["grid"], fm["pad"], fm["Ci"], fm["Co"]) for fm in (p.values[0] for p in WF.FORMS)})


def test_tables_name_every_route_and_kernel():
    names = [p.values[0]["name"] for p in WF.FORMS]
    assert len(names) == len(set(names))
    for route, r in WF.ROUTES.items():
        mine = [p.values[0] for p in WF.FORMS if p.values[0]["route"] == route]
        assert {fm["kernel"] for fm in mine} == {r["kernel"]}
        assert {fm["grid"] for fm in mine} >= set(WF.GRIDS) and {fm["pad"] for fm in mine} == set(WF.PADS)
        assert {fm["Co"] for fm in mine} == {64, 128}
        cins = {fm["Ci"] for fm in mine}
        assert cins >= {16, 32, 48, 64, 256} and (r["planes"] or cins >= {8, 24})
        assert all(fm["Ci"] % 16 == 0 for fm in mine) or not r["planes"]
    assert {r["kernel"] for r in WF.ROUTES.values()} == {"wino_kernel", "wino4_kernel", "wino_s3_kernel"}


@pytest.mark.parametrize("grid,pad,Ci,Co", PROBLEMS, ids=lambda v: str(v).replace(" ", ""))
def test_exact_case_premises(grid, pad, Ci, Co):
    pb = WF.problem(grid, pad, Ci, Co, True)
    pb.exact_premises()
    assert torch.equal(WF.y_of(pb.V, pb.U, WF.AT, pb.Ho, pb.Wo), pb.base)
    assert bool((pb.S >= pb.base.abs()).all())
    assert pb.x.abs().max() <= 4 and set(pb.w.unique().tolist()) <= {-8.0, -4.0, 0.0, 4.0, 8.0}
    # integer planes below 256: the SPLIT3 route sees them in plane 0 alone, every kept product exact
    if Ci % 16 == 0:
        assert pb.V.abs().max() <= 256 and pb.U.abs().max() <= 256
    print(f"S max {pb.S.max().item():.0f} (2^24 = {2 ** 24})")


@pytest.mark.parametrize("grid,pad,Ci,Co", PROBLEMS[::7], ids=lambda v: str(v).replace(" ", ""))
def test_bound_case_operands_are_fp32_values(grid, pad, Ci, Co):
    pb = WF.problem(grid, pad, Ci, Co, False)  # (Problem asserts it of x, w and bias)
    assert bool((pb.S + 1e-300 >= pb.base.abs() * (1 - 1e-12)).all())
    assert WF.gamma(6 * Ci + 12) < 1e-3


# which plane case must notice which loss: (dropped V planes, dropped U planes, dropped products)
MUTANTS = {
    "V plane 2": dict(case="v3", v=(2,)), "U plane 2": dict(case="u3", u=(2,)),
    "V plane 1": dict(case="v2", v=(1,)), "U plane 1": dict(case="u2", u=(1,)),
    "v1 u1": dict(case="v2u2", drop=(1, 1)), "v2 u0": dict(case="v3", drop=(2, 0)), "v0 u2": dict(case="u3", drop=(0, 2)),
    "v1 u0": dict(case="v2", drop=(1, 0)), "v0 u1": dict(case="u2", drop=(0, 1)), "v0 u0": dict(case="v2", drop=(0, 0)),
}


@pytest.mark.parametrize("Ci", [16, 32, 48])
@pytest.mark.parametrize("case", list(WF.PLANE_CASES))
def test_plane_case_premises_and_emulation(case, Ci):
    pb, Vp, Up, q = WF.plane_problem(case, Ci)  # budget, occupancy, zero dropped products: asserted inside
    assert torch.equal(WF.split3_emulate(Vp, Up, pb.Ho, pb.Wo), pb.base)  # the kernel as specified is exact
    zero = torch.zeros_like
    for name, m in MUTANTS.items():
        if m["case"] != case:
            continue
        V = [zero(p) if i in m.get("v", ()) else p for i, p in enumerate(Vp)]
        U = [zero(p) if i in m.get("u", ()) else p for i, p in enumerate(Up)]
        kept = tuple(t for t in WF.KEPT if t != m.get("drop"))
        bad = WF.split3_emulate(V, U, pb.Ho, pb.Wo, kept)
        wrong = (bad.float() != pb.base.float()).double().mean().item()
        print(f"{case} Cin {Ci}: without {name} {100 * wrong:.1f} % of the outputs differ")
        assert wrong > 0, name
    print(f"sum / q = {pb.Sq:.3g} (2^24 = {2 ** 24:.3g}); shares V {pb.shares['V']} U {pb.shares['U']}")


def test_every_plane_and_product_has_a_case():
    assert {m["case"] for m in MUTANTS.values()} <= set(WF.PLANE_CASES)
    assert {m["drop"] for m in MUTANTS.values() if "drop" in m} == set(WF.KEPT)
    assert len(WF.KEPT) == 6 and all(i + j <= 2 for i, j in WF.KEPT)


@pytest.mark.parametrize("fm", WF.WG_FORMS)
def test_wgrad_case_premises(fm):
    pb = WF.wg_problem(fm["grid"], fm["zero"], fm["Ci"], fm["Co"], True)
    WF.wg_exact_premises(pb)
    assert pb.x.abs().max() <= 2 and pb.g.abs().max() <= 2
    assert bool((pb.Sw >= pb.dw.abs()).all()) and bool((pb.Sb >= pb.db.abs()).all())
    B, H, W = fm["grid"]
    nchunk = B * (H // 2) * (W // 16)
    assert nchunk == {(1, 2, 16): 1, (2, 16, 32): 32, (1, 20, 80): 50}[fm["grid"]]
    # the wrapper's split rule (csrc/wino.hip): at least 16 chunks per split, about 512 workgroups
    blocks = (fm["Ci"] // 64) * (fm["Co"] // 64)
    S = 1 if fm["one_slab"] else max(1, min(-(-512 // blocks), nchunk // 16))
    cps = -(-nchunk // S)
    assert -(-nchunk // cps) == fm["S"]
    assert pb.n + 9 >= pb.n // 4 + fm["S"] + 9  # the depth the bound assumes covers tiles + slabs + transforms


def test_prepack_bound_is_what_the_fp32_transform_needs():
    """The filter transform in fp32 with the kernel's association stays inside gamma_4 |G| |g| |G|^T, and does
    not stay inside 2 ulp of the result (cancellation), which is why the GPU test states the former."""
    pb = WF.problem((1, 2, 2), ("reflect", 1), 48, 128, False)
    g = pb.w.float()
    a, b, c = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    gg = torch.stack([a, 0.5 * (a + b + c), 0.5 * (a - b + c), c], 2)
    a, b, c = gg[..., 0], gg[..., 1], gg[..., 2]
    u = torch.stack([a, 0.5 * (a + b + c), 0.5 * (a - b + c), c], 3).double()
    err = (u - pb.U).abs()
    assert bool((err <= WF.gamma(4) * WF.u_of(pb.w.abs(), WF.G.abs())).all())
    ulp = torch.exp2(torch.floor(torch.log2(pb.U.abs().clamp_min(2.0 ** -126))) - 23)
    assert (err / ulp).max().item() > 2
