"""CPU: the fp64 reference of the transmission profile (tests/gj_profile_ref.py) and its allowance B are sound - the fp32
oracle (oracle.transmission_update, forward and torch autograd) stays within K_REF * B of it on the whole grid.

Measured on the CPU, maximum of err / (B * allowance) over the comparable points (734 of the 880 grid points - 16.6 %
excluded - and the finite edge and digamma points):
    forward 0.36, max_infectiousness 0.36, shape 0.73, rate 5.85, shift 0.40, infection_time 0.40, is_infected 0.36
(rate: autograd adds the pow's (shape - 1) / rate * T and the factor's T / rate, each ~50 times their sum at shape 0.02
with d = 1e-3; the kernel forms shape / rate - d directly).  K_REF = 6 is that maximum rounded up: the one constant
taken from a measurement, and the measurement is of the oracle, not of a kernel.  Off the comparable points (a factor
subnormal, overflowed or zero, d <= 0) the oracle is held to the same allowance plus the reference's floor, and to
the fp64 value's inf / NaN wherever fp32 did not overflow."""
import math

import pytest
import torch

import gj_profile_ref as R


@pytest.fixture(scope="module")
def pts():
    x, kinds = R.all_points()
    T32, g32 = R.oracle32(x)
    return {"x": x, "kinds": kinds, "ref": R.reference(x), "T32": T32, "g32": g32,
            "grid": torch.tensor([k == "grid" for k in kinds])}


def test_grid_is_the_issues_and_mostly_comparable(pts):
    grid = pts["grid"]
    assert int(grid.sum()) == len(R.SHAPES) * len(R.DS) * len(R.RATES) == 880
    excluded = grid & ~pts["ref"]["comparable"]
    share = float(excluded.sum()) / float(grid.sum())
    print(f"excluded from the relative comparison: {int(excluded.sum())} of {int(grid.sum())} = {share:.3f}")
    assert share < R.MAX_EXCLUDED_SHARE
    # every branch of inv_gamma, both sides of each boundary, and d on both sides of 0 (fp32 rounding of d = 1e-6)
    s = pts["x"]["shape"][grid & pts["ref"]["comparable"]]
    for lo, hi in ((0.0, 0.25), (0.25, 1.0), (1.0, 2.0), (2.0, 16.0), (16.0, 1e9)):
        assert bool(((s > lo) & (s < hi)).any())
    for edge in (0.25, 1.0, 2.0, 16.0):
        assert bool((s == edge).any())
    d = R.fp32_d(pts["x"], R.NOW)[grid]
    assert bool((d == 0).any()) and bool((d < 0).any())


def test_fp32_oracle_within_k_ref_of_the_reference(pts):
    ref, c = pts["ref"], pts["ref"]["comparable"]
    q, placed = R.check_forward(pts["T32"], ref, pts["T32"])
    assert bool(placed.all())                                  # (the oracle is finite on every comparable point)
    measured = {"forward": R.worst(torch.where(c, q, torch.zeros_like(q)))[0]}
    off = {"forward": R.worst(torch.where(c, torch.zeros_like(q), q))[0]}
    scope = R.partial_scope(pts["kinds"], pts["T32"])
    assert bool(scope[c].all())
    for k in R.FIELDS:
        q, placed = R.check_partial(k, pts["g32"][k], ref, scope)
        assert bool(placed.all()), (k, torch.nonzero(~placed).flatten().tolist())
        measured[k] = R.worst(torch.where(c, q, torch.zeros_like(q)))[0]
        off[k] = R.worst(torch.where(c, torch.zeros_like(q), q))[0]
    print("oracle, max err / (B * allowance), comparable points:", {k: round(v, 2) for k, v in measured.items()})
    print("oracle, the same with the floor, other points:      ", {k: round(v, 2) for k, v in off.items()})
    k_ref = max(measured.values())
    print(f"K_ref measured {k_ref:.2f}, asserted {R.K_REF}")
    assert k_ref <= R.K_REF and max(off.values()) <= R.K_REF
    assert math.ceil(k_ref) == R.K_REF       # the constant is the measurement rounded up, not a looser one


def test_oracle_has_the_references_inf_and_nan_at_the_edge_points(pts):
    """d <= 0, max_infectiousness 0, is_infected 2 and the digamma points: no fp32 overflow, so the oracle's inf / NaN are
    the fp64 value's, in the forward and (outside the forward-only kinds) in every partial."""
    ref, edge = pts["ref"], ~pts["grid"]
    assert torch.equal(R.placement(pts["T32"])[edge], R.placement(ref["T"])[edge])
    keep = edge & torch.tensor([k not in R.FORWARD_ONLY_KINDS for k in pts["kinds"]])
    for k in R.FIELDS:
        assert torch.equal(R.placement(pts["g32"][k])[keep], R.placement(ref["partial"][k])[keep]), k
    nan_shape = torch.isnan(ref["partial"]["shape"])
    for kind, want in (("neg_int", True), ("d0_int", False), ("mx0", False), ("inf2", False)):
        m = torch.tensor([k == kind for k in pts["kinds"]])
        assert bool((nan_shape[m] == want).all()), kind
    dg = torch.tensor([k == "digamma" for k in pts["kinds"]])
    poles = dg & ((pts["x"]["shape"] == -1.0) | (pts["x"]["shape"] == -2.0) | (pts["x"]["shape"] == 0.0))
    assert torch.equal(nan_shape[dg], poles[dg])


def test_d_zero_with_integer_shape_is_finite_in_autograd(pts):
    """t == shift exactly, shape 1, 2, 3, 4, rate 0.53, max_infectiousness 1.3: d/d infection_time = d/d shift =
    +r T, -r^2 max_inf, 0, 0."""
    m = torch.tensor([k == "d0_int" for k in pts["kinds"]])
    assert pts["x"]["shape"][m].tolist() == [1.0, 2.0, 3.0, 4.0]
    want = torch.tensor([0.36517, -0.36517, 0.0, 0.0], dtype=torch.float64)
    for k in ("infection_time", "shift"):
        for v in (pts["ref"]["partial"][k][m], pts["g32"][k][m].double()):
            assert torch.allclose(v, want, rtol=0.0, atol=5e-6), (k, v)
