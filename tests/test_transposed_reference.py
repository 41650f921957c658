"""The float64 restatement of the transposed sparse passes (gj_testlib.sparse_passes_fp64) - what the GPU tests of
tests/test_gpu_transposed_passes.py compare the kernels with - pinned to the oracle: its `out` must be the gradient that
torch.autograd computes through the oracle's own `infection_network`, and its forward form the oracle's forward."""
import numpy as np
import pytest
import torch

import gj_oracle as O
import gj_testlib as L


def signed_vector(n, seed, zeros=0.3):
    """Standard normal with ~30 % exact zeros, max |x| = 1 (float32)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    x[rng.random(n) < zeros] = 0.0
    return (x / np.abs(x).max()).astype(np.float32)


def june769_case(day_type, quarantine, seed=0):
    """The reference's 769-agent world with all eleven networks active, betas drawn in [0.1, 40] (float32 values) and -
    with ``quarantine`` - the stages recorded at step 7 of the trajectory under the threshold 4."""
    npz = L.load_npz("june769.npz")
    world, tables = L.world_from(npz), L.tables_from(npz)
    rng = np.random.default_rng(77 + seed)
    betas = {n: float(np.float32(rng.uniform(0.1, 40.0))) for n in L.HIERARCHY}
    stage = npz["step7/pre/current_stage"].astype(np.float32) if quarantine else None
    assert stage is None or 10 < int((stage >= 4).sum()) < 200
    return dict(world=world, tables=tables, active=list(L.HIERARCHY), betas=betas, day_type=day_type, stage=stage,
                q_thr=4.0 if quarantine else None)


def qmask_of(case):
    return None if case["stage"] is None else (case["stage"] < case["q_thr"]).astype(np.float64)


def oracle_ts(case, t, susc):
    """sum_n ts_n and {n: cum_n} through the oracle's functions in float64 (`people` as float64, so that p_contact and
    beta * p_contact are float64 too: every op of `infection_network` then follows the input dtype)."""
    world, total, cums = case["world"], 0.0, {}
    q = 1.0 if case["stage"] is None else O.quarantine_mask(torch.from_numpy(case["stage"]), [case["q_thr"]]).double()
    for name in case["active"]:
        es = world["edge_sets"][O.edge_set_of(name)]
        kind = O.network_kind(name)
        lp = None
        if kind in ("leisure", "care_visit"):
            lp = O.leisure_agent_probabilities(case["tables"][name], world["sex"], world["age"], case["day_type"]).double()
        ts, cum = O.infection_network(kind=kind, beta=case["betas"][name], people=es["people"].double(),
                                      agent_index=es["agent"], venue_index=es["venue"], transmission=t,
                                      susceptibility=susc, qmask=q, leisure_prob=lp, age=world["age"], return_cum=True)
        assert ts.dtype == torch.float64 and cum.dtype == torch.float64
        total = total + ts
        cums[name] = cum
    return total, cums


@pytest.mark.parametrize("quarantine", [False, True], ids=["no-quarantine", "quarantine"])
@pytest.mark.parametrize("day_type", [0, 1], ids=["weekday", "weekend"])
def test_restatement_is_the_gradient_autograd_takes_through_the_oracle(day_type, quarantine):
    """d <x, sum_n ts_n(t)> / d t by torch.autograd through the oracle in float64 == the restatement's `out` on x, for
    every agent within 1e-13 of the sum of the absolute values of its terms (float64 on both sides: only the order of
    the additions differs).  The forward form (transpose=False) equals the oracle's forward at the same bound."""
    case = june769_case(day_type, quarantine)
    A = case["world"]["n_agents"]
    x = signed_vector(A, seed=3)
    assert float((x == 0).mean()) > 0.2 and x.min() < 0 < x.max()
    t = torch.from_numpy(np.abs(signed_vector(A, seed=4)).astype(np.float64)).requires_grad_(True)
    ones = torch.ones(A, dtype=torch.float64)
    total, cums = oracle_ts(case, t, ones)
    (grad,) = torch.autograd.grad((torch.from_numpy(x.astype(np.float64)) * total).sum(), t)
    args = (case["world"], case["active"], case["betas"], case["tables"], day_type, qmask_of(case))
    ref = L.sparse_passes_fp64(*args, x, transpose=True, pc_float32=False)
    assert np.abs(ref["out"]).max() > 0
    assert (np.abs(grad.numpy() - ref["out"]) <= 1e-13 * ref["out_abs"]).all()
    # the transposed operator is not the forward one on this world (care_visit: the age > 75 factor changes sides)
    fwd_on_x = L.sparse_passes_fp64(*args, x, transpose=False, pc_float32=False)
    assert np.abs(fwd_on_x["out"] - ref["out"]).max() > 1e-6 * np.abs(ref["out"]).max()
    fwd = L.sparse_passes_fp64(*args, t.detach().numpy(), transpose=False, pc_float32=False)
    assert (np.abs(total.detach().numpy() - fwd["out"]) <= 1e-13 * fwd["out_abs"]).all()
    for n, cum in cums.items():
        assert (np.abs(cum.detach().numpy() - fwd["cum"][n]) <= 1e-13 * fwd["bp"][n] * fwd["cum_abs"][n]).all(), n
    # term counts: one per edge and network
    n_edges = sum(len(case["world"]["edge_sets"][L.edge_set_name(n)]["agent"]) for n in case["active"])
    assert int(ref["out_terms"].sum()) == n_edges == int(sum(c.sum() for c in ref["cum_terms"].values()))


def test_bounds_scale_with_a_power_of_two():
    """The bounds of x * 2^k through `scale = 2^k` are 2^k times those of x, and the float32 p_contact differs from the
    float64 one by at most one rounding."""
    case = june769_case(0, True)
    A = case["world"]["n_agents"]
    x = signed_vector(A, seed=3)
    args = (case["world"], case["active"], case["betas"], case["tables"], 0, qmask_of(case))
    one = L.sparse_passes_with_bounds(*args, x)
    big = L.sparse_passes_with_bounds(*args, x * np.float32(2.0 ** 17), scale=2.0 ** 17)
    assert np.array_equal(big["out"], one["out"] * 2.0 ** 17) and np.array_equal(big["out_bound"], one["out_bound"] * 2.0 ** 17)
    assert (one["out_bound"] > 0).any() and (one["out_bound"] <= 1e-5 * np.maximum(1e-12, np.abs(one["out"]).max())).all()
    exact, rounded = L.sparse_passes_fp64(*args, x, pc_float32=False), L.sparse_passes_fp64(*args, x)
    assert (np.abs(exact["out"] - rounded["out"]) <= L.U32 * rounded["out_abs"]).all()
