"""CPU: seeding by agent group - the numpy restatement of the seed and its adjoint (tests/gj_seed_ref.py) against torch
autograd and against the reference's records (tests/golden/grads_seed.npz, written by make_golden_seed.py), the
``infection_seed`` keys of the YAML schema, and the C declaration of gj_adjoint_seed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gj_seed_ref as R
import gj_testlib as L
from grad_june_amd import _native as N
from grad_june_amd.groups import seed_log_fractions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gradjune_hip.h")


# ---- the restatement's adjoint against torch autograd of the same formulas ---------------------------------------------
def _inputs(n, G, seed):
    rng = np.random.default_rng(seed)
    d = {"labels": rng.integers(0, G, n), "p_not": 1.0 - rng.uniform(0.03, 0.4, G),
         "e": rng.exponential(size=(2, n)), "susc0": np.where(rng.random(n) < 0.8, 1.0, rng.random(n)),
         "time0": rng.random(n), "now": 1.5}
    d["susc0"][:: 7] = 0.0
    for k in ("g_susc", "g_inf", "g_time", "g_new"):
        d[k] = rng.standard_normal(n)
    return d


@pytest.mark.parametrize("n,G", [(1, 1), (65, 2), (1003, 7), (300, 300)])
def test_restatement_adjoint_equals_autograd(n, G):
    d = _inputs(n, G, 5 + n)
    nu = R.decisions(d["p_not"][d["labels"]], d["e"][0], d["e"][1])
    got = R.seed_adjoint(d["p_not"], d["labels"], G, d["susc0"], d["time0"], d["now"], d["e"][0], d["e"][1], nu=nu,
                         **{k: d[k] for k in ("g_susc", "g_inf", "g_time", "g_new")})
    fraction = torch.tensor(1.0 - d["p_not"], dtype=torch.float64, requires_grad=True)
    p = (1.0 - fraction)[torch.from_numpy(d["labels"])]
    e = torch.from_numpy(d["e"])
    z0, z1 = (p.log() + (-e[0].log())) / 0.1, ((1.0 - p).log() + (-e[1].log())) / 0.1
    m = torch.maximum(z0, z1)
    x0, x1 = torch.exp(z0 - m), torch.exp(z1 - m)            # (the softmax op by op: torch.softmax's own backward
    y0 = x0 / (x0 + x1)                                      # cancels 1 - y0 where it saturates and is good to 1e-7 there)
    hard0 = torch.from_numpy(1.0 - nu)
    new = 1.0 - (hard0 - y0.detach() + y0)                          # straight-through, infection.py:13-18
    s0, t0 = torch.from_numpy(d["susc0"]), torch.from_numpy(d["time0"])
    susc = torch.maximum(torch.tensor(0.0, dtype=torch.float64), s0 - new)     # model.py:103-110
    inf = new
    time = t0 + new * (d["now"] - t0)
    loss = sum((torch.from_numpy(d[k]) * v).sum() for k, v in (("g_susc", susc), ("g_inf", inf), ("g_time", time),
                                                              ("g_new", new)))
    (ref,) = torch.autograd.grad(loss, fraction)
    assert np.all(got["abs_sum"][np.bincount(d["labels"], minlength=G) > 0] > 0)
    for g in range(G):
        assert got["grad_fraction"][g] == pytest.approx(float(ref[g]), rel=1e-9, abs=1e-300), g


def test_out_of_range_labels_contribute_nothing():
    d = _inputs(50, 3, 1)
    lab = d["labels"].copy()
    lab[[3, 17]] = [-1, 3]
    a = R.seed_adjoint(d["p_not"], lab, 3, d["susc0"], d["time0"], 1.5, d["e"][0], d["e"][1], g_inf=d["g_inf"],
                       g_time=d["g_time"])
    keep = np.ones(50, bool)
    keep[[3, 17]] = False
    b = R.seed_adjoint(d["p_not"], lab[keep], 3, d["susc0"][keep], d["time0"][keep], 1.5, d["e"][0][keep], d["e"][1][keep],
                       g_inf=d["g_inf"][keep], g_time=d["g_time"][keep])
    assert np.array_equal(a["grad_fraction"], b["grad_fraction"])
    assert a["nu"][3] == 0 and a["nu"][17] == 0 and a["grad_time"][3] == d["g_time"][3]


# ---- the restatement against the reference's records, the seed alone ----------------------------------------------------
@pytest.mark.parametrize("case", ["s1", "s2"])
def test_restatement_reproduces_the_recorded_seed(case):
    z = {k[len(case) + 1:]: v for k, v in L.load_npz("grads_seed.npz").items() if k.startswith(case + "/")}
    lf, lab, noise = z["seed/log_fraction"], z["seed/labels"], z["seed/exp_noise"]
    assert lf.shape == ((1,) if case == "s1" else (3,)) and np.bincount(lab).min() >= 20
    p_not = (1.0 - (10.0 ** torch.from_numpy(lf)).double()).float().numpy()     # as infect_fraction_by_group forms it
    nu, susc, inf, time = R.seed_forward(p_not, lab, z["seed/pre/susceptibility"], z["seed/pre/is_infected"],
                                         z["seed/pre/infection_time"], float(z["seed/now"]), noise[0], noise[1],
                                         dtype=np.float32)
    assert np.array_equal(nu, z["seed/new_infected"]) and nu.sum() >= 3
    assert np.array_equal(susc, z["state0/susceptibility"])
    assert np.array_equal(inf, z["state0/is_infected"])
    assert np.array_equal(time, z["state0/infection_time"])
    for tag in ("last", "series"):
        g = z[f"grad_{tag}/log_fraction"]
        assert g.shape == lf.shape and np.all(np.isfinite(g)) and np.all(g != 0)


# ---- infection_seed in the YAML schema -----------------------------------------------------------------------------------
def test_scalar_only_config_yields_no_labelling():
    assert seed_log_fractions({"log_fraction_initial_cases": -2.5}) == (None, -2.5)
    assert seed_log_fractions({"log_fraction_initial_cases": -2.5}, keys=["a", "b"]) == (None, -2.5)


def test_default_fills_the_groups_not_listed():
    by, lf = seed_log_fractions({"log_fraction_initial_cases": -2.5, "by": "area",
                                 "log_fraction_by_group": {"E02": -1.0, 7: -0.5}}, keys=["E01", "E02", 7, "E04"])
    assert by == "area" and lf.dtype == torch.float64            # the YAML's doubles, as the scalar seed reads them
    assert lf.tolist() == [-2.5, -1.0, -0.5, -2.5]
    by, lf = seed_log_fractions({"log_fraction_initial_cases": -3.0, "by": "area"}, keys=[0, 1, 2])
    assert lf.tolist() == [-3.0] * 3


def test_unknown_key_and_missing_attribute_raise():
    with pytest.raises(ValueError, match="E09"):
        seed_log_fractions({"log_fraction_initial_cases": -2.5, "by": "area", "log_fraction_by_group": {"E09": -1.0}},
                           keys=["E01", "E02"])
    with pytest.raises(ValueError, match="no such labelling"):
        seed_log_fractions({"log_fraction_initial_cases": -2.5, "by": "area"}, keys=None)
    with pytest.raises(ValueError, match="needs infection_seed.by"):
        seed_log_fractions({"log_fraction_initial_cases": -2.5, "log_fraction_by_group": {"E01": -1.0}})


def test_get_data_refuses_an_attribute_the_world_does_not_have(monkeypatch):
    from grad_june_amd import runner as RN
    from grad_june_amd.defaults import default_parameters

    monkeypatch.setattr(RN, "require_hip", lambda d: torch.device("cpu"))
    params = default_parameters("cpu")
    params["infection_seed"]["by"] = "no_such_attribute"
    with pytest.raises(ValueError, match="no_such_attribute"):
        RN.Runner.get_data(params)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_in_the_header_and_the_binding_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+gj_adjoint_seed\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "gj_adjoint_seed is not declared in the header"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    restype, argtypes = N.SYMBOLS["gj_adjoint_seed"]
    assert restype is C.c_int and len(argtypes) == len(declared) == 22
    for arg, ct in zip(declared, argtypes):
        if "gj_seed_plan" in arg:
            assert ct is C.POINTER(N.SeedPlan)
        elif "*" in arg:
            assert ct is C.c_void_p, arg
        else:
            assert ct is {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "float": C.c_float}[arg.split()[0]], arg
    assert N.GJ_ABI_VERSION == 7 and "#define GJ_ABI_VERSION 7" in src
    assert "#define GJ_SEED_CHUNK 1024" in src and N.GJ_SEED_CHUNK == 1024
    assert C.sizeof(N.SeedPlan) == 48


def test_argument_errors_come_before_any_device_work():
    lib = N.load()
    one = C.c_void_p(8)                                            # never dereferenced: the checks refuse first
    plan = N.SeedPlan(10, 1, 8, 8, 8, 8)

    def call(n=10, p=one, group=one, G=3, plan=C.byref(plan), susc=one, out=one, contrib=one, partial=one):
        return lib.gj_adjoint_seed(n, p, group, G, plan, susc, one, None, 0, 0, 0, 0.0, None, None, None, None, contrib,
                                   partial, out, None, None, None)

    assert call(n=-1) == -2 and call(G=0) == -2 and call(G=N.GJ_MAX_GROUPS + 1) == -2
    assert call(group=None, G=2) == -2                             # no labels: one group
    assert call(out=None) == -1 and call(plan=None) == -1
    assert call(p=None) == -1 and call(susc=None) == -1 and call(contrib=None) == -1 and call(partial=None) == -1
    bad = N.SeedPlan(11, 1, 8, 8, 8, 8)                            # more sorted agents than agents
    assert call(plan=C.byref(bad)) == -2
    bad = N.SeedPlan(10, 5, 8, 8, 8, 8)                            # more chunks than 10 agents in 3 groups can have
    assert call(plan=C.byref(bad)) == -2
