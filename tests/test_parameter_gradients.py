"""CPU: gradients w.r.t. the transmission-profile parameters - the oracle's autograd against the reference's recorded
gradients (tests/golden/grads_params.npz, written by make_golden_params.py), the C entry's argument contract (no launch
is made: the checks come first) and the detection that puts a run on the autograd graph."""
import ctypes

import numpy as np
import pytest
import torch

from grad_june_amd import _native as N

PROFILE_KEYS = ("max_infectiousness", "shape", "rate", "shift")


def _load():
    import importlib.util
    import os

    if not os.path.exists(N.LIB_PATH):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(root, "__graft_entry__.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        m.build()
    return N.load()


def test_abi_7_exports_the_profile_adjoint():
    lib = _load()
    assert N.GJ_ABI_VERSION == 7 and lib.gj_version() == 7
    assert "gj_adjoint_transmission_params" in N.SYMBOLS
    assert hasattr(lib, "gj_adjoint_transmission_params")


def test_profile_adjoint_argument_contract():
    """n < 0: range error; n == 0: nothing to do; a missing required pointer: NULL error - all before any launch.
    The four parameter outputs are optional (NULL = not computed)."""
    lib = _load()
    st = N.AgentState()
    f = lib.gj_adjoint_transmission_params
    OK, E_NULL, E_RANGE = 0, -1, -2                    # include/gradjune_hip.h
    fake = 0x1000                                        # never dereferenced: the checks fail or return first
    assert f(-1, ctypes.byref(st), 0.0, fake, None, fake, fake, None, None, None, None, None) == E_RANGE
    assert f(0, ctypes.byref(st), 0.0, None, None, None, None, None, None, None, None, None) == OK
    assert f(4, None, 0.0, fake, None, fake, fake, None, None, None, None, None) == E_NULL
    assert f(4, ctypes.byref(st), 0.0, None, None, fake, fake, None, None, None, None, None) == E_NULL
    assert f(4, ctypes.byref(st), 0.0, fake, None, None, fake, fake, fake, fake, fake, None) == E_NULL
    assert f(4, ctypes.byref(st), 0.0, fake, None, fake, fake, fake, fake, fake, fake, None) == E_NULL   # (no profile arrays)


def test_profile_tensors_that_require_a_gradient_make_the_run_differentiable():
    from grad_june_amd.graph import HeteroData
    from grad_june_amd.transmission import PROFILE, profile_inputs, profile_requires_grad

    d = HeteroData()
    ip = {k: torch.ones(5) for k in PROFILE}
    d["agent"].infection_parameters = ip
    assert not profile_requires_grad(d) and profile_inputs(ip) == []
    loc = torch.nn.Parameter(torch.tensor(1.56))
    ip["shape"] = loc + torch.zeros(5)                   # what rsample of a Normal(loc, ...) hands over
    assert profile_requires_grad(d)
    assert [t is ip[k] for t, k in zip(profile_inputs(ip), PROFILE)] == [True] * 4


# ---- the oracle against the reference's recorded gradients (tests/golden/grads_params.npz) -------------------------
PARAM_CASES = ["p1", "p2"]


def load_params_case(case):
    import gj_testlib as L

    npz = L.load_npz("grads_params.npz")
    pre = case + "/"
    sub = {k[len(pre):]: v for k, v in npz.items() if k.startswith(pre)}
    world = L.world_from(sub)
    tables = {k[6:]: torch.from_numpy(v) for k, v in sub.items() if k.startswith("table/")}
    return sub, world, tables, str(sub["networks"]).split(",")


def distribution_gradients(sub, k, g_agent):
    """d loss / d (loc, scale) of the distribution parameter ``k`` from the per-agent gradients, by the reparameterisation
    rsample used: Normal x = loc + scale * eps; LogNormal x = exp(loc + scale * eps)."""
    x = torch.from_numpy(sub["state0/" + k]).double()
    g = g_agent.double()
    loc, scale = float(sub[f"dist/{k}/loc"]), float(sub[f"dist/{k}/scale"])
    if str(sub[f"dist/{k}/kind"]) == "LogNormal":
        eps = (torch.log(x) - loc) / scale
        return float((g * x).sum()), float((g * x * eps).sum())
    eps = (x - loc) / scale
    return float(g.sum()), float((g * eps).sum())


def assert_matches_reference(sub, tag, got_agent, got_log_beta, names, rtol=2e-4, atol=1e-6):
    for k in PROFILE_KEYS:
        ref = torch.from_numpy(sub[f"grad_{tag}/agent/{k}"]).double()
        g = got_agent[k].detach().double().cpu()
        err = float((g - ref).abs().max())
        assert err <= rtol * float(ref.abs().max()) + atol, (tag, k, err)
        loc, scale = distribution_gradients(sub, k, g)
        assert loc == pytest.approx(float(sub[f"grad_{tag}/dist/{k}/loc"]), rel=rtol, abs=atol), (tag, k, "loc")
        assert scale == pytest.approx(float(sub[f"grad_{tag}/dist/{k}/scale"]), rel=rtol, abs=atol), (tag, k, "scale")
    for n in names:
        assert got_log_beta[n] == pytest.approx(float(sub[f"grad_{tag}/{n}"]), rel=rtol, abs=atol), (tag, n)



def test_the_reparameterisation_reproduces_the_recorded_distribution_gradients():
    """The fixture is self-consistent: its loc / scale gradients are the chain rule of its per-agent ones."""
    for case in PARAM_CASES:
        sub, _, _, _ = load_params_case(case)
        for tag in ("last", "series"):
            for k in PROFILE_KEYS:
                loc, scale = distribution_gradients(sub, k, torch.from_numpy(sub[f"grad_{tag}/agent/{k}"]))
                assert loc == pytest.approx(float(sub[f"grad_{tag}/dist/{k}/loc"]), rel=1e-4, abs=1e-6), (case, k)
                assert scale == pytest.approx(float(sub[f"grad_{tag}/dist/{k}/scale"]), rel=1e-4, abs=1e-6), (case, k)


@pytest.mark.parametrize("case", PARAM_CASES)
def test_oracle_autograd_matches_the_reference_profile_gradients(case):
    """Autograd through oracle/gj_oracle.py (transmission_update, sample_infected, hot_path_step with tensor betas) on
    the recorded steps reproduces the reference's gradients w.r.t. the drawn profile, the distributions' loc / scale and
    every log_beta of the same run, for both losses."""
    import gj_oracle as O
    from test_gradients import step_info

    sub, world, tables, names = load_params_case(case)
    mult = {n: torch.ones((), requires_grad=True) for n in names}
    st = {k[7:]: torch.from_numpy(v) for k, v in sub.items() if k.startswith("state0/")}
    leaves = {k: st[k].clone().requires_grad_() for k in PROFILE_KEYS}
    st.update(leaves)
    series = []
    for i in range(int(sub["n_steps"])):
        s = step_info(sub, i)
        st["current_stage"] = s["stage"]
        betas = {n: torch.tensor(np.float32(s["betas"][n])) * mult[n] for n in s["active"]}
        out = O.hot_path_step(world, st, now=s["now"], delta_time=s["dt"], day_type=s["day_type"], active=s["active"],
                              betas=betas, leisure_tables=tables, quarantine_thresholds=s["thr"], exp_noise=s["noise"])
        for k in ("susceptibility", "is_infected", "infection_time"):
            st[k] = out[k]
        assert np.array_equal(out["is_infected"].detach().numpy(), s["is_infected"]), i
        series.append(out["is_infected"].sum())
    for tag, loss in (("last", series[-1]), ("series", torch.stack(series).sum())):
        grads = torch.autograd.grad(loss, [leaves[k] for k in PROFILE_KEYS] + [mult[n] for n in names],
                                    retain_graph=True, allow_unused=True)
        agent = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(PROFILE_KEYS, grads[:4])}
        lb = {n: (0.0 if g is None else float(g) * np.log(10.0)) for n, g in zip(names, grads[4:])}
        assert_matches_reference(sub, tag, agent, lb, names)


# ---- what is not differentiable yet says so instead of cutting the gradient ----------------------------------------
def test_a_distancing_factor_that_requires_a_gradient_is_refused():
    import datetime

    from grad_june_amd.infection_networks import HouseholdNetwork
    from grad_june_amd.policies import InteractionPolicies, Policies, SocialDistancing

    sd = SocialDistancing("2022-02-01", "2022-03-01", {"household": 0.5})
    policies = Policies(interaction_policies=InteractionPolicies([sd]))
    net = HouseholdNetwork(log_beta=0.3, device="cpu")
    timer = type("T", (), {"date": datetime.datetime(2022, 2, 3)})()
    plain = net.beta_value(policies, timer)
    assert plain == pytest.approx(10 ** 0.3 * 0.5, rel=1e-6)
    sd.beta_factors["household"] = torch.nn.Parameter(torch.tensor(0.5))
    with pytest.raises(NotImplementedError, match="SocialDistancing"):
        net.beta_value(policies, timer)
    with torch.no_grad():                                   # no gradient asked for: the plain value
        assert net.beta_value(policies, timer) == plain


def test_an_initial_case_fraction_that_requires_a_gradient_is_refused():
    from grad_june_amd.infection import infect_fraction_of_people

    log_fraction = torch.nn.Parameter(torch.tensor(-2.0))
    with pytest.raises(NotImplementedError, match="initial-case fraction"):
        infect_fraction_of_people(data=None, timer=None, symptoms_updater=None, fraction=10.0 ** log_fraction,
                                  device="cpu")
