"""CPU: the Testing policy's host side - schema, refusals, tables - the numpy restatement (tests/gj_testing_ref.py) driven
by the recorded stage rows of the 769-agent world, the struct's layout and the entry points' argument checks.  The
kernels are tested in test_gpu_testing_kernel.py, whole runs in test_gpu_testing.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import gj_testing_ref as R
import gj_testlib as L
import grad_june_amd.policies as P
from grad_june_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gradjune_hip.h")

CONFIG = """
policies:
  testing:
    testing:
      start_date: 2020-03-16
      end_date: 2020-09-01
      stage_threshold: 4
      probability: {"0-18": 0.1, "18-65": 0.4, "65-100": 0.7}
      delay: {1: 0.2, 2: 0.5, 3: 0.3}
      isolation: {days: 10, compliance: 0.9}
"""
WINDOW = dict(start_date="2020-03-16", end_date="2020-09-01", stage_threshold=4)


def _params(text=CONFIG):
    params = yaml.safe_load(text) or {}
    params["system"] = {"device": "cpu"}
    return params


def test_from_parameters_builds_the_policy():
    """(fails without the feature: there is no class for the ``testing`` key)"""
    import grad_june_amd as G

    policies = P.Policies.from_parameters(_params())
    assert isinstance(policies.testing_policies, P.TestingPolicies) and G.Testing is P.Testing
    (t,) = policies.testing_policies.policies
    assert t.spec == "testing" and t.stage_threshold == 4.0
    assert t.probability.dtype == torch.float32 and t.probability.tolist() == [np.float32(0.1), np.float32(0.4), np.float32(0.7)]
    assert t.band_of_age == [0] * 18 + [1] * 47 + [2] * 35
    assert t.delay_days.tolist() == [1.0, 2.0, 3.0]
    assert t.delay_cum.tolist() == [np.float32(0.2), np.float32(0.7), 1.0]
    assert t.isolates and t.isolation_days == 10.0 and t.compliance == 0.9
    assert P.Policies().testing_policies is None
    assert len(P.Policies.from_parameters(_params("{}")).testing_policies.policies) == 0


def test_numbered_windows_and_plain_numbers():
    text = """
policies:
  testing:
    testing:
      1: {start_date: 2020-03-01, end_date: 2020-04-01, stage_threshold: 4, probability: 0.25, delay: 2}
      2: {start_date: 2020-04-01, end_date: 2020-05-01, stage_threshold: 3, probability: 1}
"""
    a, b = P.Policies.from_parameters(_params(text)).testing_policies.policies
    assert a.probability.tolist() == [0.25] and a.band_of_age == [0] * 100 and not a.isolates
    assert a.delay_days.tolist() == [2.0] and a.delay_cum.tolist() == [1.0]
    assert b.delay_days.tolist() == [0.0] and b.stage_threshold == 3.0


def test_the_tables_round_each_value_once():
    t = P.Testing(**WINDOW, probability={"65-100": 0.7, "0-18": 0.1}, delay={0: 0.1, 5: 0.2, 1: 0.7})      # file order
    assert t.band_of_age[17] == 1 and t.band_of_age[18] == -1 and t.band_of_age[65] == 0
    tab = t.tables()
    assert list(tab.probability) == list(R.probability_table({"65-100": 0.7, "0-18": 0.1}))
    assert tab.probability[30] == 0.0      # an age in no band
    cum, days = R.delay_tables({0: 0.1, 5: 0.2, 1: 0.7})
    assert tab.n_delays == 3 and list(tab.delay_cum)[:3] == list(cum) and list(tab.delay_days)[:3] == list(days)
    assert cum[1] == np.float32(0.1 + 0.2)      # the running fp64 sum, rounded once
    # a probability replaced by a Parameter of the same shape is what the tables read
    t.probability = torch.nn.Parameter(torch.tensor([0.5, 0.25]))
    assert t.tables().probability[70] == 0.5 and t.tables().probability[3] == 0.25
    t.probability = torch.nn.Parameter(torch.tensor([0.5]))
    with pytest.raises(ValueError, match="one value per band"):
        t.tables()


@pytest.mark.parametrize("kwargs, word", [
    (dict(probability=1.5), "1.5"),
    (dict(probability={"0-18": -0.25}), "-0.25"),
    (dict(probability={"18-10": 0.5}), "18-10"),
    (dict(probability={"0-30": 0.5, "20-40": 0.5}), "overlapping"),
    (dict(probability=0.5, delay=-1), "-1"),
    (dict(probability=0.5, delay={1: 0.5, 2: 0.25}), "0.75"),
    (dict(probability=0.5, delay={1: 1.5, 2: -0.5}), "-0.5"),
    (dict(probability=0.5, delay={-2: 1.0}), "-2"),
    (dict(probability=0.5, delay={k: 1 / 17 for k in range(17)}), "17"),
    (dict(probability=0.5, isolation={"days": 0}), "days = 0"),
    (dict(probability=0.5, isolation={"days": 5, "compliance": 1.25}), "1.25"),
    (dict(probability=0.5, isolation={"compliance": 1.0}), "isolation"),
])
def test_bad_values_are_refused_by_name(kwargs, word):
    with pytest.raises(ValueError, match=word):
        P.Testing(**WINDOW, **kwargs)


def test_a_compliance_that_requires_a_gradient_is_refused():
    with pytest.raises(NotImplementedError, match="compliance"):
        P.Testing(**WINDOW, probability=0.5, isolation={"days": 5, "compliance": torch.tensor(0.5, requires_grad=True)})


def test_overlapping_windows_are_refused():
    a = P.Testing("2020-03-01", "2020-04-01", 4, 0.5)
    b = P.Testing("2020-03-31", "2020-05-01", 4, 0.5)
    with pytest.raises(ValueError, match="overlap"):
        P.TestingPolicies([a, b])
    P.TestingPolicies([a, P.Testing("2020-04-01", "2020-05-01", 4, 0.5)])      # adjoining windows do not
    cq = P.ContactQuarantine("2020-03-15", "2020-06-01", 4, {"household": 14})
    isolating = P.Testing("2020-03-01", "2020-04-01", 4, 0.5, isolation={"days": 7})
    with pytest.raises(ValueError, match="ContactQuarantine"):
        P.Policies.from_policy_list([cq, isolating])
    P.Policies.from_policy_list([cq, a])      # without isolation nothing collides
    P.Policies.from_policy_list([P.ContactQuarantine("2020-04-01", "2020-06-01", 4, {"household": 14}), isolating])


def test_a_negative_time_is_refused_before_any_launch():
    class Clock:
        import datetime
        date, now = datetime.datetime(2020, 3, 20), -1.0

    tp = P.TestingPolicies([P.Testing(**WINDOW, probability=0.5)])
    with pytest.raises(ValueError, match="timer.now"):
        tp.step({"agent": {}}, Clock(), seed=1)
    Clock.date = Clock.datetime.datetime(2020, 1, 1)      # before the first active step: nothing at all
    assert tp.step({"agent": {}}, Clock(), seed=1) is None and tp.state(0) is None


def test_layout_equals_what_a_c_compiler_sees(tmp_path):
    import shutil
    import subprocess

    assert ctypes.sizeof(N.TestingTables) == 4 * (100 + 2 * N.GJ_TESTING_MAX_DELAYS + 2)
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gj_testing_tables));',
             '  printf("flags %u\\n", GJ_TESTING_DECIDED | GJ_TESTING_POSITIVE << 8 | GJ_TESTING_DUE << 16);',
             '  printf("delays %d\\n", GJ_TESTING_MAX_DELAYS);']
    for field, _ in N.TestingTables._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(gj_testing_tables, {field}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(N.TestingTables)
    assert int(got["flags"]) == N.GJ_TESTING_DECIDED | N.GJ_TESTING_POSITIVE << 8 | N.GJ_TESTING_DUE << 16
    assert (R.DECIDED, R.POSITIVE, R.DUE) == (N.GJ_TESTING_DECIDED, N.GJ_TESTING_POSITIVE, N.GJ_TESTING_DUE)
    assert int(got["delays"]) == N.GJ_TESTING_MAX_DELAYS == P.TESTING_MAX_DELAYS == R.MAX_DELAYS
    for field, _ in N.TestingTables._fields_:
        assert int(got[field]) == getattr(N.TestingTables, field).offset, field
    assert (P.TESTING_STREAM, P.TESTING_COMPLY_STREAM) == (R.TESTING_STREAM, R.COMPLY_STREAM)


from test_launch_validation import lib  # noqa: E402,F401  (the fixture: the library, built if it is not there)


def test_the_abi_version_is_still_7(lib):  # noqa: F811
    assert N.GJ_ABI_VERSION == 7 and lib.gj_version() == 7
    assert hasattr(lib, "gj_testing_step") and hasattr(lib, "gj_adjoint_testing")


def test_the_entries_reject_bad_arguments_before_any_launch(lib):  # noqa: F811
    """The host never dereferences a device pointer: every case is rejected with a negative code before a launch (or,
    n == 0, returns at once)."""
    from test_launch_validation import E_NULL, E_RANGE, FAKE, OK

    t = N.TestingTables()
    t.n_delays = 1
    bad_lo, bad_hi = N.TestingTables(), N.TestingTables()
    bad_lo.n_delays, bad_hi.n_delays = 0, N.GJ_TESTING_MAX_DELAYS + 1
    S = R.TESTING_STREAM

    def step(n=8, cls=FAKE, tab=t, stage=FAKE, time=FAKE, now=1.0, stream=S, offset=0, dec=FAKE, res=FAKE, pos=FAKE,
             iso=FAKE, conf=FAKE, q=FAKE):
        return lib.gj_testing_step(n, cls, tab, stage, time, 4.0, 1, now, 1e30, 10.0, 1.0, 7, stream, R.COMPLY_STREAM,
                                   offset, dec, res, pos, iso, conf, None, q, None, None, None)

    assert step(n=0, cls=None, tab=None, stage=None, time=None, dec=None, res=None, pos=None, iso=None, conf=None, q=None) == OK
    assert step(n=-1) == E_RANGE and step(offset=-1) == E_RANGE and step(now=-0.5) == E_RANGE
    assert step(now=float("nan")) == E_RANGE and step(stream=S | 5) == E_RANGE
    assert step(tab=bad_lo) == E_RANGE and step(tab=bad_hi) == E_RANGE
    for name in ("cls", "tab", "stage", "time", "dec", "res", "pos", "conf"):
        assert step(**{name: None}) == E_NULL, name
    assert step(iso=None) == E_NULL      # a mask without isolate_until
    plan = N.SeedPlan(8, 1, FAKE, FAKE, FAKE, FAKE)

    def adj(n=8, flags=FAKE, stage=FAKE, band=FAKE, B=1, plan=plan, contrib=FAKE, partial=FAKE, out=FAKE):
        return lib.gj_adjoint_testing(n, flags, stage, None, None, band, B,
                                      ctypes.byref(plan) if plan is not None else None, contrib, partial, out, None, None,
                                      None)

    assert adj(n=-1) == E_RANGE and adj(B=0) == E_RANGE and adj(B=N.GJ_MAX_GROUPS + 1) == E_RANGE
    for name in ("flags", "stage", "band", "plan", "contrib", "partial", "out"):
        assert adj(**{name: None}) == E_NULL, name
    assert adj(plan=N.SeedPlan(9, 1, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more sorted agents than agents
    assert adj(plan=N.SeedPlan(8, 3, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more chunks than the sizes allow
    assert adj(plan=N.SeedPlan(8, 1, None, FAKE, FAKE, FAKE)) == E_NULL


# ---- the restatement on the recorded run ------------------------------------------------------------------------------
PROBABILITY = {"0-18": 0.3, "18-65": 0.5, "65-100": 0.8}
DELAY = {1: 0.2, 2: 0.5, 3: 0.3}
SEED = 20200316


@pytest.fixture(scope="module")
def recorded():
    z = L.load_npz("june769_series.npz")
    infected, stage = z["post/is_infected"], z["post/current_stage"].astype(np.float32)
    ever = (infected > 0).any(0)
    infection_time = np.where(ever, (infected > 0).argmax(0), -1).astype(np.float32)
    cls = (z["sex"] * 100 + z["age"]).astype(np.uint8)
    band = np.digitize(z["age"], [18, 65])
    return {"stage": stage, "infection_time": infection_time, "cls": cls, "band": band, "n": stage.shape[1]}


def run(rec, probability=PROBABILITY, delay=DELAY, order=None, **kwargs):
    """The 90 launches: launch k (the Runner's row k + 1) sees stage row k at time k + 1.  Returns the per-launch
    outputs and the final state; ``order``: a permutation of the agents, which keep their ids."""
    n = rec["n"]
    order = np.arange(n) if order is None else order
    state = R.initial_state(n)
    cum, days = R.delay_tables(delay)
    table = R.probability_table(probability) if isinstance(probability, dict) else np.full(100, probability, np.float32)
    outs = [R.step(state, rec["cls"][order], rec["stage"][k][order], rec["infection_time"][order], probability=table,
                   delay_cum=cum, delay_days=days, stage_threshold=4, active=True, now=float(k + 1), seed=SEED,
                   ids=order.astype(np.uint64), **kwargs) for k in range(len(rec["stage"]))]
    return outs, state


def test_the_recording_reaches_the_threshold_as_documented(recorded):
    reached = (recorded["stage"] >= 4).any(0)
    assert int(reached.sum()) == 285
    assert np.bincount(recorded["band"][reached], minlength=3).tolist() == [51, 217, 17]


def test_floors_on_the_recorded_run(recorded):
    """What keeps the GPU tests from passing vacuously: enough positives, negatives and decisions in every band."""
    outs, state = run(recorded)
    decided = state["decided"] != 0xFFFFFFFF
    assert sum(o["counts"][1] for o in outs) == int(decided.sum()) == 285      # each infection decided once
    positives = int((state["positive"] != 0).sum())
    print("positives", positives, "negatives", int(decided.sum()) - positives)
    assert positives >= 40 and int(decided.sum()) - positives >= 40
    assert np.bincount(recorded["band"][decided], minlength=3).min() >= 3
    confirmed = sum(o["counts"][0] for o in outs)
    assert 0 < confirmed <= positives and confirmed == int((state["confirmed_time"] >= 0).sum())
    # every delay of the table occurs: the time from the first row at the threshold to the confirmation
    first = (recorded["stage"] >= 4).argmax(0) + 1.0
    lag = (state["confirmed_time"] - first)[state["confirmed_time"] >= 0]
    assert set(np.unique(lag).tolist()) == {1.0, 2.0, 3.0}


def test_full_ascertainment_without_delay_counts_everybody_at_the_threshold(recorded):
    outs, state = run(recorded, probability=1.0, delay=0)
    cumulative = np.cumsum([o["counts"][0] for o in outs])
    seen = np.cumsum([(~(recorded["stage"][: k + 1] < 4)).any(0).sum() - (~(recorded["stage"][:k] < 4)).any(0).sum()
                      for k in range(len(outs))])
    # row k + 1 of the Runner = launch k: the agents at or above the threshold in the stage rows up to k
    assert cumulative.tolist() == seen.tolist() and cumulative[-1] == 285
    assert np.isinf(state["result_time"]).all()


def test_rows_by_group_sum_to_the_national_row(recorded):
    outs, _ = run(recorded)
    for o in outs:
        by_band = np.bincount(recorded["band"], weights=o["newly"], minlength=3)
        assert by_band.sum() == o["counts"][0]


def test_permuting_the_agents_with_their_ids_permutes_the_result(recorded):
    order = np.random.default_rng(3).permutation(recorded["n"])
    outs, state = run(recorded, isolation_days=10, compliance=0.9)
    outs_p, state_p = run(recorded, order=order, isolation_days=10, compliance=0.9)
    for key in state:
        assert np.array_equal(state[key][order], state_p[key]), key
    for o, o_p in zip(outs, outs_p):
        assert np.array_equal(o["newly"][order], o_p["newly"]) and np.array_equal(o["qstate"][order], o_p["qstate"])
    assert any((o["qstate"] == 3).any() for o in outs) and (state["isolate_until"] > 0).sum() < (state["confirmed_time"] >= 0).sum()


def test_the_restatement_takes_each_branch():
    cum, days = R.delay_tables({0: 0.5, 2: 0.5})
    table = np.full(100, 1.0, np.float32)
    table[50:] = 0.0
    cls = np.array([10, 10, 60, 10, 110, 10], np.uint8)
    stage = np.array([4, 3, 4, np.nan, 5, 4], np.float32)
    time = np.array([0.0, 0.0, 1.0, 2.0, -0.0, 3.0], np.float32)
    state = R.initial_state(6)
    state["decided"][5] = np.float32(3.0).view(np.uint32)      # this infection was decided before
    state["result_time"][5], state["positive"][5] = 7.0, 1.0      # ... and its result is due exactly now
    kw = dict(probability=table, delay_cum=cum, delay_days=days, stage_threshold=4, seed=5, isolation_days=4, q_threshold=5)
    out = R.step(state, cls, stage, time, active=True, now=7.0, **kw)
    assert (out["flags"] & R.DECIDED).tolist() == [1, 0, 1, 1, 1, 0]
    assert state["positive"].tolist() == [1, 0, 0, 1, 1, 1]      # ages 10 / 110 % 100 = 10: p = 1; age 60: p = 0
    assert out["flags"][5] == R.DUE | R.POSITIVE and state["confirmed_time"][5] == 7.0 and state["isolate_until"][5] == 11.0
    assert out["qstate"][4] == 1.0 and out["qstate"][5] == 3.0 and out["qstate"][1] == 0.0
    assert set(state["result_time"][[0, 2, 3, 4]].tolist()) <= {np.inf, 9.0}
    again = R.step(state, cls, stage, time, active=True, now=8.0, **kw)
    assert again["counts"][1] == 0      # equal bits: no new decision
    time[0] = -0.0      # other bits: a new infection
    assert R.step(state, cls, stage, time, active=True, now=8.5, **kw)["counts"][1] == 1
    time[4] = 0.0
    assert R.step(state, cls, stage, time, active=False, now=9.0, **kw)["counts"][1] == 0      # decisions only while active
