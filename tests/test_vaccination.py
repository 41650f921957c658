"""CPU: the Vaccination policy's host side - schema, ramp, per-age tables, reset - and the monotone rollout of the numpy
restatement (tests/gj_vaccination_ref.py).  The kernels are tested in test_gpu_vaccination.py."""
import datetime

import numpy as np
import pytest
import torch
import yaml

import gj_vaccination_ref as V
from grad_june_amd import policies as P

CONFIG = """
policies:
  vaccination:
    vaccination:
      1: {start_date: 2021-01-04, end_date: 2021-03-01,
          coverage: {"65-100": 0.9, "18-65": 0.6}, efficacy: {"65-100": 0.6, "18-65": 0.8}}
      2: {start_date: 2021-02-01, end_date: 2021-02-01, coverage: 0.25, efficacy: 0.5}
"""


def _params(text=CONFIG):
    params = yaml.safe_load(text)
    params["system"] = {"device": "cpu"}
    return params


def test_numbered_windows_with_age_dicts_and_numbers():
    pol = P.Policies.from_parameters(_params())
    vp = pol.vaccination_policies
    assert isinstance(vp, P.VaccinationPolicies) and len(vp.policies) == 2
    a, b = vp[0], vp[1]
    assert isinstance(a, P.Vaccination) and a.spec == "vaccination"
    assert a.start_date == datetime.datetime(2021, 1, 4) and a.end_date == datetime.datetime(2021, 3, 1)
    assert len(a.coverage) == 100 and all(type(c) is float for c in a.coverage)
    assert a.coverage[17] == 0.0 and a.coverage[18] == 0.6 and a.coverage[64] == 0.6 and a.coverage[65] == 0.9
    assert a.coverage[99] == 0.9
    assert a.efficacy.dtype == torch.float32 and a.efficacy.tolist() == [np.float32(0.6), np.float32(0.8)]   # file order
    assert a.band_of_age[17] == -1 and a.band_of_age[18] == 1 and a.band_of_age[64] == 1 and a.band_of_age[65] == 0
    assert b.coverage == [0.25] * 100 and b.efficacy.tolist() == [0.5] and b.band_of_age == [0] * 100
    # the other kinds are there, and empty
    assert len(pol.interaction_policies.policies) == len(pol.quarantine_policies.policies) == 0


def test_one_window():
    params = _params("""
policies:
  vaccination:
    vaccination: {start_date: 2021-01-04, end_date: 2021-03-01, coverage: 0.5, efficacy: {"0-50": 0.7}}
""")
    (p,) = P.Policies.from_parameters(params).vaccination_policies.policies
    assert p.coverage == [0.5] * 100 and p.band_of_age == [0] * 50 + [-1] * 50
    t = p.tables(0.0, 1.0)
    assert list(t.factor)[:50] == [np.float32(1.0 - float(np.float32(0.7)))] * 50 and list(t.factor)[50:] == [1.0] * 50


def test_overlapping_efficacy_bands_are_refused():
    with pytest.raises(ValueError, match="overlapping"):
        P.Vaccination("2021-01-01", "2021-02-01", coverage=0.5, efficacy={"0-50": 0.5, "40-100": 0.6})
    P.Vaccination("2021-01-01", "2021-02-01", coverage=0.5, efficacy={"50-100": 0.5, "0-50": 0.6})      # touching: fine


def test_coverage_that_requires_a_gradient_is_refused():
    c = torch.tensor(0.5, requires_grad=True)
    with pytest.raises(NotImplementedError, match="coverage"):
        P.Vaccination("2021-01-01", "2021-02-01", coverage=c, efficacy=0.5)
    with pytest.raises(NotImplementedError, match="coverage"):
        P.Vaccination("2021-01-01", "2021-02-01", coverage={"0-50": c}, efficacy=0.5)
    p = P.Vaccination("2021-01-01", "2021-02-01", coverage=torch.tensor(0.5), efficacy=0.5)      # a plain tensor: fine
    assert p.coverage == [0.5] * 100


def test_efficacy_may_be_replaced_by_a_parameter():
    p = P.Vaccination("2021-01-01", "2021-02-01", coverage=0.5, efficacy={"0-50": 0.5, "50-100": 0.25})
    p.efficacy = torch.nn.Parameter(torch.tensor([0.75, 0.125]))
    assert [n for n, _ in p.named_parameters()] == ["efficacy"]
    assert P.VaccinationPolicies([p]).requires_grad()
    t = p.tables(0.0, 0.5)
    assert t.factor[10] == 0.25 and t.factor[60] == 0.875 and t.thr_hi[10] == 0.25 and t.thr_lo[10] == 0.0
    p.efficacy = torch.nn.Parameter(torch.tensor([0.75]))
    with pytest.raises(ValueError, match="one value per band"):
        p.tables(0.0, 0.5)


def test_ramp_values():
    p = P.Vaccination("2021-01-04", "2021-03-01", coverage=1.0, efficacy=0.5)
    start, end = p.start_date, p.end_date
    mid = start + (end - start) / 2
    assert p.ramp(start - datetime.timedelta(days=3)) == 0.0 and p.ramp(start) == 0.0
    assert p.ramp(mid) == 0.5
    assert p.ramp(start + datetime.timedelta(days=14)) == 14 / 56
    assert p.ramp(end) == 1.0 and p.ramp(end + datetime.timedelta(days=400)) == 1.0
    q = P.Vaccination("2021-02-01", "2021-02-01", coverage=1.0, efficacy=0.5)      # start == end
    assert q.ramp(q.start_date - datetime.timedelta(hours=12)) == 0.0 and q.ramp(q.start_date) == 1.0
    assert q.ramp(q.start_date + datetime.timedelta(hours=12)) == 1.0
    for date in (start, mid, end, end + datetime.timedelta(days=1)):
        assert p.ramp(date) == V.ramp(date, start, end)
    with pytest.raises(ValueError):
        P.Vaccination("2021-02-02", "2021-02-01", coverage=1.0, efficacy=0.5)


def test_tables_are_rounded_once_and_match_the_restatement():
    p = P.Policies.from_parameters(_params()).vaccination_policies[0]
    lo, hi = 3 / 7, 0.9
    t = p.tables(lo, hi)
    thr_lo, thr_hi, factor = V.tables(p.coverage, p.band_of_age, p.efficacy.numpy(), lo, hi)
    assert np.array_equal(np.array(list(t.thr_lo), dtype=np.float32), thr_lo)
    assert np.array_equal(np.array(list(t.thr_hi), dtype=np.float32), thr_hi)
    assert np.array_equal(np.array(list(t.factor), dtype=np.float32), factor)
    assert thr_lo[70] == np.float32(0.9 * lo) and factor[10] == 1.0 and thr_hi[10] == 0.0


def test_reset_zeroes_the_applied_ramps():
    pol = P.Policies.from_parameters(_params())
    for p in pol.vaccination_policies.policies:
        p.applied = 0.75
    pol.reset()
    assert [p.applied for p in pol.vaccination_policies.policies] == [0.0, 0.0]


def test_rollout_of_the_restatement_is_monotone():
    """The union of the [lo, hi) slices over a run equals one [0, final) slice, and nobody is moved twice."""
    p = P.Policies.from_parameters(_params()).vaccination_policies[0]
    rng = np.random.default_rng(0)
    n = 5000
    age = rng.integers(0, 100, n)
    u = V.uniforms(99, V.stream_of(0), 5, n)
    eff = p.efficacy.numpy()
    date, applied, seen = p.start_date - datetime.timedelta(days=2), 0.0, np.zeros(n, dtype=np.int64)
    while date < p.end_date + datetime.timedelta(days=3):
        hi = p.ramp(date)
        if hi > applied:
            seen += V.newly(u, age, *V.tables(p.coverage, p.band_of_age, eff, applied, hi)[:2])
            applied = hi
        date += datetime.timedelta(hours=12)
    assert applied == 1.0
    once = V.newly(u, age, *V.tables(p.coverage, p.band_of_age, eff, 0.0, 1.0)[:2])
    assert np.array_equal(seen, once.astype(np.int64)) and 0 < once.sum() < n
    assert not once[age < 18].any()
    assert abs(once[age >= 65].mean() - 0.9) < 0.05 and abs(once[(age >= 18) & (age < 65)].mean() - 0.6) < 0.05


def test_policies_without_the_new_keyword_behave_as_before():
    pol = P.Policies(interaction_policies=P.InteractionPolicies([]), quarantine_policies=P.QuarantinePolicies([]),
                     close_venue_policies=P.CloseVenuePolicies([]))
    assert pol.vaccination_policies is None
    pol.reset()
    assert pol.vaccinate({"agent": {}}, timer=None, seed=1) is None      # nothing is touched: no campaign
    assert P.Policies().vaccination_policies is None
    empty = P.Policies.from_policy_list([])
    assert len(empty.vaccination_policies.policies) == 0
    assert empty.vaccinate({"agent": {}}, timer=None, seed=1) is None


from test_launch_validation import lib  # noqa: E402,F401  (the fixture: the library, built if it is not there)


def test_the_entries_reject_bad_arguments_before_any_launch(lib):  # noqa: F811
    """The library loads without a GPU and the host never dereferences a device pointer: every case is rejected with a
    negative code before a launch (or, n == 0, returns at once)."""
    import ctypes as C

    from grad_june_amd import _native as N
    from test_launch_validation import E_NULL, E_RANGE, FAKE, OK

    t = N.VaccinateTables()
    assert lib.gj_vaccinate(0, None, None, 1, 2, 0, None, None, None, None) == OK
    assert lib.gj_vaccinate(-1, FAKE, t, 1, 2, 0, FAKE, None, None, None) == E_RANGE
    assert lib.gj_vaccinate(8, FAKE, t, 1, 2, -4, FAKE, None, None, None) == E_RANGE
    assert lib.gj_vaccinate(8, None, t, 1, 2, 0, FAKE, None, None, None) == E_NULL
    assert lib.gj_vaccinate(8, FAKE, None, 1, 2, 0, FAKE, None, None, None) == E_NULL
    assert lib.gj_vaccinate(8, FAKE, t, 1, 2, 0, None, None, None, None) == E_NULL
    plan = N.SeedPlan(8, 1, FAKE, FAKE, FAKE, FAKE)
    adj = lambda n=8, cls=FAKE, tab=t, off=0, s0=FAKE, band=FAKE, B=1, plan=plan, contrib=FAKE, partial=FAKE, out=FAKE: \
        lib.gj_adjoint_vaccinate(n, cls, tab, 1, 2, off, s0, None, band, B, C.byref(plan) if plan is not None else None,
                                 contrib, partial, out, None, None)
    assert adj(n=-1) == E_RANGE and adj(off=-1) == E_RANGE and adj(B=0) == E_RANGE
    assert adj(out=None) == E_NULL and adj(plan=None) == E_NULL
    assert adj(cls=None) == E_NULL and adj(tab=None) == E_NULL and adj(s0=None) == E_NULL and adj(band=None) == E_NULL
    assert adj(contrib=None) == E_NULL and adj(partial=None) == E_NULL
    assert adj(plan=N.SeedPlan(9, 1, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more sorted agents than agents
    assert adj(plan=N.SeedPlan(8, 3, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more chunks than the sizes allow
    assert adj(plan=N.SeedPlan(8, 1, None, FAKE, FAKE, FAKE)) == E_NULL
