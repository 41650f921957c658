"""CPU: the ContactQuarantine policy's host side - the YAML schema (one window and numbered windows), what it refuses
(overlapping windows, days <= 0, a compliance that requires a gradient), its place among the quarantine policies, and
that a configuration without the policy builds exactly as before.  No launch: the kernels are tested on the GPU."""
import datetime
import math

import pytest
import torch

from grad_june_amd.policies import ContactQuarantine, Policies, Quarantine, QuarantinePolicies, QUARANTINE_STREAM
from grad_june_amd.timer import Timer

WINDOW = {"start_date": "2020-03-16", "end_date": "2020-07-01", "stage_threshold": 4, "contacts": {"household": 14},
          "compliance": 0.8}


def _params(quarantine):
    return {"system": {"device": "cpu"}, "policies": {"quarantine": quarantine}}


def test_one_window_from_yaml():
    pol = Policies.from_parameters(_params({"contact_quarantine": dict(WINDOW)}))
    (p,) = pol.quarantine_policies.policies
    assert isinstance(p, ContactQuarantine) and isinstance(p, Quarantine) and p.spec == "quarantine"
    assert p.contacts == {"household": 14.0} and p.compliance == 0.8 and p.stage_threshold == 4
    assert p.start_date == datetime.datetime(2020, 3, 16) and p.end_date == datetime.datetime(2020, 7, 1)
    assert pol.quarantine_policies.contact_policies == [p]
    assert ContactQuarantine(**{k: v for k, v in WINDOW.items() if k != "compliance"}).compliance == 1.0


def test_numbered_windows_and_any_policy_group():
    second = dict(WINDOW, start_date="2020-07-01", end_date="2020-09-01", contacts={"household": 14, "company": 7})
    params = {"system": {"device": "cpu"},
              "policies": {"tracing": {"contact_quarantine": {1: dict(WINDOW), 2: second}},
                           "quarantine": {"quarantine": {"start_date": "2020-03-01", "end_date": "2020-04-01",
                                                         "stage_threshold": 5}}}}
    qp = Policies.from_parameters(params).quarantine_policies
    assert len(qp.policies) == 3 and len(qp.contact_policies) == 2      # adjacent windows do not overlap
    assert qp.contact_policies[1].contacts == {"household": 14.0, "company": 7.0}
    assert [type(p) for p in qp.policies].count(Quarantine) == 1


def test_its_threshold_joins_the_minimum_like_a_plain_quarantine():
    """``threshold`` (the index rule) is the min over the active policies, a ContactQuarantine among them; with no mask
    formed yet the launch threshold is that value, and the mask is the plain one."""
    timer = Timer(initial_day="2020-03-20", total_days=5)
    stages = torch.tensor([1.0, 3.0, 4.0, 5.0])
    for cls, extra in ((Quarantine, {}), (ContactQuarantine, {"contacts": {"household": 14}})):
        qp = QuarantinePolicies([cls(start_date="2020-03-16", end_date="2020-07-01", stage_threshold=4, **extra),
                                 Quarantine(start_date="2020-01-01", end_date="2020-03-18", stage_threshold=2)])
        qp.apply(symptom_stages=stages, timer=timer)
        assert qp.threshold == 4.0 and qp.launch_threshold == 4.0 and qp.qstate is None
        assert qp.quarantine_mask.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert QUARANTINE_STREAM == 1 << 59


def test_overlapping_windows_are_refused_naming_both():
    a = ContactQuarantine(**WINDOW)
    b = ContactQuarantine(**dict(WINDOW, start_date="2020-06-30", end_date="2020-08-01"))
    with pytest.raises(ValueError, match=r"\[2020-03-16, 2020-07-01\).*\[2020-06-30, 2020-08-01\).*overlap"):
        QuarantinePolicies([a, b])
    with pytest.raises(ValueError, match="overlap"):
        Policies.from_parameters(_params({"contact_quarantine": {1: dict(WINDOW), 2: dict(WINDOW)}}))
    QuarantinePolicies([a, Quarantine(start_date="2020-03-16", end_date="2020-07-01", stage_threshold=3)])   # a plain one may


@pytest.mark.parametrize("days", [0, -1, float("nan")])
def test_days_must_be_positive(days):
    with pytest.raises(ValueError, match="days > 0"):
        ContactQuarantine(**dict(WINDOW, contacts={"household": days}))


def test_contacts_and_compliance_are_checked():
    with pytest.raises(ValueError, match="contacts"):
        ContactQuarantine(**dict(WINDOW, contacts={}))
    with pytest.raises(ValueError, match="compliance"):
        ContactQuarantine(**dict(WINDOW, compliance=1.5))
    with pytest.raises(NotImplementedError, match="compliance"):
        ContactQuarantine(**dict(WINDOW, compliance=torch.tensor(0.5, requires_grad=True)))
    assert ContactQuarantine(**dict(WINDOW, compliance=torch.tensor(0.5))).compliance == 0.5


def test_a_model_without_the_policy_builds_as_before():
    """Nothing of the policy is allocated, and the quarantine collection answers as it did."""
    from grad_june_amd.defaults import default_parameters

    pol = Policies.from_parameters(default_parameters("cpu"))
    qp = pol.quarantine_policies
    assert qp.contact_policies == [] and qp.qstate is None and qp._contact == {} and qp._qstate_buffer is None
    assert all(type(p) is Quarantine for p in qp.policies)
    timer = Timer(initial_day="2022-02-01", total_days=3)
    stages = torch.tensor([1.0, 5.0, 7.0])
    qp.apply(symptom_stages=stages, timer=timer)
    active = [float(p.stage_threshold) for p in qp.policies if p.is_active(timer.date)]
    want = min(active) if active else math.inf
    assert qp.threshold == want and qp.launch_threshold == want
    assert qp.quarantine_mask.tolist() == (stages < want).float().tolist()
    pol.reset()                                                    # nothing to forget: no error, nothing allocated
    assert qp._contact == {}
    empty = Policies.from_policy_list([])
    assert not list(empty.quarantine_policies.policies) and empty.quarantine_policies.contact_policies == []


def test_the_entry_points_check_their_arguments_without_a_gpu():
    """GJ_E_RANGE / GJ_E_NULL come back before anything touches the device; n == 0 launches nothing."""
    import ctypes as C

    from grad_june_amd import _native as N

    lib = N.load()
    rowptr, venue, until = (C.c_int32 * 2)(0, 0), (C.c_int32 * 1)(0), (C.c_uint32 * 1)(0)
    stage, q, err = (C.c_float * 1)(1.0), (C.c_float * 1)(0.0), C.c_uint32(0)
    sets = (N.ContactSet * 2)()
    for s in sets:
        s.a_rowptr, s.a_venue, s.until = C.addressof(rowptr), C.addressof(venue), C.addressof(until)
        s.n_venues, s.release = 1, 15.0
    st, qs, er = C.addressof(stage), C.addressof(q), C.addressof(err)
    mark = lambda n=1, stage=st, sets=sets, n_sets=2, err=er: lib.gj_contact_mark(n, stage, 4.0, sets, n_sets, err, None)
    mask = lambda n=1, stage=st, sets=sets, n_sets=2, offset=0, qstate=qs, err=er: lib.gj_contact_mask(
        n, stage, 4.0, sets, n_sets, 1.0, 1.0, 1, 2, offset, qstate, err, None)
    for call in (mark, mask):
        assert call(n=-1) == -2 and call(n_sets=0) == -2 and call(n_sets=N.GJ_MAX_SETS + 1) == -2
        assert call(sets=None) == -1 and call(err=None) == -1 and call(stage=None) == -1
        sets[1].n_venues = 2 ** 31
        assert call() == -2
        sets[1].n_venues, sets[1].a_venue = 1, None
        assert call() == -1
        sets[1].a_venue = C.addressof(venue)
        assert call(n=0, stage=None) == 0
    assert mask(qstate=None) == -1 and mask(offset=-1) == -2 and mask(n=0, stage=None, qstate=None) == 0
    sets[0].release = float("nan")
    assert mark() == -2
    assert err.value == 0 and until[0] == 0 and q[0] == 0.0
