"""CPU: the numpy restatement of the contact-quarantine kernels (tests/gj_contact_ref.py) against a brute-force double
loop over COO edges on random small worlds, and the two properties the policy rests on: ``until`` never decreases, and a
venue stays marked exactly while its release time is later than ``now``."""
import numpy as np
import pytest

import gj_contact_ref as R


def _world(rng, n, n_sets=2):
    """COO edge lists of ``n_sets`` sets: agents with no edge, one edge and several; venues with no member."""
    sets = []
    for s in range(n_sets):
        n_venues = int(rng.integers(1, max(2, n // 2) + 1))
        degree = rng.choice([0, 1, 1, 1, 2, 5], size=n)
        agent = np.repeat(np.arange(n), degree)
        venue = rng.integers(0, n_venues, len(agent))
        shuffle = rng.permutation(len(agent))
        sets.append({"agent": agent[shuffle], "venue": venue[shuffle], "n_venues": n_venues, "days": [14.0, 2.5][s % 2]})
    return sets


def _csr_sets(coo, n, until):
    out = []
    for s, u in zip(coo, until):
        rowptr, venue = R.csr_by_agent(s["agent"], s["venue"], n)
        out.append({"rowptr": rowptr, "venue": venue, "until": u, "days": s["days"]})
    return out


def _brute_mark(stage, thr, coo, until, now):
    out = [u.copy() for u in until]
    for s, u in zip(coo, out):
        release = np.float32(np.float64(now) + s["days"])
        for a in range(len(stage)):
            if stage[a] < thr:
                continue
            for ea, ev in zip(s["agent"], s["venue"]):
                if ea == a and (u[ev].view(np.float32) < release):
                    u[ev] = release.view(np.uint32)
    return out


def _brute_mask(stage, thr, coo, until, now, compliance, u):
    q = np.zeros(len(stage), dtype=np.float32)
    for a in range(len(stage)):
        if not stage[a] < thr:
            q[a] = 1.0
            continue
        if not u[a] < np.float32(compliance):
            continue
        for s, ut in zip(coo, until):
            for ea, ev in zip(s["agent"], s["venue"]):
                if ea == a and ut[ev].view(np.float32) > np.float32(now):
                    q[a] = 2.0
    return q


@pytest.mark.parametrize("n", [1, 7, 40])
def test_restatement_against_a_double_loop(n):
    rng = np.random.default_rng(n)
    for trial in range(4):
        coo = _world(rng, n)
        stage = rng.choice([1.0, 2.0, 4.0, 5.0, np.nan, np.inf, -np.inf], size=n).astype(np.float32)
        now = float(rng.integers(0, 30)) + 0.5 * trial
        until = [np.where(rng.random(s["n_venues"]) < 0.5, 0, np.float32(now + rng.integers(-3, 4, s["n_venues"])).clip(0)
                          .view(np.uint32)).astype(np.uint32) for s in coo]
        u = R.uniforms(1234, R.stream_of(1), 4 * trial, n)
        sets = _csr_sets(coo, n, until)
        got, err = R.mark(stage, 4.0, sets, now)
        want = _brute_mark(stage, 4.0, coo, until, now)
        assert err == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
        assert all(np.array_equal(s["until"], u0) for s, u0 in zip(sets, until)), "mark changed its input"
        for compliance in (0.0, 0.5, 1.0):
            after = _csr_sets(coo, n, got)
            q, err = R.mask(stage, 4.0, after, now, compliance, u)
            assert err == 0 and np.array_equal(q, _brute_mask(stage, 4.0, coo, got, now, compliance, u)), compliance
            if compliance == 0.0:
                assert not (q == 2.0).any()


def test_until_never_decreases_and_holds_exactly_while_release_is_later():
    """Two agents in one household, agent 0 symptomatic on days 0 to 2, 3 days of quarantine: the household is marked
    until day 5 (2 + 3) - agent 1 is a contact on the days 0 .. 4 and free from day 5 on, the first with now >= release."""
    rowptr, venue = R.csr_by_agent([0, 1], [0, 0], 2)
    until = np.zeros(1, dtype=np.uint32)
    u = np.zeros(2, dtype=np.float32)
    seen = []
    for day in range(8):
        stage = np.array([5.0 if day <= 2 else 1.0, 1.0], dtype=np.float32)
        s = [{"rowptr": rowptr, "venue": venue, "until": until, "days": 3.0}]
        (after,), _ = R.mark(stage, 4.0, s, float(day))
        assert after[0] >= until[0]
        until = after
        q, _ = R.mask(stage, 4.0, [dict(s[0], until=until)], float(day), 1.0, u)
        assert (q[1] == 2.0) == (until.view(np.float32)[0] > np.float32(day))
        seen.append(q.tolist())
    assert until.view(np.float32)[0] == 5.0
    assert [q[1] for q in seen] == [2.0] * 5 + [0.0] * 3
    assert [q[0] for q in seen] == [1.0] * 3 + [2.0] * 2 + [0.0] * 3


def test_bad_rows_are_skipped_and_reported():
    rowptr, venue = R.csr_by_agent([0, 1, 2], [0, 1, 0], 3)
    stage = np.array([5.0, 5.0, 1.0], dtype=np.float32)
    bad = venue.copy()
    bad[1] = 7
    (until,), err = R.mark(stage, 4.0, [{"rowptr": rowptr, "venue": bad, "until": np.zeros(2, np.uint32), "days": 1.0}], 0.0)
    assert err == R.ERR_ROWS and until.view(np.float32).tolist() == [1.0, 0.0]
    broken = rowptr.copy()
    broken[1] = 9
    (until,), err = R.mark(stage, 4.0, [{"rowptr": broken, "venue": venue, "until": np.zeros(2, np.uint32), "days": 1.0}], 0.0)
    assert err == R.ERR_ROWS and until.view(np.float32).tolist() == [0.0, 0.0]
