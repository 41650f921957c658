"""GPU: gj_contact_mark and gj_contact_mask against their numpy restatement (tests/gj_contact_ref.py), bit for bit -
``until`` as uint32, ``qstate`` as fp32, the error word - over the sizes at which the kernels change form (vector tail,
wave and workgroup edges, a second trip of the grid-stride loops), in the four-agents-per-lane and the one-agent-per-lane
form, and every documented argument error."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gj_contact_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

SEED, POLICY = 0x1234567, 2
THRESHOLD, NOW = 4.0, 10.0
E_NULL, E_RANGE = -1, -2
STAGES = np.array([1.0, 2.0, 3.0, THRESHOLD, 5.0, np.nan, np.inf, -np.inf], dtype=np.float32)
#: until before the launch: never marked, released before / exactly at / after ``now``, and far later than any release
PRELOAD = np.array([0.0, NOW - 1.0, NOW, NOW + 1.0, NOW + 30.0], dtype=np.float32).view(np.uint32)


def _world(rng, n, long_row=True):
    """Two sets that share the agents, 14 and 7 days: agents with no row, one row, two rows, and (set 0, n >= 3) one
    agent with 70 rows; venue ids repeat inside a row."""
    sets = []
    for s, (days, degrees) in enumerate(((14.0, [0, 1, 1, 1]), (7.0, [0, 0, 1, 2]))):
        n_venues = max(1, n // (3 + 2 * s))
        degree = rng.choice(degrees, size=n)
        if s == 0 and long_row and n >= 3:
            degree[n // 2] = 70
        venue = rng.integers(0, n_venues, int(degree.sum())).astype(np.int32)
        sets.append({"rowptr": np.concatenate(([0], np.cumsum(degree))).astype(np.int32), "venue": venue, "days": days,
                     "until": rng.choice(PRELOAD, size=n_venues)})
    return sets


def _stages(rng, n):
    stage = rng.choice(STAGES, size=n, p=[0.3, 0.2, 0.2, 0.06, 0.06, 0.06, 0.06, 0.06])
    stage[: min(n, len(STAGES))] = STAGES[: min(n, len(STAGES))][::-1]      # the edge values are met at every n they fit in
    return stage.astype(np.float32)


def _shifted(values, shift, device, fill=None):
    """``values`` on the device at an element offset of ``shift``: 1 makes the array 4-byte, not 16-byte aligned."""
    buf = torch.empty(len(values) + shift + 4, dtype=torch.float32, device=device)
    view = buf[shift: shift + len(values)]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)) if fill is None
               else torch.full((len(values),), fill))
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return view


class Launch:
    """The two kernels on one world: device copies of the sets and the ctypes array that points at them."""

    def __init__(self, device, sets, now=NOW):
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if a.dtype == np.uint32
                                             else np.ascontiguousarray(a, dtype=dt)).to(device)
        self.device, self.now = device, now
        self.keep = [(dev(s["rowptr"], np.int32), dev(s["venue"], np.int32), dev(s["until"], np.int32)) for s in sets]
        self.sets = (N.ContactSet * len(sets))()
        for k, (s, (rowptr, venue, until)) in enumerate(zip(sets, self.keep)):
            self.sets[k].a_rowptr, self.sets[k].a_venue, self.sets[k].until = rowptr.data_ptr(), venue.data_ptr(), until.data_ptr()
            self.sets[k].n_venues = len(s["until"])
            self.sets[k].release = now + s["days"]
        self.err = torch.zeros(1, dtype=torch.int32, device=device)

    def until(self):
        torch.cuda.synchronize()
        return [u.cpu().numpy().view(np.uint32) for _, _, u in self.keep]

    def error(self):
        return int(self.err.item()) & 0xFFFFFFFF

    def mark(self, stage, threshold=THRESHOLD, shift=0):
        st = _shifted(stage, shift, self.device)
        return N.load().gj_contact_mark(len(stage), N.ptr(st), threshold, self.sets, len(self.sets), N.ptr(self.err),
                                        N.current_stream())

    def mask(self, stage, compliance, offset=0, threshold=THRESHOLD, shift=0):
        st = _shifted(stage, shift, self.device)
        q = _shifted(stage, shift, self.device, fill=float("nan"))
        rc = N.load().gj_contact_mask(len(stage), N.ptr(st), threshold, self.sets, len(self.sets), self.now, compliance,
                                      SEED, R.stream_of(POLICY), offset, N.ptr(q), N.ptr(self.err), N.current_stream())
        torch.cuda.synchronize()
        return rc, q.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _check(device, n, rng, compliances=(0.0, 0.5, 1.0), offsets=(0, 4, 3), long_row=True):
    sets, stage = _world(rng, n, long_row), _stages(rng, n)
    ref_until, ref_err = R.mark(stage, THRESHOLD, sets, NOW)
    assert ref_err == 0
    marked = [dict(s, until=u) for s, u in zip(sets, ref_until)]
    for shift in (0, 1):          # four agents per lane, then one agent per lane: the same bits
        run = Launch(device, sets)
        assert run.mark(stage, shift=shift) == 0
        got = run.until()
        for g, w, s in zip(got, ref_until, sets):
            assert np.array_equal(g, w), (n, shift)
            assert np.all(g >= s["until"]), "until decreased"
        for compliance, offset in itertools.product(compliances, offsets):
            u = R.uniforms(SEED, R.stream_of(POLICY), offset, n)
            ref_q, _ = R.mask(stage, THRESHOLD, marked, NOW, compliance, u)
            rc, q = run.mask(stage, compliance, offset=offset, shift=shift)
            assert rc == 0 and _same_bits(q, ref_q), (n, shift, compliance, offset)
            index = R.index_cases(stage, THRESHOLD)
            assert np.array_equal(q == 1.0, index)
            if compliance == 0.0:
                assert not (q == 2.0).any()
        assert all(np.array_equal(g, w) for g, w in zip(run.until(), ref_until)), "the mask wrote until"
        assert run.error() == 0
    return sets, stage, marked


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4099])
def test_kernels_against_the_restatement(device, n):
    """Both kernels, both forms, compliance 0 / 0.5 / 1, agent_offset 0 and 4 (quads share a Philox block) and 3 (the
    draw follows the global id: one agent per lane); stages at the threshold, NaN and +-inf; until preloaded below, at
    and above ``now``; agents with 0, 1, 2 and 70 rows; two sets of 14 and 7 days that share the agents."""
    rng = np.random.default_rng(1000 + n)
    sets, stage, marked = _check(device, n, rng)
    if n >= 255:      # the cases the parameters are there for do occur
        u = R.uniforms(SEED, R.stream_of(POLICY), 0, n)
        q, _ = R.mask(stage, THRESHOLD, marked, NOW, 0.5, u)
        comply = u < np.float32(0.5)
        assert 0.3 * n < comply.sum() < 0.7 * n and (q == 2.0).any() and (q[~comply] != 2.0).all()
        q1, _ = R.mask(stage, THRESHOLD, marked, NOW, 1.0, u)
        assert (q1 == 2.0).sum() > (q == 2.0).sum()
        assert not np.array_equal(u, R.uniforms(SEED, R.stream_of(POLICY), 3, n))


def test_a_second_trip_of_the_grid_stride_loops(device):
    """More agents than one pass of the capped grid holds, in either form (2048 workgroups of 256 lanes, four agents per
    lane in the vector form)."""
    rng = np.random.default_rng(5)
    _check(device, 4 * 2048 * 256 + 13, rng, compliances=(0.5,), offsets=(0,), long_row=False)


def test_permuted_agents_mark_the_same_venues(device):
    """The max is order-independent: with the agents renumbered ``until`` is identical, and ``qstate`` is permuted
    (compliance 1: the uniform, which follows the id, decides nothing)."""
    n = 1025
    rng = np.random.default_rng(77)
    sets, stage = _world(rng, n), _stages(rng, n)
    perm = rng.permutation(n)                       # new agent i is old agent perm[i]
    moved = []
    for s in sets:
        degree = np.diff(s["rowptr"])[perm]
        rows = [s["venue"][s["rowptr"][a]: s["rowptr"][a + 1]] for a in perm]
        moved.append(dict(s, rowptr=np.concatenate(([0], np.cumsum(degree))).astype(np.int32),
                          venue=np.concatenate(rows).astype(np.int32)))
    a, b = Launch(device, sets), Launch(device, moved)
    assert a.mark(stage) == 0 and b.mark(stage[perm]) == 0
    assert all(np.array_equal(x, y) for x, y in zip(a.until(), b.until()))
    (_, qa), (_, qb) = a.mask(stage, 1.0), b.mask(stage[perm], 1.0)
    assert _same_bits(qb, qa[perm]) and (qa == 2.0).any()


def test_bad_rows_set_the_error_bit_and_change_nothing_else(device):
    """A venue id outside the set and a row outside the edge list are skipped - never an index - and reported; every
    other edge is marked and read as before."""
    n = 257
    rng = np.random.default_rng(9)
    sets, stage = _world(rng, n), _stages(rng, n)
    stage[:] = np.where(np.arange(n) % 2 == 0, 5.0, 1.0)      # every other agent marks, the others walk in the mask
    for case in ("venue id", "negative venue id", "row"):
        bad = [dict(s, venue=s["venue"].copy(), rowptr=s["rowptr"].copy()) for s in sets]
        for parity in (0, 1):                                  # an index agent's edge and a walker's edge
            # (not the last agents: rowptr[n] is the edge count the rows are checked against)
            a = next(a for a in range(parity, n - 2, 2) if bad[0]["rowptr"][a + 1] > bad[0]["rowptr"][a] and a != n // 2)
            if case == "row":
                bad[0]["rowptr"][a + 1] = bad[0]["rowptr"][-1] + 5 if parity == 0 else -3
            else:
                bad[0]["venue"][bad[0]["rowptr"][a]] = len(bad[0]["until"]) if case == "venue id" else -1
        ref_until, ref_err = R.mark(stage, THRESHOLD, bad, NOW)
        run = Launch(device, bad)
        assert run.mark(stage) == 0
        assert all(np.array_equal(g, w) for g, w in zip(run.until(), ref_until)), case
        assert ref_err == R.ERR_ROWS and run.error() == N.GJ_CONTACT_ERR_ROWS, case
        run.err.zero_()
        marked = [dict(s, until=u) for s, u in zip(bad, ref_until)]
        u = R.uniforms(SEED, R.stream_of(POLICY), 0, n)
        ref_q, ref_err = R.mask(stage, THRESHOLD, marked, NOW, 1.0, u)
        rc, q = run.mask(stage, 1.0)
        assert rc == 0 and _same_bits(q, ref_q), case
        assert ref_err == R.ERR_ROWS and run.error() == N.GJ_CONTACT_ERR_ROWS, case


def test_every_documented_argument_error(device):
    n = 64
    rng = np.random.default_rng(3)
    sets, stage = _world(rng, n), _stages(rng, n)
    run = Launch(device, sets)
    before = run.until()
    lib, stream = N.load(), N.current_stream()
    st, q = _shifted(stage, 0, device), _shifted(stage, 0, device, fill=-7.0)
    err = N.ptr(run.err)

    def mark(n=n, stage=N.ptr(st), sets=run.sets, n_sets=2, err=err):
        return lib.gj_contact_mark(n, stage, THRESHOLD, sets, n_sets, err, stream)

    def mask(n=n, stage=N.ptr(st), sets=run.sets, n_sets=2, offset=0, qstate=N.ptr(q), err=err):
        return lib.gj_contact_mask(n, stage, THRESHOLD, sets, n_sets, NOW, 1.0, SEED, R.stream_of(POLICY), offset, qstate,
                                   err, stream)

    for call in (mark, mask):
        assert call(n=-1) == E_RANGE
        assert call(n_sets=0) == E_RANGE and call(n_sets=N.GJ_MAX_SETS + 1) == E_RANGE and call(n_sets=-1) == E_RANGE
        assert call(sets=None) == E_NULL and call(err=None) == E_NULL and call(stage=None) == E_NULL
        for field in ("a_rowptr", "a_venue", "until"):
            held = getattr(run.sets[1], field)
            setattr(run.sets[1], field, None)
            assert call() == E_NULL, field
            setattr(run.sets[1], field, held)
        for n_venues in (-1, 2 ** 31):
            held = run.sets[0].n_venues
            run.sets[0].n_venues = n_venues
            assert call() == E_RANGE
            run.sets[0].n_venues = held
    assert mask(qstate=None) == E_NULL and mask(offset=-1) == E_RANGE
    for release in (-1.0, float("nan")):
        held = run.sets[1].release
        run.sets[1].release = release
        assert mark() == E_RANGE and mask() == 0          # (the mask does not read it)
        run.sets[1].release = held
    assert (q.cpu().numpy() != -7.0).all()
    q.fill_(-7.0)
    # n == 0 launches nothing (NULL per-agent arrays are then accepted); twelve sets are
    assert mark(n=0, stage=None) == 0 and mask(n=0, stage=None, qstate=None) == 0
    twelve = (N.ContactSet * N.GJ_MAX_SETS)(*[run.sets[k % 2] for k in range(N.GJ_MAX_SETS)])
    assert mask(sets=twelve, n_sets=N.GJ_MAX_SETS) == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, run.until())) and run.error() == 0
