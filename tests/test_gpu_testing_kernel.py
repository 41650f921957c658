"""GPU: gj_testing_step and gj_adjoint_testing against their numpy restatement (tests/gj_testing_ref.py), bit for bit,
over the agent counts at which the launch changes form (a quad, a wave, a workgroup of 1024 lanes, several workgroups),
with aligned arrays (four agents per lane) and arrays one element into their allocation (one agent per lane)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gj_testing_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4 * 1024 + 3]
OFFSETS = [0, (1 << 32) + 3, 1 << 33]
SEED = 0x5EEDC0FFEE123
#: ages 0-4 and 50-59 are in no band
BANDS = {"5-18": 0.25, "18-50": 0.5, "60-100": 0.875}
DELAY16 = {d: s for d, s in zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0.5],
                                [0.05, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.15])}
CONFIGS = {
    "banded-16-delays": dict(probability=R.probability_table(BANDS), delay=DELAY16, isolation_days=2.5, compliance=0.7,
                             q_threshold=6.0, policy=3),
    "certain-at-once": dict(probability=np.ones(100, np.float32), delay=0, isolation_days=1.0, compliance=1.0,
                            q_threshold=np.inf, policy=0),
    "never": dict(probability=np.zeros(100, np.float32), delay={1: 0.5, 2: 0.5}, isolation_days=3.0, compliance=0.0,
                  q_threshold=np.inf, policy=1),
}
STATE = ("decided", "result_time", "positive", "isolate_until", "confirmed_time")
OUTPUTS = ("newly", "qstate", "flags", "counts")


class Shifted:
    """Device copies of host arrays, either as allocated (16-byte aligned: four agents per lane) or one element into a
    longer allocation (no alignment: one agent per lane)."""

    def __init__(self, device, shift):
        self.device, self.shift = device, int(shift)

    def __call__(self, a, dtype=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        if not self.shift:
            return torch.from_numpy(a).to(self.device)
        buf = torch.zeros(len(a) + 1, dtype=torch.from_numpy(a).dtype, device=self.device)
        buf[1:] = torch.from_numpy(a).to(self.device)
        return buf[1:]

    def full(self, n, value, dtype):
        return self(np.full(n, value, dtype=dtype))


def _c_tables(cfg):
    cum, days = R.delay_tables(cfg["delay"])
    t = N.TestingTables()
    t.probability[:] = [float(v) for v in cfg["probability"]]
    t.n_delays = len(days)
    for k in range(len(days)):
        t.delay_cum[k], t.delay_days[k] = float(cum[k]), float(days[k])
    return t, cum, days


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _launch(dev, state, cls, stage, time, cfg, now, active, offset, outputs=OUTPUTS, isolates=True, counts_start=(0, 0)):
    """One gj_testing_step on device copies of ``state`` (host arrays, left as they are).  Returns the updated state and
    the optional outputs asked for."""
    n = len(cls)
    tab, _, _ = _c_tables(cfg)
    d = {k: dev(state[k]) for k in STATE if isolates or k != "isolate_until"}
    out = {"newly": dev.full(n, np.nan, np.float32) if "newly" in outputs else None,
           "qstate": dev.full(n, np.nan, np.float32) if "qstate" in outputs and isolates else None,
           "flags": dev.full(n, 0xEE, np.uint8) if "flags" in outputs else None,
           "counts": torch.tensor(counts_start, dtype=torch.int64, device=dev.device) if "counts" in outputs else None}
    k, st, tm = dev(cls), dev(stage), dev(time)
    N.check(N.load().gj_testing_step(
        n, N.ptr(k), tab, N.ptr(st), N.ptr(tm), 4.0, int(active), now, cfg["q_threshold"],
        float(np.float64(now) + np.float64(cfg["isolation_days"])), cfg["compliance"], SEED,
        R.decide_stream(cfg["policy"]), R.comply_stream(cfg["policy"]), offset, N.ptr(d["decided"]),
        N.ptr(d["result_time"]), N.ptr(d["positive"]), N.ptr(d.get("isolate_until")), N.ptr(d["confirmed_time"]),
        N.ptr(out["newly"]), N.ptr(out["qstate"]), N.ptr(out["flags"]), N.ptr(out["counts"]), N.current_stream()),
        "gj_testing_step")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    new_state = {key: host(t) for key, t in d.items()}
    new_state["decided"] = new_state["decided"].view(np.uint32)
    # the inputs are only read
    assert _same_bits(host(st), stage) and _same_bits(host(tm), time) and np.array_equal(host(k), cls)
    return new_state, {key: host(t) for key, t in out.items()}


def _reference(state, cls, stage, time, cfg, now, active, offset, isolates=True):
    cum, days = R.delay_tables(cfg["delay"])
    state = {k: (None if v is None else v.copy()) for k, v in state.items()}
    out = R.step(state, cls, stage, time, probability=cfg["probability"], delay_cum=cum, delay_days=days,
                 stage_threshold=4.0, active=active, now=now, seed=SEED, policy=cfg["policy"], agent_offset=offset,
                 q_threshold=cfg["q_threshold"], isolation_days=cfg["isolation_days"] if isolates else None,
                 compliance=cfg["compliance"])
    return state, out


def _agents(n, rng):
    """Stages below, exactly at and above the threshold and NaN; infection times among which 0.0 and -0.0; ages in the
    bands and in the gaps.  The first agents are fixed by hand so that the smallest n too decides."""
    age = rng.integers(0, 100, n)
    stage = rng.choice(np.array([0, 2, 3, 4, 5, 6, 7, np.nan], dtype=np.float32), n, p=[0.3, 0.1, 0.1, 0.2, 0.1, 0.1, 0.05, 0.05])
    time = rng.choice(np.array([0.0, -0.0, 0.5, 1.0, 3.0], dtype=np.float32), n)
    hand = [(30, 4.0, 0.0), (70, np.nan, -0.0), (2, 5.0, 1.0), (55, 4.0, 0.5), (10, 3.0, 0.0)]
    for i, (a, st, t) in enumerate(hand[:n]):
        age[i], stage[i], time[i] = a, st, t
    cls = (rng.integers(0, 2, n) * 100 + age).astype(np.uint8)
    return cls, age, stage, time


def _check(got_state, got_out, ref_state, ref_out, isolates=True, counts_start=(0, 0), what=""):
    for key in STATE:
        if key == "isolate_until" and not isolates:
            continue
        assert _same_bits(got_state[key], ref_state[key]), (what, key)
    if got_out["newly"] is not None:
        assert _same_bits(got_out["newly"], ref_out["newly"]), what
    if got_out["qstate"] is not None:
        assert _same_bits(got_out["qstate"], ref_out["qstate"]), what
    if got_out["flags"] is not None:
        assert np.array_equal(got_out["flags"], ref_out["flags"]), what
    if got_out["counts"] is not None:
        assert got_out["counts"].tolist() == [counts_start[0] + ref_out["counts"][0], counts_start[1] + ref_out["counts"][1]], what


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_three_launches_against_the_restatement(device, n, config):
    """State, optional outputs and counts after each of three launches in a row - the second at a time at which results
    of the first fall due exactly, with new bits in some infection times (0.0 against -0.0) and equal bits in the others;
    the third after the policy's end, which reports and decides nothing - for both launch forms and agent offsets 0 and
    above 2^32."""
    cfg = CONFIGS[config]
    rng = np.random.default_rng(1000 + n)
    seen = {"due_exactly": 0, "redecided": 0, "isolating": 0, "confirmed": 0, "no_band_decisions": 0}
    for shift, offset in itertools.product((0, 1), OFFSETS):
        dev = Shifted(device, shift)
        cls, age, stage, time = _agents(n, rng)
        state = R.initial_state(n)
        for launch, (now, active) in enumerate([(1.0, True), (2.0, True), (16.5, False)]):
            if launch == 1:      # some infections are new ones (other bits), and some agents move to the threshold
                flip = rng.random(n) < 0.3
                time = np.where(flip & (time == 0), -time, time).astype(np.float32)
                stage = np.where(rng.random(n) < 0.2, np.float32(4.0), stage).astype(np.float32)
            ref_state, ref_out = _reference(state, cls, stage, time, cfg, now, active, offset)
            got_state, got_out = _launch(dev, state, cls, stage, time, cfg, now, active, offset, counts_start=(7, 11))
            _check(got_state, got_out, ref_state, ref_out, counts_start=(7, 11), what=(shift, offset, launch))
            if launch == 1:
                seen["due_exactly"] += int((state["result_time"] == np.float32(now)).sum())
                seen["redecided"] += int(((ref_out["flags"] & R.DECIDED) != 0)[state["decided"] != 0xFFFFFFFF].sum())
            if launch == 2:
                assert ref_out["counts"][1] == 0
            seen["isolating"] += int((ref_out["qstate"] == 3).sum())
            seen["confirmed"] += ref_out["counts"][0]
            gap = (age < 5) | ((age >= 50) & (age < 60))
            seen["no_band_decisions"] += int(((ref_out["flags"] & R.DECIDED) != 0)[gap].sum())
            if config == "banded-16-delays":
                assert not ref_state["positive"][gap].any()      # an age in no band is never positive
            state = ref_state
    if config == "certain-at-once":      # everybody at the threshold is confirmed in the deciding launch, and isolates
        assert seen["confirmed"] > 0 and seen["isolating"] > 0
    if config == "never":
        assert seen["confirmed"] == 0 and seen["isolating"] == 0
    if config == "banded-16-delays" and n >= 255:
        assert min(seen.values()) > 0, seen


@pytest.mark.parametrize("n", [5, 257, 4 * 1024 + 3])
def test_every_optional_output_may_be_null(device, n):
    """Each optional output NULL in turn, all of them NULL, and a policy that does not isolate (isolate_until and qstate
    NULL): the state is the same bits, and the outputs that are given are too."""
    cfg = CONFIGS["banded-16-delays"]
    rng = np.random.default_rng(77 + n)
    cls, age, stage, time = _agents(n, rng)
    start = R.initial_state(n)
    start["result_time"][::3] = 1.0      # results due in this launch ...
    start["positive"][::6] = 1.0      # ... half of them positive
    start["decided"][::3] = time[::3].view(np.uint32)
    for shift in (0, 1):
        dev = Shifted(device, shift)
        ref_state, ref_out = _reference(start, cls, stage, time, cfg, 1.0, True, 8)
        assert ref_out["counts"][0] > 0 and ref_out["counts"][1] > 0
        for missing in [(), *[(o,) for o in OUTPUTS], OUTPUTS]:
            given = tuple(o for o in OUTPUTS if o not in missing)
            got_state, got_out = _launch(dev, start, cls, stage, time, cfg, 1.0, True, 8, outputs=given)
            assert all(got_out[o] is None for o in missing)
            _check(got_state, got_out, ref_state, ref_out, what=(shift, missing))
        plain_state, plain_out = _reference(start, cls, stage, time, cfg, 1.0, True, 8, isolates=False)
        got_state, got_out = _launch(dev, start, cls, stage, time, cfg, 1.0, True, 8, isolates=False)
        assert got_out["qstate"] is None and "isolate_until" not in got_state
        _check(got_state, got_out, plain_state, plain_out, isolates=False, what=(shift, "no isolation"))


def test_a_launch_in_which_nothing_happens_writes_nothing(device):
    """Nobody at the threshold and no result due: every state array keeps its bits, a NaN payload included."""
    n = 1025
    state = R.initial_state(n)
    state["confirmed_time"][:] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    state["positive"][:] = 5.0
    state["result_time"][::2] = np.nan      # never due
    cls, stage, time = np.zeros(n, np.uint8), np.full(n, 3.0, np.float32), np.zeros(n, np.float32)
    for shift in (0, 1):
        got_state, got_out = _launch(Shifted(device, shift), state, cls, stage, time, CONFIGS["certain-at-once"], 4.0, True, 0)
        for key in STATE:
            assert _same_bits(got_state[key], state[key]), key
        assert not got_out["flags"].any() and not got_out["newly"].any() and not got_out["qstate"].any()
        assert got_out["counts"].tolist() == [0, 0]


# ---- the adjoint ---------------------------------------------------------------------------------------------------------
def _same_numbers(a, b):
    """Equal bits where the values are numbers, NaN where the other is NaN (a NaN's payload is not specified)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _adjoint(dev, flags, stage, g_y, g_row, band, n_bands, outputs=True):
    from grad_june_amd.groups import SeedPlan

    n = len(flags)
    plan = SeedPlan(torch.from_numpy(np.ascontiguousarray(band, np.int32)).to(dev.device), n_bands, device=dev.device)
    fl, st, gy, b = dev(flags), dev(stage), dev(g_y), dev(band, np.int32)
    grow = None if g_row is None else torch.tensor([g_row], dtype=torch.float32, device=dev.device)
    contrib = dev.full(max(1, n), np.nan, np.float64)
    partial = torch.full((max(1, plan.n_chunks),), float("nan"), dtype=torch.float64, device=dev.device)
    sums = torch.full((n_bands,), float("nan"), dtype=torch.float64, device=dev.device)
    g_stage = dev.full(n, np.nan, np.float32) if outputs else None
    g_y_in = dev.full(n, np.nan, np.float32) if outputs else None
    N.check(N.load().gj_adjoint_testing(n, N.ptr(fl), N.ptr(st), N.ptr(gy), N.ptr(grow), N.ptr(b), n_bands,
                                        C.byref(plan.c), N.ptr(contrib), N.ptr(partial), N.ptr(sums), N.ptr(g_stage),
                                        N.ptr(g_y_in), N.current_stream()), "gj_adjoint_testing")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(sums), host(g_stage), host(g_y_in)


@pytest.mark.parametrize("n", COUNTS)
def test_adjoint_against_the_restatement(device, n):
    """The per-band sums equal the fp64 restatement summed in the kernels' fixed order - bit for bit, and from launch to
    launch - and the stage gradient and the cotangent handed on match per agent, in both launch forms; g_y and g_row
    NULL are zeros; labels outside [0, n_bands) give no term.  Bands of several chunks at the largest count."""
    rng = np.random.default_rng(500 + n)
    n_bands = 3
    flags = rng.choice(np.array([0, R.DECIDED, R.DECIDED | R.POSITIVE, R.DUE, R.DUE | R.POSITIVE, R.DECIDED | R.DUE,
                                 R.DECIDED | R.DUE | R.POSITIVE], np.uint8), n)
    stage = rng.choice(np.array([4, 5, 6, 7, 3, 0, np.nan], np.float32), n, p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05])
    g_y = rng.normal(size=n).astype(np.float32) * np.float32(3.0)
    band = rng.choice(np.array([0, 0, 0, 1, 2, -1, 3, 1 << 20], np.int32), n)      # band 0 holds several chunks at 4099
    if n:
        flags[0], stage[0], band[0] = R.DECIDED | R.DUE | R.POSITIVE, 4.0, 0
    for shift in (0, 1):
        dev = Shifted(device, shift)
        for gy, grow in ((g_y, 0.75), (g_y, None), (None, -2.0), (None, None)):
            ref = R.adjoint(flags, stage, np.zeros(n, np.float32) if gy is None else gy, 0.0 if grow is None else grow,
                            band, n_bands)
            got = _adjoint(dev, flags, stage, gy, grow, band, n_bands)
            assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), (shift, got[0], ref[0])
            assert _same_numbers(got[1], ref[1]) and _same_numbers(got[2], ref[2]), shift
            again = _adjoint(dev, flags, stage, gy, grow, band, n_bands, outputs=False)
            assert again[1] is None and again[2] is None
            assert np.array_equal(again[0].view(np.uint64), got[0].view(np.uint64))
    decided = (flags & R.DECIDED) != 0
    assert (ref[1][~decided] == 0).all() and (ref[2][decided] == 0).all()
