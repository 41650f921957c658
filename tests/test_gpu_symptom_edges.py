"""GPU: the symptom kernels at the edges - gj_symptoms_update, gj_adjoint_symptoms and gj_symptoms_step_stats on a few
hundred hand-made agents, against oracle.symptoms_update and oracle.adjoint_symptoms evaluated in fp64 on the fp32
inputs, with the randomness injected (progresses, dwell).

The agents: time_to_next_stage exactly `time` and one ulp on either side; every current stage 0 .. n_stages - 1 with the
next one behind it, so that the stage after the move is 1, the two ends 2 and n_stages - 2 of the range in which a draw
is due, and n_stages - 1; the last stage with its time up (it does not move); a next stage that is not an integer (no
draw is due on it); a new infection of an agent that is due, of a recovered one and of a susceptible one; both outcomes
of the draw.  Times are dyadic, so that time_to_next_stage + new_infected * (time - time_to_next_stage) is exact and the
fp64 oracle takes the fp32 kernel's branch; the forward values are then small integers and ONE sum with the dwell time,
which fp32 and fp64 round alike: they are compared exactly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gj_oracle as O
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

N_STAGES = 8
TIME = 7.5
U = 2.0 ** -24
F32 = np.float32
FIELDS = ("cur", "nxt", "ttn")
OUTS = ("g_cur_in", "g_nxt_in", "g_ttn_in", "g_new")


def _ulp(x, up):
    return float(np.nextafter(F32(x), F32(np.inf if up else -np.inf), dtype=F32))


@functools.lru_cache(maxsize=None)
def agents():
    """The hand-made agents (fp32 arrays, left unchanged) and the cotangents of the adjoint."""
    rows = []                                        # (kind, cur, nxt, ttn, new, progresses)
    for ttn in (TIME, _ulp(TIME, False), _ulp(TIME, True), 0.0, 2.25, 7.25, 30.0):
        for cur in range(N_STAGES):
            for pr in (0.0, 1.0):
                rows.append(("walk", float(cur), float(min(cur + 1, N_STAGES - 1)), ttn, 0.0, pr))
    for cur in range(N_STAGES):                      # a new infection whatever the stage: next = 2, due now
        for ttn in (2.25, TIME, 30.0, _ulp(TIME, True)):
            for pr in (0.0, 1.0):
                rows.append(("new", float(cur), float(min(cur + 1, N_STAGES - 1)), ttn, 1.0, pr))
    for new in (0.0, 1.0):                           # recovered (stage 0, nothing ahead) and susceptible (1)
        for pr in (0.0, 1.0):
            rows.append(("recovered", 0.0, 0.0, 2.25, new, pr))
            rows.append(("recovered", 0.0, 0.0, 30.0, new, pr))
            rows.append(("susceptible", 1.0, 1.0, 30.0, new, pr))
    for nxt in (2.5, _ulp(3.0, True), _ulp(3.0, False), 6.5, 0.5, -1.0, 9.0):      # not an integer, or outside the table
        for pr in (0.0, 1.0):
            rows.append(("fraction", 1.0, nxt, 2.25, 0.0, pr))
    for pr in (0.0, 1.0):                            # the last stage with its time up
        rows.append(("last", float(N_STAGES - 1), float(N_STAGES - 1), 2.25, 0.0, pr))
        rows.append(("last", float(N_STAGES - 1), float(N_STAGES - 1), TIME, 1.0, pr))
    n = len(rows)
    g = np.random.default_rng(31)
    col = lambda i: np.array([r[i] for r in rows], dtype=F32)
    a = {"kinds": [r[0] for r in rows], "n": n, "cur": col(1), "nxt": col(2), "ttn": col(3), "new": col(4),
         "progresses": col(5), "dwell": g.uniform(0.5, 9.0, n).astype(F32),
         "cls": g.integers(0, 200, n).astype(np.uint8)}
    for k in ("g_cur", "g_nxt", "g_ttn"):
        a[k] = (g.uniform(0.1, 1.0, n) * g.choice([-1.0, 1.0], n)).astype(F32)
    return a


def t64(v):
    return torch.from_numpy(np.ascontiguousarray(v)).double()


@functools.lru_cache(maxsize=None)
def oracle():
    """the fp64 oracle's forward (cast to fp32: exact, see above) and adjoint on the agents"""
    a = agents()
    fwd = O.symptoms_update(None, t64(a["cur"]), t64(a["nxt"]), t64(a["ttn"]), t64(a["new"]), TIME, N_STAGES,
                            t64(a["progresses"]), t64(a["dwell"]))
    adj = O.adjoint_symptoms(t64(a["cur"]), t64(a["nxt"]), t64(a["ttn"]), t64(a["new"]), TIME, N_STAGES,
                             t64(a["progresses"]), t64(a["g_cur"]), t64(a["g_nxt"]), t64(a["g_ttn"]), t64(a["dwell"]))
    return dict(zip(FIELDS, (v.numpy() for v in fwd))), dict(zip(OUTS, (v.numpy() for v in adj)))


def adjoint_restated(a, dtype):
    """The adjoint in ``dtype`` in the kernel's order of operations (csrc/gj_agent.h, k_adjoint_symptoms), and per
    output the sum of the absolute values of the terms it adds - what a rounding error is relative to."""
    c0, x0, t0, nw, d = (a[k].astype(dtype) for k in ("cur", "nxt", "ttn", "new", "dwell"))
    gc, gx, gt = (a[k].astype(dtype) for k in ("g_cur", "g_nxt", "g_ttn"))
    time, one = dtype(TIME), dtype(1.0)
    x1 = x0 + nw * (dtype(2.0) - x0)
    t1 = t0 + nw * (time - t0)
    moving = (time >= t1) & (c0 < dtype(N_STAGES - 1))
    m = moving.astype(dtype)
    c1 = c0 - (c0 - x1) * m
    s = np.clip(np.nan_to_num(c1, nan=0.0).astype(np.int64), 0, N_STAGES - 1)
    due = moving & (s >= 2) & (s <= N_STAGES - 2) & (c1 == s.astype(dtype))
    sf = np.maximum(s, 1).astype(dtype)
    onward = a["progresses"] != 0
    t_d, t_on, t_off = gt * d / sf, gx / sf, gx * x1 / sf
    gc1 = gc + np.where(due, t_d, 0)
    gc1 = gc1 + np.where(due & onward, t_on, 0) - np.where(due & ~onward, t_off, 0)
    scale_c = np.abs(gc) + np.where(due, np.abs(t_d) + np.where(onward, np.abs(t_on), np.abs(t_off)), 0)
    gx1 = np.where(due & ~onward, 0, gx)
    scale_x = np.abs(gx1) + scale_c * m
    gx1 = gx1 + gc1 * m
    out = {"g_cur_in": gc1 * (one - m), "g_nxt_in": gx1 * (one - nw), "g_ttn_in": gt * (one - nw),
           "g_new": gx1 * (dtype(2.0) - x0) + gt * (time - t0)}
    scale = {"g_cur_in": scale_c, "g_nxt_in": scale_x, "g_ttn_in": np.abs(gt),
             "g_new": scale_x * np.abs(dtype(2.0) - x0) + np.abs(gt * (time - t0))}
    return out, scale


@functools.lru_cache(maxsize=None)
def adjoint_tolerance():
    """(k_ref, scale): the fp32 restatement's largest error against the fp64 oracle in units of u * scale - measured
    here, on the CPU, before any kernel result is looked at; the kernel is held to twice that."""
    a = agents()
    _, want = oracle()
    r64, scale = adjoint_restated(a, np.float64)
    r32, _ = adjoint_restated(a, np.float32)
    k_ref = 0.0
    for k in OUTS:
        assert np.allclose(r64[k], want[k], rtol=1e-14, atol=1e-300), k       # the restatement IS the oracle's adjoint
        err = np.abs(r32[k].astype(np.float64) - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / (U * scale[k]))
        k_ref = max(k_ref, float(q.max()))
    return k_ref, scale


def params(time=TIME):
    p = N.SymptomsParams()
    p.n_stages, p.time, p.seed, p.step, p.agent_offset = N_STAGES, time, 1, 2, 0
    return p


def dev(v, device):
    return torch.from_numpy(np.ascontiguousarray(v)).to(device)


def update(device, a, idx=None, fused=False):
    """gj_symptoms_update (or gj_symptoms_step_stats) on the arrangement ``idx``; the three arrays on the CPU."""
    idx = np.arange(a["n"]) if idx is None else idx
    n = len(idx)
    t = {k: dev(a[k][idx], device) for k in FIELDS + ("new", "progresses", "dwell", "cls")}
    p = params()
    lib = N.load()
    if fused:
        inf = dev((a["cur"][idx] >= 2).astype(F32), device)
        out = torch.zeros(5, dtype=torch.float64, device=device)
        edges = (C.c_int32 * 4)(0, 18, 65, 100)
        N.check(lib.gj_symptoms_step_stats(n, N.ptr(t["cls"]), N.ptr(t["new"]), N.ptr(t["cur"]), N.ptr(t["nxt"]),
                                           N.ptr(t["ttn"]), C.byref(p), N.ptr(t["progresses"]), N.ptr(t["dwell"]),
                                           N.ptr(inf), 3, edges, N_STAGES - 1, N.ptr(out), N.current_stream()),
                "gj_symptoms_step_stats")
    else:
        N.check(lib.gj_symptoms_update(n, N.ptr(t["cls"]), N.ptr(t["new"]), N.ptr(t["cur"]), N.ptr(t["nxt"]), N.ptr(t["ttn"]),
                                       C.byref(p), N.ptr(t["progresses"]), N.ptr(t["dwell"]), N.current_stream()),
                "gj_symptoms_update")
    torch.cuda.synchronize()
    got = {k: t[k].cpu().numpy() for k in FIELDS}
    if fused:
        got["stats"] = out.cpu().numpy()
    return got


def adjoint(device, a, with_time_out=True):
    n = a["n"]
    t = {k: dev(a[k], device) for k in FIELDS + ("new", "progresses", "dwell", "cls", "g_cur", "g_nxt", "g_ttn")}
    out = {k: torch.full((n,), -77.0, device=device) for k in OUTS}
    p = params()
    N.check(N.load().gj_adjoint_symptoms(
        n, N.ptr(t["cls"]), N.ptr(t["new"]), N.ptr(t["cur"]), N.ptr(t["nxt"]), N.ptr(t["ttn"]), C.byref(p),
        N.ptr(t["progresses"]), N.ptr(t["dwell"]), N.ptr(t["g_cur"]), N.ptr(t["g_nxt"]), N.ptr(t["g_ttn"]),
        N.ptr(out["g_cur_in"]), N.ptr(out["g_nxt_in"]), N.ptr(out["g_ttn_in"]) if with_time_out else None,
        N.ptr(out["g_new"]), N.current_stream()), "gj_adjoint_symptoms")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(v):
    return np.ascontiguousarray(v).view(np.int32)


@pytest.fixture(scope="module")
def first(device):
    return update(device, agents())


def test_the_agents_cover_the_edges():
    a = agents()
    fwd, _ = oracle()
    moved = fwd["cur"] != a["cur"]
    t1 = a["ttn"] + a["new"] * (F32(TIME) - a["ttn"])
    moving = (F32(TIME) >= t1) & (a["cur"] < N_STAGES - 1)
    assert not (moved & ~moving).any()
    for ttn in (TIME, _ulp(TIME, False), _ulp(TIME, True)):
        at = (a["ttn"] == F32(ttn)) & (a["new"] == 0) & (a["cur"] < N_STAGES - 1) & (a["cur"] != a["nxt"])
        assert at.sum() >= 14 and (moved[at] == (ttn <= TIME)).all()        # time >= time_to_next_stage, not >
    last = a["cur"] == N_STAGES - 1
    assert last.sum() >= 10 and not moved[last].any()
    after = set(fwd["cur"][moved].tolist())
    assert {1.0, 2.0, float(N_STAGES - 2), float(N_STAGES - 1)} <= after
    # a draw is due exactly on the stages 2 .. n_stages - 2 after the move: there the time grows by the dwell time
    drew = fwd["ttn"] != t1
    whole = fwd["cur"] == np.floor(fwd["cur"])
    assert np.array_equal(drew, moving & whole & (fwd["cur"] >= 2) & (fwd["cur"] <= N_STAGES - 2))
    for s in (2.0, float(N_STAGES - 2)):
        assert (drew & (fwd["cur"] == s) & (a["progresses"] == 0)).any() and (drew & (fwd["cur"] == s) & (a["progresses"] == 1)).any()
    frac = np.array([k == "fraction" for k in a["kinds"]])
    assert moved[frac].all() and not drew[frac & ~whole].any() and (frac & ~whole).sum() >= 8
    already_due = (a["new"] == 1) & (a["cur"] >= 1) & (a["ttn"] <= TIME) & (a["cur"] < N_STAGES - 1)
    assert already_due.sum() >= 12 and (fwd["cur"][already_due] == 2).all() and drew[already_due].all()
    rec = np.array([k == "recovered" for k in a["kinds"]])
    assert set(a["new"][rec].tolist()) == {0.0, 1.0} and (fwd["cur"][rec & (a["new"] == 1)] == 2).all()
    assert (fwd["cur"][rec & (a["new"] == 0)] == 0).all()


def test_update_is_the_oracle_exactly(first):
    a = agents()
    fwd, _ = oracle()
    for k in FIELDS:
        want = fwd[k].astype(F32)
        assert np.array_equal(want.astype(np.float64), fwd[k]) or k == "ttn"
        assert np.array_equal(bits(first[k] + F32(0.0)), bits(want + F32(0.0))), (k, np.nonzero(first[k] != want)[0][:10].tolist())


def test_adjoint_against_fp64(device):
    """Every output of every agent within 2 * k_ref * u * (the sum of the absolute terms of the output), k_ref the fp32
    restatement's largest error against the fp64 oracle in those units.  Measured: k_ref 1.80 on the CPU; the kernel
    on an MI355X: g_current_in 0, g_next_in 1.51, g_time_in 0, g_new_infected 1.80 (the restatement's arithmetic)."""
    a = agents()
    _, want = oracle()
    k_ref, scale = adjoint_tolerance()
    got = adjoint(device, a)
    worst = {}
    for k in OUTS:
        err = np.abs(got[k].astype(np.float64) - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / (U * scale[k]))
        worst[k] = float(q.max())
    print(f"k_ref (fp32 restatement against fp64) = {k_ref:.2f}; the kernel's max err / (u * scale) per output:",
          {k: round(v, 2) for k, v in worst.items()})
    assert k_ref > 0
    for k in OUTS:
        assert worst[k] <= 2.0 * k_ref, k
    # without g_time_in the other three are the same bits
    less = adjoint(device, a, with_time_out=False)
    assert (less["g_ttn_in"] == -77.0).all()
    for k in ("g_cur_in", "g_nxt_in", "g_new"):
        assert np.array_equal(bits(less[k]), bits(got[k])), k


@pytest.mark.parametrize("n", [5, 1027])
def test_fused_pass_gives_the_update_s_bits(device, first, n):
    a = agents()
    idx = (np.arange(n) * 3 + 1) % a["n"]
    alone, fused = update(device, a, idx), update(device, a, idx, fused=True)
    for k in FIELDS:
        assert np.array_equal(bits(alone[k]), bits(first[k][idx])), k
        assert np.array_equal(bits(fused[k]), bits(alone[k])), k
    assert fused["stats"][4] == float((alone["cur"] == N_STAGES - 1).sum())


def test_a_nan_stage_stays_with_its_agent(device, first):
    """A NaN current or next stage ((int)NaN before the clamp): every other agent's output keeps its bits, and the NaN
    agent's three values are NaN or unchanged - the oracle gives NaN in all three (its masks multiply by the stage),
    the kernel moves nothing on a NaN current stage and lets a NaN next stage become the current one."""
    a = agents()
    poisoned = dict(a)
    where = {"cur": np.arange(3, a["n"], 41), "nxt": np.arange(17, a["n"], 43)}
    for k, at in where.items():
        poisoned[k] = a[k].copy()
        poisoned[k][at] = np.nan
    bad = np.zeros(a["n"], dtype=bool)
    bad[np.concatenate(list(where.values()))] = True
    got = update(device, poisoned)
    fwd = O.symptoms_update(None, *[t64(poisoned[k]) for k in ("cur", "nxt", "ttn", "new")], TIME, N_STAGES,
                            t64(poisoned["progresses"]), t64(poisoned["dwell"]))
    # "unchanged": the values after the new infection alone (next += new * (2 - next), time += new * (now - time))
    unchanged = {"cur": poisoned["cur"], "nxt": poisoned["nxt"] + poisoned["new"] * (F32(2.0) - poisoned["nxt"]),
                 "ttn": poisoned["ttn"] + poisoned["new"] * (F32(TIME) - poisoned["ttn"])}
    for k, o in zip(FIELDS, fwd):
        o = o.numpy()
        assert np.array_equal(bits(got[k][~bad]), bits(first[k][~bad])), k
        assert np.array_equal(o[~bad].astype(F32) + F32(0.0), first[k][~bad] + F32(0.0)), k
        assert np.isnan(o[bad]).all(), k
        assert (np.isnan(got[k][bad]) | (bits(got[k][bad]) == bits(unchanged[k][bad]))).all(), k
    g = adjoint(device, poisoned)
    clean = adjoint(device, a)
    for k in OUTS:
        assert np.array_equal(bits(g[k][~bad]), bits(clean[k][~bad])), k
