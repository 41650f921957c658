"""CPU: the fp64 reference of the infection sampler and its adjoint (tests/gj_sampler_ref.py) and its bound B are sound -
the same formulas run in fp32 numpy stay within K_REF * B of it on every point.

Measured on the CPU, maximum of err / B over the 3294 points of the six launches (dt = 1/24, 0.25, 0.5, 1 with the grid,
0.01 and 2 with the named points only):  x_out 0.43 (ts * dt = 0.01, draws (5, 0.01)),
grad_susc_out 0.47 (ts * dt = 0.1, draws (0.3, 0.31)), grad_time_out 0 (exact).  K_REF = 0.5 is that maximum rounded up to the next tenth: the one
constant taken from a measurement, and the measurement is of the restatement, not of a kernel.  The loose points (B
above 1 % of |ts_bar|) are 24 %, 31 %, 30 % and 23 % of the grids' points with a non-zero reference, all of them at
ts * dt < 1e-3, above 10, or with a draw pair whose softmax term y0 * y1 is below 1e-33; the cap is 35 %.  The
decision is unsafe on 4 of the 3294 points (ts = 100 and +inf at dt = 2: p is below fp32's range altogether).

The step's a7 (prob_reference / prob_f32) and the in-step points (step_points) are checked at the end of the file: the
fp32 restatement of p reaches 0.453 of its bound, and 0.27 % of the step points are unsafe once p is 2 ulp off."""
import math

import numpy as np
import pytest
import torch

import gj_oracle as O
import gj_sampler_ref as R
import gj_seed_ref as S


@pytest.fixture(scope="module")
def sets():
    out = []
    for pts in R.all_point_sets():
        f32 = R.adjoint(pts, np.float32)
        out.append({"pts": pts, "f32": f32, "ref": R.reference(pts, nu=f32["nu"])})
    return out


def kind_mask(pts, kind):
    return np.array([k == kind for k in pts["kinds"]])


def test_fp32_restatement_within_k_ref_of_the_reference(sets):
    measured = {k: 0.0 for k in R.OUTPUTS}
    for s in sets:
        pts, ref = s["pts"], s["ref"]
        # on the safe points the fp32 restatement took the fp64 decision
        assert np.array_equal(s["f32"]["nu"][ref["safe"]], ref["nu64"][ref["safe"]])
        for k in R.OUTPUTS:
            q, ok = R.excess(s["f32"][k], ref[k], ref["bound"][k])
            assert ok.all(), (pts["dt"], k, np.nonzero(~ok)[0].tolist())
            v, i = R.worst(q)
            if v > measured[k]:
                measured[k] = v
                print(f"dt {pts['dt']:.4g} {k}: err / B = {v:.3f} at point {i} ({pts['kinds'][i]}, ts = {float(ref['ts'][i]):.6g}, "
                      f"p = {float(ref['p'][i]):.9g}, draws ({float(pts['e0'][i]):.3g}, {float(pts['e1'][i]):.3g}))")
    k_ref = max(measured.values())
    print("fp32 restatement, max err / B per output:", {k: round(v, 3) for k, v in measured.items()})
    print(f"K_ref measured {k_ref:.3f}, asserted {R.K_REF}")
    assert measured["grad_time"] == 0.0
    assert k_ref <= R.K_REF
    assert math.ceil(10 * k_ref) / 10 == R.K_REF       # the constant is the measurement rounded up, not a looser one


def test_loose_and_unsafe_shares(sets):
    n = unsafe = nonzero_all = loose_all = 0
    for s in sets:
        pts, ref, f32 = s["pts"], s["ref"], s["f32"]
        # the condition is asserted with the fp32 restatement: a point is loose where B exceeds 1 % of the fp64 |ts_bar|
        nonzero = ref["ts_bar"] != 0
        share = ref["loose"].sum() / nonzero.sum()
        print(f"dt {pts['dt']:.4g}: {pts['n']} points, {int(nonzero.sum())} with a non-zero reference, loose share {share:.3f}, "
              f"unsafe {int((~ref['safe']).sum())}")
        assert share <= R.MAX_LOOSE_SHARE, pts["dt"]
        # every loose point is at an extreme of ts * dt, or its softmax term y0 * y1 is at the bottom of fp32's range (the
        # floor 2^-126 is 1 % of it below 1e-36, and S / |nu_bar| multiplies that)
        a = np.abs(ref["ts"].astype(np.float64)) * pts["dt"]
        tiny = ref["y0"] * ref["y1"] < 1e-33
        assert (~ref["loose"] | (a < 1e-3) | (a > 10) | tiny).all()
        # ... and the fp32 restatement keeps the sign of every non-zero reference it does not flush to 0
        assert (f32["ts_bar"].astype(np.float64) * ref["ts_bar"] >= 0).all()
        n, unsafe = n + pts["n"], unsafe + int((~ref["safe"]).sum())
        nonzero_all, loose_all = nonzero_all + int(nonzero.sum()), loose_all + int(ref["loose"].sum())
    print(f"all launches: loose {loose_all} of {nonzero_all} = {loose_all / nonzero_all:.3f}, unsafe {unsafe} of {n}")
    assert unsafe <= R.MAX_UNSAFE_SHARE * n


def test_the_grid_is_the_issues(sets):
    for s in sets[:len(R.DTS)]:
        pts, ref = s["pts"], s["ref"]
        g = kind_mask(pts, "grid")
        assert g.sum() == (len(R.clamp_edges()) + len(R.CORE) + len(R.ABSOLUTE)) * len(R.DRAWS) * len(R.SUSC)
        ts = ref["ts"][g]
        for edge in (R.TS_LO, R.TS_HI):       # below, at and just above both bounds - as fp32 PRODUCTS, susc0 = 0.3 included
            for s0 in (np.float32(0.3), np.float32(1.0)):
                m = pts["susc0"][g] == s0
                assert (ts[m] == edge).any() and (ts[m] == R._na(edge, False)).any() and (ts[m] == R._na(edge, True)).any()
        assert (ts == np.float32(1e30)).any() and (ts < 0).any()
        core = (ts * np.float32(pts["dt"]) >= 0.0099) & (ts * np.float32(pts["dt"]) <= 5.01)
        assert core.sum() >= len(R.CORE) * len(R.DRAWS) * 2
        # both decisions, and the subgradient's three cases: the tie susc0 == nu and both sides of it
        x = pts["susc0"][g].astype(np.float64) - ref["nu"][g]
        assert (x > 0).any() and (x == 0).any() and (x < 0).any()
        assert set(np.unique(ref["h"][g]).tolist()) == {0.0, 0.5, 1.0}
        for s0, nu in ((0.0, 0.0), (1.0, 1.0)):
            tie = (pts["susc0"][g] == s0) & (ref["nu"][g] == nu)
            assert tie.any() and (ref["h"][g][tie] == 0.5).all()


def test_inside_mask_is_the_fp32_comparison(sets):
    """ts == 1e-6f is inside; a double constant 1e-6 would put it outside (1e-6f < 1e-6), where ts_bar is 0."""
    assert float(R.TS_LO) < 1e-6
    pts, ref = sets[3]["pts"], sets[3]["ref"]
    at = (ref["ts"] == R.TS_LO) & (pts["susc0"] == 1.0)
    assert at.any() and ref["inside"][at].all()
    assert (ref["ts_bar"][at] != 0).all()
    for ts, inside in ((R._na(R.TS_LO, False), False), (R._na(R.TS_LO, True), True), (R._na(R.TS_HI, False), True),
                       (R.TS_HI, True), (R._na(R.TS_HI, True), False), (np.float32(1e30), False)):
        m = ref["ts"] == ts
        assert m.any() and (ref["inside"][m] == inside).all(), ts
        if not inside:
            assert (ref["ts_bar"][m] == 0).all() and (sets[3]["f32"]["ts_bar"][m] == 0).all()


def test_named_points(sets):
    by_dt = {round(s["pts"]["dt"], 4): s for s in sets}
    # the exact tie: p == 0.5 after rounding at dt = 1, e0 == e1: not infected, in fp32 and by the reference's rule
    s = by_dt[1.0]
    m = kind_mask(s["pts"], "tie") & (s["pts"]["susc0"] == 1.0)
    _, _, p32 = R.epilogue(s["pts"], np.float32)
    assert (p32[m] == 0.5).all() and s["ref"]["tie"][m].all() and (s["f32"]["nu"][m] == 0).all() and (s["ref"]["nu"][m] == 0).all()
    assert (s["f32"]["y0"][m] == s["f32"]["y1"][m]).all()
    # p == 1 after rounding (ts = 1e-6, dt = 0.01) and p == 0 (ts = 100, dt = 2): d nu / d p is 0 by the library's rule.
    # torch's autograd gives NaN there (0 * inf); include/gradjune_hip.h documents 0.
    for dt, kind, p in ((0.01, "p_one", 1.0), (2.0, "p_zero", 0.0)):
        s = by_dt[dt]
        m = kind_mask(s["pts"], kind)
        _, _, p32 = R.epilogue(s["pts"], np.float32)
        assert m.any() and (p32[m] == p).all() and s["ref"]["inside"][m].all()
        assert (s["f32"]["dnu_dp"][m] == 0).all() and (s["f32"]["x_out"][m] == 0).all()
        y0, y1 = S.softmax_terms(p32[m], s["pts"]["e0"][m], s["pts"]["e1"][m], np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.isnan(-(y0 * y1 / np.float32(0.1)) * (np.float32(1) / p32[m] + np.float32(1) / (np.float32(1) - p32[m]))).all()
    for s in sets:
        pts, ref, f32 = s["pts"], s["ref"], s["f32"]
        for kind in ("nan_acc", "inf_acc", "draw0"):
            m = kind_mask(pts, kind)
            assert m.any()
            nan_ts = m & np.isnan(ref["ts"]) | m & (kind == "draw0")      # (acc = +inf is clamped to 100: it may infect)
            for r in (ref, f32):
                assert (r["ts_bar"][m] == 0).all() and (r["x_out"][m] == 0).all() and (r["nu"][nan_ts] == 0).all(), kind
        m = kind_mask(pts, "nan_acc") | kind_mask(pts, "inf_acc")
        assert np.isnan(ref["grad_susc"][m]).all()          # g_susc * h + 0 * acc: autograd's own 0 * inf
        m = kind_mask(pts, "draw_sub")
        assert np.isfinite(ref["x_out"][m]).all() and np.isfinite(f32["x_out"][m]).all()


def test_null_cotangents_are_zeros(sets):
    pts = sets[3]["pts"]
    for k in R.COTANGENTS:
        zeroed = dict(pts)
        zeroed[k] = np.zeros_like(pts[k])
        a, b = R.adjoint(pts, np.float32, drop=(k,)), R.adjoint(zeroed, np.float32)
        for o in R.OUTPUTS:
            assert np.array_equal(a[o], b[o], equal_nan=True)


# ---- the forward ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd():
    fp = R.forward_points()
    nu64, safe, ruled = R.forward_decision(fp)
    oracle = O.sample_infected(torch.from_numpy(fp["p"]), torch.from_numpy(np.stack([fp["e0"], fp["e1"]]))).numpy()
    return {"fp": fp, "nu64": nu64, "safe": safe, "ruled": ruled, "oracle": oracle}


def test_forward_decisions(fwd):
    fp, safe, ruled = fwd["fp"], fwd["safe"], fwd["ruled"]
    unsafe = ~safe & ~ruled
    print(f"forward: {fp['n']} points, unsafe {int(unsafe.sum())} ({unsafe.mean():.4f}), ruled {int(ruled.sum())}")
    assert unsafe.mean() <= R.MAX_UNSAFE_SHARE
    assert (fwd["nu64"][safe] == 0).any() and (fwd["nu64"][safe] == 1).any()
    # the fp32 restatement and torch's fp32 ops take the fp64 decision on every safe point, and the value is exactly 0 or 1
    assert np.array_equal(S.decisions(fp["p"], fp["e0"], fp["e1"])[safe], fwd["nu64"][safe])
    assert np.array_equal(fwd["oracle"][safe].astype(np.float64), fwd["nu64"][safe])
    tie = kind_mask(fp, "tie")
    assert tie.sum() == 3 and safe[tie].all() and (fwd["oracle"][tie] == 0).all()
    # what torch does off the safe points: NaN p and a draw of 0 give NaN; p == 0 infects, p == 1 does not
    p, o = fp["p"], fwd["oracle"]
    assert np.isnan(o[np.isnan(p)]).all() and np.isnan(o[kind_mask(fp, "draw0")]).all()
    edge = kind_mask(fp, "p_edge")
    assert (o[edge & (p == 0)] == 1).all() and (o[edge & (p == 1)] == 0).all()
    assert np.isfinite(o[kind_mask(fp, "draw_sub")]).all()


def test_state_update_restatement(fwd):
    """infect_unfused is oracle.infect_people bit for bit (NaN as a class).  With nu in {0, 1} - all a8 produces, NaN
    aside - a contracted t + nu * (now - t) gives the SAME bits (a product by 0 or 1 is exact), so the update cannot
    show a changed contraction flag; what the full mantissas pin is the sequence itself: t + (now - t) differs from
    `now` in the last bit on most agents, and a fused form would differ for any fractional nu."""
    fp = fwd["fp"]
    st = R.forward_state(fp["n"])
    nu = np.nan_to_num(fwd["oracle"], nan=1.0)
    nu[::11] = np.nan
    got = R.infect_unfused(st, nu)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    want = O.infect_people(t(st["susc"]), t(st["inf"]), t(st["time"]), t(nu), st["now"])
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.int32)[~np.isnan(g)], w.numpy().view(np.int32)[~np.isnan(g)])
        assert np.array_equal(np.isnan(g), np.isnan(w.numpy()))
    assert np.isnan(got[0][::11]).all()                    # torch.maximum(0, NaN) is NaN: a poisoned agent stays poisoned
    one = np.ones(fp["n"], dtype=np.float32)
    assert np.array_equal(R.infect_time_fused(st, one), R.infect_unfused(st, one)[2])
    moved = R.infect_unfused(st, one)[2] != np.float32(st["now"])
    assert moved.mean() > 0.25
    frac = np.full(fp["n"], 0.7, dtype=np.float32)
    assert (R.infect_time_fused(st, frac) != R.infect_unfused(st, frac)[2]).mean() > 0.1


# ---- the step's own a7 - a9 ------------------------------------------------------------------------------------------
ALL_STEP_DTS = R.STEP_DTS + R.EDGE_DTS[:1]


def prob_excess(ts, dt):
    p64, bound = R.prob_reference(ts, dt)
    p32 = R.prob_f32(ts, dt)
    q, ok = R.excess(p32, p64, bound)
    assert ok.all(), (dt, np.nonzero(~ok)[0].tolist())
    assert np.array_equal(np.isnan(p32), np.isnan(ts))
    v, i = R.worst(q)
    print(f"dt {dt:.4g}: {len(ts)} points, max err / bound = {v:.3f} at ts = {float(ts[i]):.6g} (p = {float(p64[i]):.9g})")
    return v


def test_prob_restatement_within_k_ref_of_its_bound():
    """not_infected_prob restated in fp32 stays within K_REF x the bound of prob_reference on every in-step point, at
    every dt of the in-step drive; NaN exactly where ts is NaN; the edges give the values they are named for.
    Measured: max err / bound 0.453 (ts = 100 at dt = 1: the subnormal p), 0.38 on the normal numbers.
    On the sampler grid's own ts (clamp edges, core, absolute) at its dts it is held to the bound itself, K: a correctly
    rounded evaluation errs by at most u p (x + r / 2), r = ulp(p) / (u p) in (1, 2], that is up to (x + 1) / (x + 3) of
    the bound - below 1 everywhere, but above K_REF from x = 2 on where the product rounds badly (the step points' targets
    at dt = 1 / 24, which is no dt of the in-step drive, reach 0.501 at ts * dt = 2.04).  Measured on the grid: 0.453."""
    top = (0.0, None)
    for dt in ALL_STEP_DTS:
        sp = R.step_points(dt)
        assert np.isnan(sp["ts"]).sum() == 3
        v = prob_excess(sp["ts"], dt)
        if v > top[0]:
            top = (v, dt)
        assert v <= R.K_REF, dt
    grid_top = 0.0
    for dt in R.DTS:
        grid = [R.F32(c / R.F32(dt)) for c in R.CORE] + R.clamp_edges() + [R.F32(t) for t in R.ABSOLUTE]
        grid_top = max(grid_top, prob_excess(np.array(grid, dtype=np.float32), dt))
    assert grid_top <= R.K
    print(f"sampler grid: max err / bound {grid_top:.3f}; asserted {R.K}")
    print(f"not_infected_prob, fp32 restatement: max err / bound {top[0]:.3f} at dt {top[1]:.4g}; asserted {R.K_REF}")
    # the in-step edges
    at = lambda dt, kind: R.prob_f32(R.step_points(dt)["ts"][kind_mask(R.step_points(dt), kind)], dt)
    assert (at(2.0, "ts_hi") == 0).all() and (at(0.01, "ts_lo") == 1).all()
    sub = at(1.0, "ts_hi")
    assert ((sub > 0) & (sub < R.FLT_MIN)).all()
    assert np.isnan(at(1.0, "ts_nan")).all()
    for dt in ALL_STEP_DTS:
        lo = R.prob_f32(np.array([R.TS_LO]), dt)[0]
        assert (at(dt, "ts_neg") == lo).all()                              # -0.0 and a negative ts clamp to 1e-6
        sat = at(dt, "ts_sat")                                             # +1e30 clamps to 100, -1e30 to 1e-6
        assert (sat[:3] == R.prob_f32(np.array([R.TS_HI]), dt)[0]).all() and (sat[3:] == lo).all()


def test_step_points_are_the_forward_points_as_target_ts():
    fp = R.forward_points()
    keep = np.array([k != "p_edge" for k in fp["kinds"]])
    for dt in R.STEP_DTS:
        sp = R.step_points(dt)
        n = int(keep.sum())
        assert sp["kinds"][:n] == [k for k in fp["kinds"] if k != "p_edge"]
        assert np.array_equal(sp["e0"][:n], fp["e0"][keep]) and np.array_equal(sp["e1"][:n], fp["e1"][keep])
        # the target gives the p back to a few ulp: |d ln p| = dt * ts * 2^-24 from the rounding of ts, and exp's own
        p = R.prob_f32(sp["ts"][:n], dt).astype(np.float64)
        want = fp["p"][keep].astype(np.float64)
        inside = (sp["ts"][:n] >= R.TS_LO) & (sp["ts"][:n] <= R.TS_HI)
        assert inside.mean() > 0.95
        assert (np.abs(p - want)[inside] <= 4 * R.U * want[inside] * (3.0 - np.log(want[inside]))).all()
        kinds = set(sp["kinds"])
        assert {"grid", "random", "tie", "draw0", "draw_sub", "ts_hi", "ts_lo", "ts_nan", "ts_sat", "ts_neg"} <= kinds
        d0 = kind_mask(sp, "draw0") | kind_mask(sp, "draw_sub")
        assert ((sp["e0"][d0] == 0) | (sp["e1"][d0] == 0)).sum() >= 6 and (sp["e0"][d0] == np.float32(1e-40)).any()
    assert R.step_points(0.01, False)["n"] < 60


def test_unsafe_share_of_the_step_points_is_a_condition_of_the_inputs():
    """MAX_UNSAFE_SHARE holds for the step points whatever the last bits of the device's p: with p rebuilt from the target
    ts through fp32 exp and moved by -2, 0 and +2 ulp the unsafe share stays under the cap at every dt of the in-step
    drive (the exact tie p == 0.5, e0 == e1 survives the detour through ts at dt = 1 only: elsewhere those rows are
    unsafe, and they are most of what is)."""
    for dt in R.STEP_DTS:
        sp = R.step_points(dt)
        p = R.prob_f32(sp["ts"], dt)
        shares = []
        for ulps in (-2, 0, 2):
            share, unsafe, safe, ruled, _ = R.unsafe_share(R.moved(p, ulps), sp["e0"], sp["e1"])
            shares.append(share)
            assert share <= R.MAX_UNSAFE_SHARE, (dt, ulps, share)
            assert ruled.sum() >= 15 and safe.mean() > 0.95
        print(f"dt {dt:.4g}: {sp['n']} points, unsafe share at -2 / 0 / +2 ulp: " + " / ".join(f"{s:.4%}" for s in shares))
