"""fp64 restatement, per agent, of the infection sampler (a8 + a9: gj_sample_infect) and of its adjoint through the
epilogue a7 (gj_adjoint_sample), the error an fp32 evaluation of the adjoint must be allowed, and the points the two
kernels are tested at.  Test infrastructure only; numpy on the CPU.  The softmax terms and the adjoint's h, nu_bar and
d nu / d p are those of tests/gj_seed_ref.py (one ``dtype``-parametrised definition for the seed and the sampler).

The operation, from the fp32 inputs susc0, acc, time0, (e0, e1), the cotangents g_susc, g_inf, g_time, g_new, and the
scalars now, dt:
    ts = susc0 * acc                      taken as the fp32 product: what the kernel clamps is a decision of its arithmetic
    inside = 1e-6f <= ts <= 100f          against the fp32 constants (1e-6f < 1e-6: a double constant puts ts == 1e-6f outside)
    p = clamp(exp(-clamp(ts, 1e-6f, 100f) * dt), 0, 1)           (NaN passes through both clamps)
    y0, y1 = softmax(((ln p - ln e0) / 0.1, (ln(1 - p) - ln e1) / 0.1));   nu = [y1 > y0]   (a tie: not infected)
    h = 1, 0.5, 0 for susc0 - nu >, ==, < 0;   nu_bar = g_inf + g_time * (now - time0) - g_susc * h + g_new
    d nu / d p = -(y0 * y1 / 0.1) * (1 / p + 1 / (1 - p)), 0 where that is not finite
    ts_bar = inside ? nu_bar * d nu / d p * (-dt * p) : 0
    x_out = susc0 * ts_bar,  grad_susc_out = g_susc * h + ts_bar * acc,  grad_time_out = g_time * (1 - nu)
Everything after ``ts`` and ``inside`` is fp64 on the fp32 values.

What an fp32 evaluation of ts_bar is allowed, per agent (``B``), with u = 2^-24 the unit roundoff, L = |ln p| + |ln(1-p)|
+ |ln e0| + |ln e1|, q = p / (1 - p) and rp = |ln p| + 2 + 2^-149 / (p u) the relative error of p in units of u (the
product ts * dt rounds: an absolute error |ln p| u of the exponent; exp itself is given one ulp = 2 u; below 2^-126 p
is a subnormal number with a quantum of 2^-149):
  1. through D = z0 - z1, which y0 * y1 = s(D) s(-D) sees with |d ln(y0 y1) / d D| = |y1 - y0| <= 1.  Everything inside
     the division by tau is multiplied by 1 / tau = 10:  each of the four logarithms is one ulp = 2 u of itself off and
     each sum ln + (-ln e) rounds once (3 L);  the division by 0.1f rounds, 0.1f is 0.25 u away from 0.1, and z0 - z1
     rounds, each relative to |z0| + |z1| <= 10 L (2.25 L);  p's own error reaches ln p as rp and ln(1 - p) as
     1 + rp q - the cancellation in 1 - p, u p / (1 - p) per u of p, plus the rounding of the difference.
         10 * (5.25 L + rp (1 + q) + 1)
  2. directly:  exp (one of the two is exp(0) = 1), x0 + x1, the two quotients, y0 * y1 and the division by 0.1f: 7.25;
     1/p + 1/(1-p): rp max(1, q) + 3;  -dt * p: rp + 1;  the two remaining products: 2.
         rp (2 + q) + 14
  3. nu_bar is a sum of four terms that may cancel: its three additions, the product and now - time0 round relative to
     S = |g_inf| + |g_time (now - time0)| + |g_susc h| + |g_new|, at most 5 u S, an ABSOLUTE error 5 u S |d nu / d p| dt p.
  4. where y0 * y1 (or the smaller of x0, x1) falls below fp32's normal range it is a subnormal number or flushed to 0:
     off by at most 2^-126, which reaches ts_bar as 2^-126 * S * (1/p + 1/(1-p)) * dt * p / 0.1.
    cond = 10 * (5.25 L + rp (1 + q) + 1) + rp (2 + q) + 14
    B    = u * (|ts_bar| * cond + 5 S |d nu / d p| dt p) + 2^-126 * S * (1/p + 1/(1-p)) * dt * p / 0.1
x_out and grad_susc_out carry it through one product, and their own roundings:
    B_x = |susc0| B + u |x_out|,     B_g = |acc| B + 2 u (|g_susc h| + |ts_bar acc|)
Outside the clamp, for a NaN ts, and where d nu / d p is not finite ts_bar is exactly 0 (no allowance), and
grad_time_out has none anywhere: g_time * (1 - nu) is one exact difference and one product of the fp32 inputs.

The decision nu is a comparison of two roundings.  It is SAFE - the same in every precision - where |D| exceeds the
error of the fp32 D bounded in (1), 10 u (5.25 L + rp (1 + q) + 1), or at the exact tie p == 0.5 with e0 == e1 (the two
rows go through the same operations: not infected).  On the other points the reference takes the decision it is given.
A point is LOOSE where B exceeds 1 % of |ts_bar|: still held to K * B, to the sign and to the NaN and zero rules, but it
says little about the kernel.

The step's own a7 - a9 (tests/test_gpu_epilogue_kernels.py) take from here: ``prob_reference`` (p in fp64 and the bound
an fp32 evaluation is allowed), ``step_points`` (the forward points as the ts an agent of the step must be given, and the
in-step edges), ``forward_decision`` on the p the device wrote, and ``infect_unfused``.
"""
import functools

import numpy as np

import gj_seed_ref as S

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
F32 = np.float32
TS_LO, TS_HI = F32(1e-6), F32(100.0)
NOW = 12.25
DTS = (1.0 / 24.0, 0.25, 0.5, 1.0)      # the grid's steps
EDGE_DTS = (0.01, 2.0)                  # p == 1 after rounding at ts = 1e-6; p underflows to 0 at ts = 100
SUSC = (0.0, 0.3, 1.0)
DRAWS = ((0.01, 5.0), (5.0, 0.01), (1.0, 1.0), (0.5, 2.0), (2.0, 0.5), (0.05, 0.05), (0.3, 0.31), (3.0, 0.1), (0.1, 3.0))
CORE = (0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.3, 0.5, float(np.log(2.0)), 1.0, 1.5, 2.0, 2.5, 3.5, 4.0, 5.0)   # ts * dt
ABSOLUTE = (1e-3,)                     # ts whatever dt: between the lower bound and the core
MAX_LOOSE_SHARE = 0.35
MAX_UNSAFE_SHARE = 0.01
# The fp32 numpy restatement's measured maximum of err / B over every point and the three outputs, rounded up to the next
# tenth (tests/test_sampler_ref.py measures and asserts it); the kernels are held to K = 2 * K_REF.
K_REF = 0.5
K = 2 * K_REF
COTANGENTS = ("g_susc", "g_inf", "g_time", "g_new")
OUTPUTS = ("x_out", "grad_susc", "grad_time")


def _na(x, up, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf if up else -np.inf), dtype=F32)
    return x


def clamp_edges():
    """ts below, at and just above both clamp bounds, and beyond: negative, 0, the tiled sums' saturation value"""
    return [F32(-1.0), F32(0.0), F32(5e-7), _na(TS_LO, False), TS_LO, _na(TS_LO, True), F32(2e-6),
            _na(TS_HI, False), TS_HI, _na(TS_HI, True), F32(150.0), F32(1e30)]


def acc_for(ts, susc):
    """an fp32 acc whose fp32 product with ``susc`` is ``ts`` where one exists within four ulp of ts / susc (else the
    nearest product; the reference takes whatever the product is)"""
    ts, susc = F32(ts), F32(susc)
    if susc == 0:
        return ts
    with np.errstate(over="ignore"):
        a0 = F32(ts / susc)
    if not np.isfinite(a0) or a0 == 0:
        return a0
    cands = [_na(a0, False, k) for k in range(4, 0, -1)] + [a0] + [_na(a0, True, k) for k in range(1, 5)]
    return min(cands, key=lambda a: abs(float(F32(susc * a)) - float(ts)))


def _finish(rows, dt, seed):
    """rows of (kind, susc0, acc, e0, e1) -> the point set of one launch: fp32 arrays, random time0 and cotangents"""
    g = np.random.default_rng(seed)
    n = len(rows)
    col = lambda i: np.array([r[i] for r in rows], dtype=F32)
    pts = {"kinds": [r[0] for r in rows], "n": n, "dt": float(F32(dt)), "now": NOW, "susc0": col(1), "acc": col(2),
           "e0": col(3), "e1": col(4), "time0": (NOW * g.random(n)).astype(F32)}
    for k in COTANGENTS:                   # away from 0, so that no term of nu_bar vanishes by chance
        v = g.uniform(0.1, 1.0, n) * g.choice([-1.0, 1.0], n)
        pts[k] = v.astype(F32)
    return pts


def _edge_rows(dt):
    ln2 = F32(np.log(2.0))
    rows = []
    for s in (0.3, 1.0):
        rows.append(("tie", s, acc_for(F32(ln2 / F32(dt)), s), 0.7, 0.7))      # p == 0.5 at dt = 1
        rows.append(("p_one", s, acc_for(TS_LO, s), 0.5, 2.0))                # p == 1 at dt = 0.01
        rows.append(("p_zero", s, acc_for(TS_HI, s), 0.5, 2.0))               # p == 0 at dt = 2
    for s in SUSC:
        rows.append(("nan_acc", s, np.nan, 1.0, 1.0))
        rows.append(("inf_acc", s, np.inf, 1.0, 1.0))                         # (0 * inf: a NaN ts)
        rows.append(("inf_acc", s, -np.inf, 1.0, 1.0))
    mid = F32(1.0 / F32(dt))                                                  # ts * dt = 1
    for s in (0.3, 1.0):
        a = acc_for(mid, s)
        rows += [("draw0", s, a, 0.0, 1.0), ("draw0", s, a, 1.0, 0.0), ("draw0", s, a, 0.0, 0.0),
                 ("draw_sub", s, a, 1e-40, 1.0), ("draw_sub", s, a, 1.0, 1e-40), ("draw_sub", s, a, 1e-40, 2e-40)]
    return rows


@functools.lru_cache(maxsize=None)
def points(dt, grid=True):
    """The agents of one launch (dt is a launch scalar): the grid - (clamp edges + core + absolute ts) x DRAWS x SUSC -
    when ``grid``, then the named edge points.  Cached: callers leave the arrays unchanged."""
    rows = []
    if grid:
        ts_list = clamp_edges() + [F32(c / F32(dt)) for c in CORE] + [F32(t) for t in ABSOLUTE]
        for ts in ts_list:
            for e0, e1 in DRAWS:
                for s in SUSC:
                    rows.append(("grid", s, acc_for(ts, s), e0, e1))
    rows += _edge_rows(dt)
    return _finish(rows, dt, 1000 + int(round(1000 * dt)))


def all_point_sets():
    return [points(dt) for dt in DTS] + [points(dt, False) for dt in EDGE_DTS]


def epilogue(pts, dtype=np.float64):
    """(ts, inside, p): ts the fp32 product, inside against the fp32 constants, p in ``dtype``"""
    with np.errstate(invalid="ignore", over="ignore"):
        ts = (pts["susc0"] * pts["acc"]).astype(F32)
        inside = (ts >= TS_LO) & (ts <= TS_HI)
        tsc = np.where(np.isnan(ts), ts, np.minimum(np.maximum(ts, TS_LO), TS_HI)).astype(dtype)
        p = np.exp(-tsc * dtype(pts["dt"]))
        p = np.where(np.isnan(p), p, np.minimum(np.maximum(p, dtype(0.0)), dtype(1.0)))
    return ts, inside, p.astype(dtype)


def _abs0(v):
    """|v| with NaN and inf -> 0: an allowance never grows from an undefined term"""
    return np.nan_to_num(np.abs(v), nan=0.0, posinf=0.0, neginf=0.0)


def adjoint(pts, dtype=np.float64, nu=None, drop=()):
    """The adjoint's outputs in ``dtype`` (float64: the reference; float32: the kernel's arithmetic, op for op).
    ``nu``: the decisions to take (default: the fp32 forward's rule, gj_seed_ref.decisions).  ``drop``: cotangents
    that are NULL.  Returns a dict with the three outputs and ts_bar, nu, h, nu_bar, dnu_dp, p, y0, y1, inside."""
    ts, inside, p = epilogue(pts, dtype)
    e0, e1 = pts["e0"].astype(dtype), pts["e1"].astype(dtype)
    y0, y1 = S.softmax_terms(p, e0, e1, dtype)
    if nu is None:
        _, _, p32 = epilogue(pts, F32)
        nu = S.decisions(p32, pts["e0"], pts["e1"])
    nu = np.asarray(nu, dtype=dtype)
    zeros = np.zeros(pts["n"], dtype=dtype)
    gs, gi, gt, gn = (zeros if k in drop else pts[k].astype(dtype) for k in COTANGENTS)
    s0, t0, ac = pts["susc0"].astype(dtype), pts["time0"].astype(dtype), pts["acc"].astype(dtype)
    h, nu_bar, dnu_dp = S.sampler_adjoint_terms(p, s0, t0, y0, y1, nu, pts["now"], gs, gi, gt, gn, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        ts_bar = np.where(inside, nu_bar * dnu_dp * (-dtype(pts["dt"]) * p), dtype(0.0))
        out = {"x_out": s0 * ts_bar, "grad_susc": gs * h + ts_bar * ac, "grad_time": gt * (dtype(1.0) - nu)}
    out.update(ts_bar=ts_bar, nu=nu, h=h, nu_bar=nu_bar, dnu_dp=dnu_dp, p=p, y0=y0, y1=y1, inside=inside, ts=ts,
               S=np.abs(gi) + np.abs(gt * (dtype(pts["now"]) - t0)) + np.abs(gs * h) + np.abs(gn))
    return out


def reference(pts, nu=None):
    """The fp64 outputs with their bounds: ``B`` (of ts_bar), ``bound[k]`` per output, ``safe`` (the decision cannot
    flip under rounding), ``nu64`` (the fp64 decision), ``loose``.  ``nu``: decisions to take on the points that are not
    safe (on the safe ones the fp64 decision is taken whatever is given)."""
    f64 = adjoint(pts, np.float64, nu=np.zeros(pts["n"]))
    p, e0, e1 = f64["p"], pts["e0"].astype(np.float64), pts["e1"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        L = _abs0(np.log(p)) + _abs0(np.log1p(-p)) + _abs0(np.log(e0)) + _abs0(np.log(e1))
        q = _abs0(p / (1.0 - p))
        rp = _abs0(np.log(p)) + 2.0 + _abs0(2.0 ** -149 / (p * U))
        d_err = 10.0 * U * (5.25 * L + rp * (1.0 + q) + 1.0)
        D = (np.log(p) - np.log(e0)) / S.TAU - (np.log1p(-p) - np.log(e1)) / S.TAU
        _, _, p32 = epilogue(pts, F32)
        tie = (p32 == F32(0.5)) & (pts["e0"] == pts["e1"]) & (pts["e0"] > 0)
    # a NaN softmax (a NaN p, a draw of 0: inf - inf) compares false whatever the arithmetic: not infected
    ruled = np.isnan(f64["y0"]) | np.isnan(f64["y1"])
    nu64 = np.where(tie | ruled, 0.0, (f64["y1"] > f64["y0"]).astype(np.float64))
    safe = tie | ruled | (np.abs(D) > d_err)                        # (the comparison is false for a NaN D)
    taken = nu64 if nu is None else np.where(safe, nu64, np.asarray(nu, dtype=np.float64))
    ref = adjoint(pts, np.float64, nu=taken)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cond = 10.0 * (5.25 * L + rp * (1.0 + q) + 1.0) + rp * (2.0 + q) + 14.0
        dt = pts["dt"]
        B = (U * (_abs0(ref["ts_bar"]) * cond + 5.0 * ref["S"] * _abs0(ref["dnu_dp"]) * dt * p)
             + FLT_MIN * ref["S"] * _abs0(1.0 / p + 1.0 / (1.0 - p)) * dt * p / S.TAU)
        B = np.where(ref["inside"], np.nan_to_num(B, nan=0.0, posinf=0.0), 0.0)
        s0, ac = np.abs(pts["susc0"].astype(np.float64)), np.abs(pts["acc"].astype(np.float64))
        gsh = np.abs(pts["g_susc"].astype(np.float64) * ref["h"])
        bound = {"x_out": s0 * B + U * _abs0(ref["x_out"]),
                 "grad_susc": np.nan_to_num(ac * B, nan=0.0, posinf=0.0) + 2.0 * U * (gsh + _abs0(ref["ts_bar"] * ac)),
                 "grad_time": np.zeros(pts["n"])}
    ref.update(B=B, bound=bound, safe=safe, nu64=nu64, tie=tie, D=D,
               loose=(ref["ts_bar"] != 0) & (B > 0.01 * np.abs(ref["ts_bar"])))
    return ref


def excess(got, want, bound):
    """(q, ok): q = |got - want| / bound per agent (0 where both agree exactly, inf where they differ with no
    allowance, NaN where the reference is NaN); ok = the NaN rule (NaN exactly where the reference has one) and the
    sign rule (no non-zero value with the sign opposite to a non-zero reference's beyond the bound)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - want)
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(nan, np.nan, q)
    ok = np.isnan(got) == nan
    wrong_sign = (got * want < 0) & (err > bound)
    return q, ok & ~wrong_sign


def worst(q):
    z = np.nan_to_num(q, nan=0.0, posinf=np.inf)
    i = int(z.argmax())
    return float(z[i]), i


# ---- the forward: a8 + a9 ---------------------------------------------------------------------------------------------
def forward_points(n_random=1500, seed=5):
    """p and draw pairs for gj_sample_infect with injected draws: the grid's fp32 p's x DRAWS, random (p, e0, e1), and
    the named points - the exact tie, p in {0, 1, NaN}, a draw of 0, a subnormal draw."""
    ps = []
    for dt in DTS:
        _, _, p32 = epilogue(points(dt), F32)
        ps.append(p32[np.isfinite(p32)])
    ps = np.unique(np.concatenate(ps))
    rows = [("grid", p, e0, e1) for p in ps for e0, e1 in DRAWS]
    g = np.random.default_rng(seed)
    for p, e0, e1 in zip(g.random(n_random), g.exponential(size=n_random), g.exponential(size=n_random)):
        rows.append(("random", p, e0, e1))
    for e in (0.01, 0.7, 5.0):
        rows.append(("tie", 0.5, e, e))
    for p in (0.0, 1.0, np.nan):
        for e0, e1 in ((1.0, 1.0), (0.5, 2.0), (2.0, 0.5)):
            rows.append(("p_edge", p, e0, e1))
    for p in (0.2, 0.5, 0.9):
        rows += [("draw0", p, 0.0, 1.0), ("draw0", p, 1.0, 0.0), ("draw0", p, 0.0, 0.0),
                 ("draw_sub", p, 1e-40, 1.0), ("draw_sub", p, 1.0, 1e-40)]
    col = lambda i: np.array([r[i] for r in rows], dtype=F32)
    return {"kinds": [r[0] for r in rows], "n": len(rows), "p": col(1), "e0": col(2), "e1": col(3)}


def forward_decision(fp):
    """(nu64, safe, ruled) of the forward points.  nu64: the fp64 decision from the fp32 p and draws.  safe: it cannot
    flip under the rounding of the fp32 z0 - z1 (p is an input here: rp = 0, and 1 - p rounds once, which is one u in
    ln(1 - p)); the exact tie is safe.  ruled: p in {0, 1, NaN} or a draw of 0 - no rounding question, the value is what
    torch gives (oracle.sample_infected), NaN included."""
    p, e0, e1 = (fp[k].astype(np.float64) for k in ("p", "e0", "e1"))
    y0, y1 = S.softmax_terms(p, e0, e1, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = _abs0(np.log(p)) + _abs0(np.log1p(-p)) + _abs0(np.log(e0)) + _abs0(np.log(e1))
        D = (np.log(p) - np.log(e0)) / S.TAU - (np.log1p(-p) - np.log(e1)) / S.TAU
    ruled = ~np.isfinite(D)
    tie = (fp["p"] == F32(0.5)) & (fp["e0"] == fp["e1"]) & (fp["e0"] > 0)
    nu = np.where(tie, 0.0, (y1 > y0).astype(np.float64))
    safe = (tie | (np.abs(D) > 10.0 * U * (5.25 * L + 1.0))) & ~ruled
    return nu, safe, ruled


UPDATE_NOW = float(F32(12.3456789))      # a full mantissa, like the infection times below


def forward_state(n, seed=9):
    """Pre-states for a9 on n agents: susceptibility 0, fractional, one ulp below 1, 1, above 1; is_infected 0, 1, 0.5;
    infection times with full mantissas on both sides of ``UPDATE_NOW``, up to 30 times its size (t + (now - t) is then
    not `now`: the difference rounds at t's ulp)."""
    g = np.random.default_rng(seed)
    susc = np.array([0.0, 0.3, 1.0, float(_na(1.0, False)), 2.5], dtype=F32)[np.arange(n) % 5]
    inf = np.array([0.0, 1.0, 0.5], dtype=F32)[(np.arange(n) // 5) % 3]
    return {"susc": susc, "inf": inf, "time": (400.0 * g.random(n)).astype(F32), "now": UPDATE_NOW}


def infect_unfused(st, nu):
    """a9 as the unfused fp32 op sequence: max(0, s - nu) (torch.maximum: a NaN stays), i + nu, t + nu * (now - t), each
    operation rounded on its own."""
    nu = np.asarray(nu, dtype=F32)
    with np.errstate(invalid="ignore"):
        d = (F32(st["now"]) - st["time"]).astype(F32)
        prod = (nu * d).astype(F32)
        return (np.maximum(F32(0.0), (st["susc"] - nu).astype(F32)), (st["inf"] + nu).astype(F32),
                (st["time"] + prod).astype(F32))


def infect_time_fused(st, nu):
    """t + nu * (now - t) with the product and the sum contracted into one fused multiply-add: the product of two fp32
    values is exact in fp64, and the fp64 sum is rounded to fp32 once."""
    d = (F32(st["now"]) - st["time"]).astype(F32)
    return (st["time"].astype(np.float64) + np.asarray(nu, dtype=np.float64) * d.astype(np.float64)).astype(F32)


# ---- the step's own a7 - a9: not_infected_prob, and the points of the in-step drive -----------------------------------------
STEP_DTS = (0.25, 1.0, 2.0)              # the in-step drive's full point sets; EDGE_DTS[0] = 0.01 takes the edges only
EXPF_ULP = 1.0                           # expf's maximum error in ulp, as the HIP math API documentation states it
SUBNORMAL = 2.0 ** -149


def prob_reference(ts, dt):
    """(p64, bound) of a7 per agent.  p64 = clip(exp(-clip(ts, 1e-6f, 100f) * dt), 0, 1) in fp64 from the fp32 ``ts`` and
    the fp32 ``dt`` (a NaN stays NaN, as clamp_keep_nan keeps it; the clamp of ts is exact in every precision).  What an
    fp32 evaluation is allowed, from the number formats, with x = clip(ts) * dt:
      the product x rounds once: an absolute error u x of the exponent, which moves exp(-x) by x u relative;
      expf is EXPF_ULP ulp off, an ulp being at most 2 u of the value;  one final rounding, u (the clamp to [0, 1] is exact);
      below 2^-126 the result is a subnormal number with a quantum of 2^-149.
        bound = u p64 (x + 2 EXPF_ULP + 1) + 2^-149
    (rp of the adjoint's bound above is the same count without the final rounding: there p is an intermediate.)"""
    ts = np.asarray(ts, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(np.isnan(ts), ts, np.minimum(np.maximum(ts, TS_LO), TS_HI)).astype(np.float64)
        x = c * float(F32(dt))
        p = np.exp(-x)
        p = np.where(np.isnan(p), p, np.minimum(np.maximum(p, 0.0), 1.0))
        bound = U * p * (x + 2.0 * EXPF_ULP + 1.0) + SUBNORMAL
    return p, np.nan_to_num(bound, nan=0.0)


def prob_f32(ts, dt):
    """a7 op for op in fp32: not_infected_prob of csrc/gj_device.h, with expf the correctly rounded one - the fp64
    exponential of the fp32 product, rounded once.  (numpy's own float32 exp is measured up to 2.1 ulp off on [0.01, 5]:
    more than the one ulp the bound grants the device's expf, so it cannot stand in for it.)"""
    ts = np.asarray(ts, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        c = np.where(np.isnan(ts), ts, np.minimum(np.maximum(ts, TS_LO), TS_HI)).astype(F32)
        p = np.exp(-(c * F32(dt)).astype(F32).astype(np.float64)).astype(F32)
        return np.where(np.isnan(p), p, np.minimum(np.maximum(p, F32(0.0)), F32(1.0))).astype(F32)


def step_edges():
    """The in-step edges as (kind, ts, e0, e1): ts at and beyond both clamp bounds (p == 0 at dt = 2, a subnormal p at
    dt = 1, p == 1 at dt = 0.01), a NaN ts, the tiled sums' saturation value with both signs, -0.0 and a negative ts
    (both clamp to 1e-6); draws of 0 and a subnormal draw on a ts in the core (placed by step_points: ts * dt = 1)."""
    rows = []
    for kind, values in (("ts_hi", (TS_HI, _na(TS_HI, True), F32(150.0))), ("ts_lo", (TS_LO, _na(TS_LO, False), F32(5e-7))),
                         ("ts_nan", (F32(np.nan),)), ("ts_sat", (F32(1e30), F32(-1e30))),
                         ("ts_neg", (F32(-0.0), F32(-1.0)))):
        for ts in values:
            for e0, e1 in ((1.0, 1.0), (0.5, 2.0), (2.0, 0.5)):
                rows.append((kind, ts, e0, e1))
    return rows


@functools.lru_cache(maxsize=None)
def step_points(dt, grid=True, n_random=1500, seed=5):
    """The points of forward_points - the grid's p's x DRAWS, the random rows, the ties and the named draws - as the
    TARGET ts = -ln(p) / dt an agent of the step must be given at this ``dt`` (fp32; p == 0 asks for +inf, which the
    clamp takes as 100), when ``grid``; then the in-step edges.  Cached: callers leave the arrays unchanged."""
    rows = []
    dt32 = float(F32(dt))
    if grid:
        fp = forward_points(n_random, seed)
        with np.errstate(divide="ignore"):
            ts = (-np.log(fp["p"].astype(np.float64)) / dt32).astype(F32)
        for k, t, e0, e1 in zip(fp["kinds"], ts, fp["e0"], fp["e1"]):
            if k != "p_edge":                       # p in {0, 1, NaN} as an input: the in-step edges below take their place
                rows.append((k, t, e0, e1))
    rows += step_edges()
    mid = F32(1.0 / dt32)
    rows += [("draw0", mid, 0.0, 1.0), ("draw0", mid, 1.0, 0.0), ("draw0", mid, 0.0, 0.0),
             ("draw_sub", mid, 1e-40, 1.0), ("draw_sub", mid, 1.0, 1e-40), ("draw_sub", mid, 1e-40, 2e-40)]
    col = lambda i: np.array([r[i] for r in rows], dtype=F32)
    return {"kinds": [r[0] for r in rows], "n": len(rows), "dt": dt32, "ts": col(1), "e0": col(2), "e1": col(3)}


def moved(p, ulps):
    """p moved by ``ulps`` units in the last place, inside [0, 1]; a NaN stays"""
    p = np.asarray(p, dtype=F32).copy()
    for _ in range(abs(ulps)):
        p = np.nextafter(p, F32(np.inf if ulps > 0 else -np.inf), dtype=F32)
    return np.where(np.isnan(p), p, np.minimum(np.maximum(p, F32(0.0)), F32(1.0))).astype(F32)


def unsafe_share(p, e0, e1):
    """(share, unsafe, safe, ruled, nu64) of forward_decision on the probabilities ``p``"""
    nu64, safe, ruled = forward_decision({"p": np.asarray(p, dtype=F32), "e0": e0, "e1": e1})
    unsafe = ~safe & ~ruled
    return float(unsafe.mean()), unsafe, safe, ruled, nu64
