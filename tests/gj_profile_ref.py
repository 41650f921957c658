"""fp64 restatement of the transmission profile (reference grad_june/transmission.py:39-51) and of its six partials, the
error an fp32 evaluation of it must be allowed, and the points the profile's kernels are tested at.  Test infrastructure
only; torch on the CPU, no GPU import.

The operation, per agent:   t = now - infection_time,  d = t - shift,  u = d * rate,
    T = max_infectiousness * sign * exp(-lgamma(shape)) * pow(u, shape - 1) * exp(-u) * rate * is_infected,
    sign = (sgn(d + 1e-10) + 1) / 2.
t, d and d + 1e-10 are taken in fp32 - IEEE subtractions and one addition of the fp32 inputs, so the kernel, the fp32
oracle and this file hold the same bits (shift - t is exactly -d).  Everything after that is fp64 torch on those
values; the partials are fp64 autograd through the expression (d carries the gradient -1 to shift and infection_time).

What an fp32 evaluation is allowed, per agent (``B``):
    B = 2^-23 * (4 + |lgamma(shape)| + |(shape - 1) * log2(u)| + 1.4427 * |u|)
4: the roundings of the factors and of their products, and the 3.5e-7 of inv_gamma's polynomial; |lgamma|: exp(-lgamma)
amplifies the rounding of lgamma by |lgamma| (the libm branch outside (0.25, 16)); |(shape-1) log2 u|: the exponent of
pow = exp2(y log2 x), rounded to 2^-24 relative, is an absolute error of the exponent; 1.4427 |u|: the same for
exp(-u) = exp2(-u log2 e).  For u <= 0 or shape == 1 the pow is exact (0, 1, inf or an integer power of a negative
base by repeated rounding - the term is then that of |u|) and the log2 term is dropped.

A partial of the form T * (a - b) is allowed B * |T| * (|a| + |b|) (near a zero of a - b only absolute accuracy
survives):  shape: ln u - psi(shape);  rate: shape / rate - d;  shift, infection_time: rate - (shape - 1) / d.
max_infectiousness and is_infected: B * |partial|.  Where |T| * (|a| + |b|) is not finite or smaller (d == 0), B * |partial|.

A value is COMPARABLE - held to K * B relative - only where d > 0 and every fp32 factor is a normal number well inside
the range: 1/Gamma, pow, their product aux, exp(-u), aux2 = exp(-u) * rate, aux * aux2 and T, all with magnitude in
[1e-30, 1e30].  Elsewhere fp32 has lost its bits (exp(-100) is subnormal: 1.7 % off on the CPU, flushed to 0 by
v_exp_f32) or overflowed (pow(60, 27) = inf); there a value is held to the fp32 oracle's inf / NaN placement and, where
the oracle is finite, to K * B * |ref| + ``floor``:
    floor = 1e-30 + FLT_MIN * |max_inf * is_infected| * (|aux| + |aux2| + 1/Gamma * |aux2| + |aux| * rate)
- a factor that underflows is off by at most FLT_MIN = 2^-126 (flushed), which reaches T multiplied by the other factors.
A partial's floor is that of T times 1 + |a| + |b| (twice T's for max_infectiousness and is_infected, which divide T
by a value >= 0.5).  Partials are not compared where the fp32 forward itself is inf or NaN, nor at a non-integer shape
with d <= 0, where autograd's own 0 * inf decides (``partial_scope``).
"""
import math

import torch

FIELDS = ("max_infectiousness", "shape", "rate", "shift", "infection_time", "is_infected")
EPS = 2.0 ** -23
FLT_MIN = 2.0 ** -126
LO, HI = 1e-30, 1e30
NOW = 120.0


def _na(x, towards):
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(towards, dtype=torch.float32)))


SHAPES = (0.02, 0.1, 0.24, 0.25, _na(0.25, 1.0), 0.3, 0.5, _na(1.0, 0.0), 1.0, _na(1.0, 2.0), 1.56, _na(2.0, 1.0), 2.0,
          _na(2.0, 3.0), 3.0, 5.0, 7.5, 15.5, _na(16.0, 0.0), 16.0, 16.5, 28.0)
DS = (1e-6, 1e-3, 0.05, 0.4, 1.0, 2.5, 7.0, 14.0, 40.0, 100.0)
RATES = (0.1, 0.53, 1.0, 1.5)
# The fp32 oracle's measured maximum of err / (B * allowance) over the comparable grid points, forward and six partials,
# rounded up (tests/test_profile_ref.py measures and asserts it); the kernels are held to K = 2 * K_REF.
K_REF = 6
K = 2 * K_REF
DIGAMMA_SHAPES = (-0.5, -1.5, -2.25, -7.75, -1.0, -2.0, 0.0, -0.0, 1e-3, 5.999, 6.0, 6.001, 100.0)
MAX_EXCLUDED_SHARE = 0.20


def _f32(v):
    return torch.as_tensor(v, dtype=torch.float32).clone()


def _points(shape, d, rate, shift, mx, inf=1.0, exact_d=False):
    """Agents with t - shift == d up to fp32 rounding (infection_time = now - (d + shift) in fp32); ``exact_d``: shift
    and infection_time are chosen so that d is exact (shift = 2, small dyadic d)."""
    shape, d, rate = _f32(shape), _f32(d), _f32(rate)
    n = shape.numel()
    shift = _f32(shift).expand(n).clone()
    x = {"max_infectiousness": _f32(mx).expand(n).clone(), "shape": shape, "rate": rate.expand(n).clone(),
         "shift": shift, "infection_time": torch.tensor(NOW, dtype=torch.float32) - (d.expand(n) + shift),
         "is_infected": _f32(inf).expand(n).clone()}
    if exact_d:
        assert torch.equal(fp32_d(x, NOW), d.expand(n))
    return x


def fp32_d(x, now):
    return (torch.tensor(now, dtype=torch.float32) - x["infection_time"]) - x["shift"]


def grid_points():
    """SHAPES x DS x RATES at now = NOW, infected, shifts and max_infectiousness drawn once."""
    g = torch.Generator().manual_seed(20240607)
    s, d, r = torch.meshgrid(_f32(SHAPES), _f32(DS), _f32(RATES), indexing="ij")
    n = s.numel()
    shift = -3.0 + 6.0 * torch.rand(n, generator=g)
    mx = 0.5 + 1.5 * torch.rand(n, generator=g)
    return _points(s.reshape(-1), d.reshape(-1), r.reshape(-1), shift, mx)


def edge_points():
    """d <= 0, max_infectiousness 0 and is_infected 2 (rate 0.53, max_infectiousness 1.3, shift 2: d is exact).  Returns
    (agents, kinds): kinds[i] names what agent i is there for; ``forward_only`` kinds have partials that are inf or NaN
    by autograd's 0 * inf at a non-integer shape and are compared in the forward only."""
    rows = []   # (kind, shape, d, mx, inf)
    for s in (1.0, 2.0, 3.0, 4.0):
        rows.append(("d0_int", s, 0.0, 1.3, 1.0))
    for s in (0.5, 1.56):
        rows.append(("d0_frac", s, 0.0, 1.3, 1.0))
    for s in (1.0, 2.0, 3.0, 4.0):
        for d in (-0.5, -3.0):
            rows.append(("neg_int", s, d, 1.3, 1.0))
    for d in (-0.5, -3.0):
        rows.append(("neg_frac", 1.56, d, 1.3, 1.0))
    for s in (0.5, 1.0, 1.56, 3.0):
        rows.append(("mx0", s, 2.5, 0.0, 1.0))
        rows.append(("inf2", s, 2.5, 1.3, 2.0))
    kinds = [r[0] for r in rows]
    col = lambda i: [r[i] for r in rows]
    return _points(col(1), col(2), 0.53, 2.0, col(3), col(4), exact_d=True), kinds


FORWARD_ONLY_KINDS = ("d0_frac", "neg_frac")


def digamma_points():
    """DIGAMMA_SHAPES at d = 2.5, rate 0.53: what grad_shape's digamma sees (reflection, poles, +-0, the recurrence's end)."""
    n = len(DIGAMMA_SHAPES)
    return _points(DIGAMMA_SHAPES, [2.5] * n, 0.53, 2.0, 1.3, exact_d=True)


def all_points():
    """(agents, kinds): the grid, then the edge points, then the digamma points; kinds[i] is "grid", an edge kind or
    "digamma"."""
    g, (e, kinds), p = grid_points(), edge_points(), digamma_points()
    return concat(g, e, p), ["grid"] * g["shape"].numel() + kinds + ["digamma"] * p["shape"].numel()


def concat(*xs):
    return {k: torch.cat([x[k] for x in xs]) for k in FIELDS}


def _abs0(v):
    """|v| with NaN -> 0 (an allowance never grows from an undefined term) and inf kept"""
    return torch.nan_to_num(v.abs(), nan=0.0, posinf=math.inf)


def reference(x, now=NOW):
    """x: the six fp32 arrays.  Returns fp64 tensors: ``T``; ``partial[k]`` = dT/dk per agent; ``B``; ``comparable``;
    ``floor``; ``allow[k]``: the allowance of partial k per unit of B (multiply by K * B, and by |upstream|);
    ``allow_T`` likewise (= |T|)."""
    d32 = fp32_d(x, now)
    sign = ((torch.sign(d32 + torch.tensor(1e-10, dtype=torch.float32)) + 1) / 2).double()
    leaf = {k: x[k].double().requires_grad_() for k in FIELDS}
    mx, s, r, sh, ti, inf = (leaf[k] for k in FIELDS)
    moving = (now - ti) - sh
    d = d32.double() + (moving - moving.detach())        # the fp32 value, the gradient of (now - time) - shift
    u = d * r
    inv_gamma = torch.exp(-torch.lgamma(s))
    pw = torch.pow(u, s - 1.0)
    ex = torch.exp(-u)
    aux, aux2 = inv_gamma * pw, ex * r
    T = mx * sign * aux * aux2 * inf
    grads = torch.autograd.grad(T.sum(), [leaf[k] for k in FIELDS])
    partial = {k: g.detach() for k, g in zip(FIELDS, grads)}
    mx, s, r, inf, d, u, inv_gamma, pw, ex, aux, aux2, T = (
        v.detach() for v in (mx, s, r, inf, d, u, inv_gamma, pw, ex, aux, aux2, T))
    exact_pow = (u <= 0) | (s == 1.0)
    log_term = torch.where(exact_pow, torch.zeros_like(u), ((s - 1.0) * torch.log2(u.clamp_min(1e-300))).abs())
    B = EPS * (4.0 + torch.lgamma(s).abs() + log_term + 1.4427 * u.abs())
    comparable = d > 0
    for f in (inv_gamma, pw, aux, ex, aux2, aux * aux2, T):
        comparable &= (f.abs() >= LO) & (f.abs() <= HI)
    floor = LO + FLT_MIN * _abs0(mx * inf) * (_abs0(aux) + _abs0(aux2) * (1.0 + _abs0(inv_gamma)) + _abs0(aux) * r)
    ab = {"shape": _abs0(torch.log(u)) + _abs0(torch.digamma(s)), "rate": (s / r).abs() + d.abs(),
          "shift": r.abs() + _abs0((s - 1.0) / d)}
    ab["infection_time"] = ab["shift"]
    allow, floors = {}, {}
    for k in FIELDS:
        own = torch.nan_to_num(partial[k].abs(), nan=0.0, posinf=0.0)
        if k in ab:      # T * (a - b)
            allow[k] = torch.maximum(torch.nan_to_num(T.abs() * ab[k], nan=0.0, posinf=0.0), own)
            floors[k] = floor * (1.0 + torch.nan_to_num(ab[k], posinf=0.0))
        else:            # T / max_infectiousness, T / is_infected: both >= 0.5 on the points, or 0
            allow[k] = own
            floors[k] = 2.0 * floor
    return {"T": T, "partial": partial, "B": B, "comparable": comparable, "floor": floor, "floors": floors,
            "allow_T": T.abs(), "allow": allow, "d": d, "u": u}


def oracle32(x, now=NOW):
    """The fp32 oracle on the CPU: (T, {k: dT/dk}) by torch autograd through oracle.transmission_update."""
    import gj_oracle as O

    leaf = {k: x[k].clone().requires_grad_() for k in FIELDS}
    T = O.transmission_update(*[leaf[k] for k in FIELDS], now)
    grads = torch.autograd.grad(T.sum(), [leaf[k] for k in FIELDS])
    return T.detach(), {k: g.detach() for k, g in zip(FIELDS, grads)}


def placement(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    v = v.double()
    return torch.isposinf(v) * 1 + torch.isneginf(v) * 2 + torch.isnan(v) * 3


def excess(got, ref, B, allow, comparable, floor, extra=None):
    """The error in units of B * allow, per agent, where ``ref`` and ``got`` are finite; NaN elsewhere (placement is
    checked on its own).  Absolute allowances are taken off the error first: ``floor`` off the comparable points, and
    ``extra`` (the rounding of an accumulation) everywhere."""
    got, ref = got.double(), ref.double()
    den = B * allow
    err = (got - ref).abs()
    if extra is not None:                    # the part of the error the extra allowance explains is taken off first
        err = (err - extra).clamp_min(0.0)
    err = torch.where(comparable, err, (err - floor).clamp_min(0.0))
    q = torch.where(err == 0, torch.zeros_like(err), err / den)
    return torch.where(torch.isfinite(got) & torch.isfinite(ref), q, torch.full_like(q, math.nan))


def check_forward(got, ref, oracle_T):
    """(q, placed): q = the error of a forward in units of its allowance (NaN where it is not finite); placed = the
    inf / NaN placement is right - all finite on the comparable points, the fp32 oracle's elsewhere."""
    c = ref["comparable"]
    q = excess(got, ref["T"], ref["B"], ref["allow_T"], c, ref["floor"])
    want = torch.where(c, torch.zeros_like(placement(oracle_T)), placement(oracle_T))
    return q, placement(got) == want


def partial_scope(kinds, oracle_T):
    """The agents whose partials are compared: not the forward-only kinds, and not where the fp32 forward itself is
    inf or NaN (an fp32 overflow the fp64 reference does not have, or a non-integer power of a negative base)."""
    keep = torch.tensor([k not in FORWARD_ONLY_KINDS for k in kinds])
    return keep & torch.isfinite(oracle_T)


def check_partial(k, got, ref, scope, upstream=None, incoming=None):
    """(q, placed) for ``got`` = [incoming +] upstream * dT/dk: as check_forward, with the allowance scaled by
    |upstream| and, for an accumulation, the fp32 rounding of the sum (2^-23 of both terms) on top; NaN and inf exactly
    where the fp64 value has them.  Agents outside ``scope``: q NaN, placed True."""
    p = ref["partial"][k]
    up = torch.ones_like(p) if upstream is None else upstream.double()
    want = up * p
    extra = None
    if incoming is not None:
        extra = EPS * (incoming.double().abs() + torch.nan_to_num(want.abs(), nan=0.0, posinf=0.0))
        want = incoming.double() + want
    q = excess(got, want, ref["B"], ref["allow"][k] * up.abs(), ref["comparable"], ref["floors"][k] * up.abs(), extra)
    q = torch.where(scope, q, torch.full_like(q, math.nan))
    return q, (placement(got) == placement(want)) | ~scope


def worst(q):
    """the largest finite entry of q (0 if there is none) and its index"""
    z = torch.nan_to_num(q, nan=0.0)
    i = int(z.argmax())
    return float(z[i]), i
