"""Pass 1 of the tiled step per venue - k_tile_scatter, phase B of k_tile_venues, k_tile_presum and k_presum_reduce of
csrc/gj_tiled.h - restated in numpy float32 / int64 from the EDGE LISTS, bit for bit.

The library is built with -ffp-contract=off, so every float32 product below is one rounding, as on the device.  Nothing
here reads a tile table, a slot, a descriptor or an ELL row: the inputs are the COO lists of a set (halo agents' edges
included), the plan's float32 p_contact and which of the two rules for values that cannot be summed the set's form
follows.  Per network k of the set (column k of cum: the rank among the set's ACTIVE networks):

    x_src  = transmission                    for a MASK_RAW network (household)
           = fp32(q * transmission)          otherwise, q in {0, 1} = stage < q_threshold under quarantine (exact)
    w      = 1                               for a plain set
           = table_k[day_type, sex, age]     for a leisure network; transposed: times (age > 75) for the care-visit kind
    term   = fp32(w * x_src[agent])          ONE float32 product; for a plain set the value itself
    limit  = the bit pattern of 2^14, halved for every doubling of the set's largest venue above 4 096 edges
    in     = (bits(term) & 0x7FFFFFFF) <= limit
    fx     = rint(float64(term) * 2^36)      round half to even, as int64
    sum    = exact integer sum over the venue's edges that are `in`
    s      = fp32(float64(sum) * 2^-36)      TWO roundings: int64 -> float64, then -> float32
    default rule:  a term not `in` raises POS unless term < 0, and NEG unless term > 0;
                   s = +1e30 (POS), -1e30 (NEG), NaN (both)
    presum rule:   a term not `in` makes s NaN (one flag per sum, k_tile_presum)
    cum    = fp32(fp32(beta_k * p_contact[v]) * s)

``variant`` names deliberate MISSTATEMENTS of one rule each; tests/test_pass1_ref.py uses them to show that the inputs
of tests/test_gpu_pass1_kernels.py tell a wrong kernel from a right one."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

F32 = np.float32
FX_BITS = 36
FX_SCALE = 2.0 ** FX_BITS
SATURATED = np.float32(1.0e30)
WINDOW_EDGES = 4096                 # edges of a set's largest venue up to which the window is 2^14
VARIANTS = ("single_rounding", "floor", "window_not_shrunk", "strict_window", "mask_forward")


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def f32_of(b) -> np.ndarray:
    return np.ascontiguousarray(b).view(np.float32)


def term_limit_bits(max_venue_edges: int) -> int:
    """The set's window: 2^14 while its largest venue has at most 4 096 edges, else the power of two
    that keeps edges x window below 2^26."""
    e, p2 = 14, WINDOW_EDGES
    while p2 < max_venue_edges and e > -20:
        p2, e = 2 * p2, e - 1
    return int(np.float32(2.0 ** e).view(np.uint32))


def in_window(term: np.ndarray, limit: int, strict: bool = False) -> np.ndarray:
    a = bits(term) & np.uint32(0x7FFFFFFF)
    return (a < np.uint32(limit)) if strict else (a <= np.uint32(limit))


def to_fx(term: np.ndarray, floor: bool = False) -> np.ndarray:
    """rint(term * 2^36) as int64 (round half to even); term float32 inside the window (the product is exact)."""
    d = np.asarray(term, dtype=np.float32).astype(np.float64) * FX_SCALE
    return (np.floor(d) if floor else np.rint(d)).astype(np.int64)


def from_fx(sums: np.ndarray) -> np.ndarray:
    """fp32(float64(sum) * 2^-36): the int64 is rounded to float64 first, the scaled value to float32 second."""
    return (np.asarray(sums, dtype=np.int64).astype(np.float64) * (1.0 / FX_SCALE)).astype(np.float32)


def from_fx_once(sums: np.ndarray) -> np.ndarray:
    """The exact sum rounded to float32 ONCE (not what the device does: the ``single_rounding`` misstatement)."""
    out = np.empty(len(sums), dtype=np.float32)
    for i, s in enumerate(np.asarray(sums, dtype=np.int64).tolist()):
        neg, m = s < 0, abs(s)
        n = m.bit_length()
        if n > 24:                                   # round half to even at 24 bits, on the integer
            sh = n - 24
            q, r = m >> sh, m & ((1 << sh) - 1)
            half = 1 << (sh - 1)
            q += int(r > half or (r == half and (q & 1)))
            m = q << sh
        v = math.ldexp(float(m), -FX_BITS)           # (m has at most 24 significant bits: exact)
        out[i] = -v if neg else v
    return out


def source(x, stage, q_thr: float, has_quarantine: bool, raw: bool) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    if raw or not has_quarantine:
        return x
    q = (np.asarray(stage, dtype=np.float32) < F32(q_thr)).astype(np.float32)
    with np.errstate(all="ignore"):
        return (q * x).astype(np.float32)


def restate_set(agent, venue, p_contact, nets: Sequence[tuple], x, *, age=None, sex=None, stage=None,
                q_thr: float = math.inf, has_quarantine: bool = False, day_type: int = 0, transpose: int = 0,
                rule: str = "default", max_venue_edges: Optional[int] = None, variant: Sequence[str] = ()):
    """``nets``: the set's ACTIVE networks in order, each (beta, table [2, 2, 100] or None, age75, raw); ``x``, ``stage``,
    ``age``, ``sex``: per agent, halo agents included; ``p_contact``: the plan's float32 array [V].  Returns
    (cum [V, nk] as uint32 bit patterns, flagged [V, nk] bool: the venues whose sum raised a flag)."""
    unknown = set(variant) - set(VARIANTS)
    if unknown or rule not in ("default", "presum"):
        raise ValueError((rule, unknown))
    a = np.asarray(agent, dtype=np.int64).ravel()
    v = np.asarray(venue, dtype=np.int64).ravel()
    pc = np.asarray(p_contact, dtype=np.float32)
    V = len(pc)
    if max_venue_edges is None:
        max_venue_edges = int(np.bincount(v, minlength=1).max()) if len(v) else 0
    limit = term_limit_bits(0 if "window_not_shrunk" in variant else max_venue_edges)
    cum = np.zeros((V, len(nets)), dtype=np.uint32)
    flagged = np.zeros((V, len(nets)), dtype=bool)
    for k, (beta, table, age75, raw) in enumerate(nets):
        xs = source(x, stage, q_thr, has_quarantine, raw)
        with np.errstate(all="ignore"):
            if table is None:
                term = xs[a]
            else:
                w = np.asarray(table, dtype=np.float32).reshape(2, 2, 100)[day_type, np.asarray(sex), np.asarray(age)]
                if age75 and (transpose or "mask_forward" in variant):
                    w = (w * (np.asarray(age) > 75).astype(np.float32)).astype(np.float32)
                term = (w[a] * xs[a]).astype(np.float32)
            ok = in_window(term, limit, strict="strict_window" in variant)
            sums = np.zeros(V, dtype=np.int64)
            np.add.at(sums, v[ok], to_fx(term[ok], floor="floor" in variant))
            s = from_fx_once(sums) if "single_rounding" in variant else from_fx(sums)
            pos, neg = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
            pos[v[~ok & ~(term < 0)]] = True          # positive, +inf or NaN
            neg[v[~ok & ~(term > 0)]] = True          # negative, -inf or NaN
            if rule == "presum":
                s = np.where(pos | neg, F32(np.nan), s)
            else:
                s = np.where(pos & neg, F32(np.nan), np.where(pos, SATURATED, np.where(neg, -SATURATED, s)))
            bp = (F32(beta) * pc).astype(np.float32)
            cum[:, k] = bits((bp * s.astype(np.float32)).astype(np.float32))
        flagged[:, k] = pos | neg
    return cum, flagged


def nets_of(specs: Sequence, active: Sequence[str], betas: dict, edge_set: str) -> list:
    """The active networks of one edge set in accumulation order, as ``restate_set`` takes them.  ``specs``: every
    configured network (``plan.NetworkSpec``)."""
    from grad_june_amd import _native as N

    by_name = {s.name: s for s in specs}
    return [(float(betas[n]), None if by_name[n].table is None else np.asarray(by_name[n].table, dtype=np.float32),
             by_name[n].mask_kind == N.MASK_QL_AGE75, by_name[n].mask_kind == N.MASK_RAW)
            for n in active if by_name[n].edge_set == edge_set]


def restate(edge_sets: dict, p_contacts: dict, specs: Sequence, active: Sequence[str], betas: dict, x, *,
            rules: Optional[dict] = None, drop: Optional[dict] = None, **kw) -> dict:
    """{set name: (cum bits [V, nk], flagged [V, nk])} for every set with an active network.  ``rules``: {set name:
    "presum"} for the sets whose pass 1 k_tile_presum takes; ``drop``: {set name: bool [E]} edges left out of the sums
    but not of the window (misstatements: a dropped halo edge, a dropped agent of a run-form block)."""
    out = {}
    for name, es in edge_sets.items():
        nets = nets_of(specs, active, betas, name)
        if not nets:
            continue
        a, v = np.asarray(es["agent"]).ravel(), np.asarray(es["venue"]).ravel()
        mve = int(np.bincount(v, minlength=1).max()) if len(v) else 0
        if drop is not None and name in drop:
            a, v = a[~drop[name]], v[~drop[name]]
        out[name] = restate_set(a, v, p_contacts[name], nets, x, rule=(rules or {}).get(name, "default"),
                                max_venue_edges=mve, **kw)
    return out
