"""The infection-location attribution (include/gradjune_hip.h, gj_location_stats) restated in numpy from COO edge lists:
float64 arithmetic, Python integers for the fixed point, the same floor and remainder rule.

For an agent a with new_infected[a] == 1 and the step's active networks n in accumulation order:

    t_n[a] = w_n[a] * s0[a] * sum over the edges (a, v) of n's edge set of cum_n[v]
    T      = t_0 + t_1 + ...                                      (in that order)
    T finite and > 0:  c_n = floor(t_n / T * 2^30), the remainder 2^30 - sum c_n to the largest t_n (lowest index)
    otherwise:         2^30 to the background column

A term that is NaN or negative counts as 0 and sets ERR_VALUE.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

U = 1 << 30
ERR_LABEL, ERR_VALUE, ERR_ROWS = 1, 2, 4
MASK_RAW, MASK_Q, MASK_QL, MASK_QL_AGE75 = 0, 1, 2, 3


def mask_weight(kind: int, q: np.ndarray, table_row: Optional[np.ndarray], age: np.ndarray) -> np.ndarray:
    """w_n of gj_mask_kind, float64 [A]: 1 (RAW), q (Q), q * L (QL), q * L * (age > 75) (QL_AGE75)."""
    q = np.asarray(q, dtype=np.float64)
    if kind == MASK_RAW:
        return np.ones_like(q)
    w = q.copy()
    if kind >= MASK_QL:
        w = w * np.asarray(table_row, dtype=np.float64)
    if kind == MASK_QL_AGE75:
        w = w * (np.asarray(age) > 75).astype(np.float64)
    return w


def network_term(agent: np.ndarray, venue: np.ndarray, cum: np.ndarray, w: np.ndarray, s0: np.ndarray) -> np.ndarray:
    """t_n [A] in float64 from the COO edges (agent, venue) of the network's set and its per-venue sums ``cum`` [V]."""
    A = len(s0)
    with np.errstate(invalid="ignore", over="ignore"):
        sums = np.bincount(np.asarray(agent, dtype=np.int64), weights=np.asarray(cum, dtype=np.float64)[venue], minlength=A)
        return (np.asarray(w, dtype=np.float64) * np.asarray(s0, dtype=np.float64)) * sums


def shares(t: Sequence[float]):
    """One infection: (units per network as Python ints, units of the background column, error bits)."""
    t = [float(x) for x in t]
    err = 0
    for i, x in enumerate(t):
        if not x >= 0.0:                      # NaN or negative
            t[i], err = 0.0, err | ERR_VALUE
    T = 0.0
    for x in t:
        T = T + x
    if not (T > 0.0 and math.isfinite(T)):
        return [0] * len(t), U, err
    c = [int(math.floor(x / T * float(U))) for x in t]
    best = max(range(len(t)), key=lambda i: (t[i], -i))       # the largest term, lowest index on a tie
    c[best] += U - sum(c)
    assert all(v >= 0 for v in c) and sum(c) == U
    return c, 0, err


def location_stats(terms: np.ndarray, new_infected: np.ndarray, group: Optional[np.ndarray], n_groups: int,
                   cols: Sequence[int], n_cols: int, background: int, out: Optional[List[List[int]]] = None):
    """``terms``: float64 [n_nets, A] (``network_term`` per active network, in accumulation order).  Returns
    (out [n_groups][n_cols] as Python ints - ADDED to ``out`` when given -, error bits)."""
    out = [[0] * n_cols for _ in range(n_groups)] if out is None else [list(r) for r in out]
    err = 0
    nu = np.asarray(new_infected)
    for a in np.nonzero(nu != 0)[0]:          # (NaN != 0 too)
        if nu[a] != 1:
            err |= ERR_VALUE
            continue
        g = 0 if group is None else int(group[a])
        if not 0 <= g < n_groups:
            err |= ERR_LABEL
            continue
        c, bg, e = shares(terms[:, a])
        err |= e
        for i, units in enumerate(c):
            out[g][cols[i]] += units
        out[g][background] += bg
    return out, err


def step_terms(world: dict, tables: Optional[Dict[str, np.ndarray]], active: Sequence[str], cum: Dict[str, np.ndarray],
               s0: np.ndarray, day_type: int, qmask: Optional[np.ndarray]) -> np.ndarray:
    """[n_nets, A] for a world as gj_testlib.world_from returns it and the reference's eleven networks: ``cum[name]`` the
    per-venue sums of network ``name``, ``qmask`` the quarantine mask q (None: ones)."""
    import gj_testlib as L

    A = world["n_agents"]
    age, sex = np.asarray(world["age"]), np.asarray(world["sex"])
    q = np.ones(A) if qmask is None else np.asarray(qmask, dtype=np.float64)
    rows = []
    for name in active:
        es = world["edge_sets"][L.edge_set_name(name)]
        if name == "household":
            kind, row = MASK_RAW, None
        elif name in L.LEISURE or name == "care_visit":
            kind = MASK_QL_AGE75 if name == "care_visit" else MASK_QL
            row = np.asarray(tables[name])[day_type, sex, age]
        else:
            kind, row = MASK_Q, None
        rows.append(network_term(np.asarray(es["agent"]), np.asarray(es["venue"]), cum[name],
                                 mask_weight(kind, q, row, age), s0))
    return np.stack(rows) if rows else np.zeros((0, A))
