"""The transmission tree (include/gradjune_hip.h, gj_infection_tree) restated in numpy and Python integers, on top of
gj_infector_ref.py (the terms, the shares u and the best pair are gj_infector_scatter's) and gj_philox_ref.py (the draw).

For an agent a with new_infected[a] == 1:

    draw       one Philox4x32-10 block, counter (agent_offset + a, step | 2^60), key seed:
               r1 = word 0 & (2^30 - 1), R = word 2 | word 3 << 32
    pair       t_i, T, t_ie, u_ie as in gj_infector_ref.scatter.  T not finite or not > 0: infector -2, via background,
               venue -1.  Otherwise the pairs in canonical order - edge set (``set_order``: the plan's), position in a's
               row, the network's column - with given = sum u: r1 < given picks the first pair whose inclusive prefix sum
               exceeds r1, otherwise the best pair (largest t_ie, lowest network, lowest position)
    infector   over the members b of the venue in row order (COO order, a stable sort by venue): b == a: 0; w = m_i[b] *
               transmission[b], NaN or <= 0: 0; W = min(floor(w * 2^36), 2^46) (saturated: ERR_VALUE); S = sum W;
               S == 0: infector -3, unresolved += 1; else target = (R * S) >> 64 and the first member whose inclusive prefix
               sum exceeds target, plus agent_offset
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np

import gj_infector_ref as I
import gj_philox_ref as P

U = I.U
ERR_VALUE, ERR_ROWS = I.ERR_VALUE, I.ERR_ROWS
WEIGHT_BITS, WEIGHT_CAP = 36, 46
MAX_VENUE_ROW = 1 << 18
NEVER, NOBODY, UNRESOLVED = -1, -2, -3


def draw(seed: int, step: int, agents):
    """(r1 [n], R [n]) as Python-int lists for the global agent ids ``agents``."""
    agents = np.asarray(agents, dtype=np.uint64)
    w = P._block(seed & 0xFFFFFFFFFFFFFFFF, step | (1 << 60), agents)
    r1 = [int(x) & (U - 1) for x in w[0]]
    R = [int(lo) | (int(hi) << 32) for lo, hi in zip(w[2], w[3])]
    return r1, R


def venue_members(edges, n_venues: Dict[str, int]):
    """{set: [the agents of venue v's edges, in COO order]}: a stable sort by venue."""
    rows = {}
    for s, (agent, venue) in edges.items():
        agent, venue = np.asarray(agent, dtype=np.int64), np.asarray(venue, dtype=np.int64)
        order = np.argsort(venue, kind="stable")
        bounds = np.cumsum(np.bincount(venue, minlength=n_venues[s]))[:-1]
        rows[s] = np.split(agent[order], bounds)
    return rows


def pairs_of(nets: Sequence[I.Net], rows, cum, s0, a: int, set_order: Sequence[str]):
    """(pairs, T, err) of agent a: pairs = [(set, venue, network index, u, t_ie, position)] in canonical order, or None
    when nobody transmitted."""
    err = 0
    t = I.location_terms(nets, rows, cum, s0, a)
    for i, x in enumerate(t):
        if not x >= 0.0:
            t[i], err = 0.0, err | ERR_VALUE
    T = 0.0
    for x in t:
        T = T + x
    if not (T > 0.0 and math.isfinite(T)):
        return None, T, err
    pairs = []
    for s in set_order:
        on_set = sorted((net.column, i) for i, net in enumerate(nets) if net.set == s)
        if not on_set:
            continue
        for pos, v in enumerate(rows[s][a]):
            for column, i in on_set:
                if not t[i] > 0.0:
                    continue
                ws = nets[i].w[a] * float(s0[a])
                with np.errstate(invalid="ignore", over="ignore"):
                    te = float(ws * float(cum[s][v, column]))
                if not te >= 0.0:
                    te, err = 0.0, err | ERR_VALUE
                x = te / T * float(U)
                pairs.append((s, int(v), i, U if x >= float(U) else int(math.floor(x)), te, pos))
    return pairs, T, err


def pick_pair(pairs, r1: int):
    """The pair that r1 selects."""
    given = sum(p[3] for p in pairs)
    if r1 < given:
        prefix = 0
        for p in pairs:
            prefix += p[3]
            if prefix > r1:
                return p
    return max(pairs, key=lambda p: (p[4], -p[2], -p[5]))


def weights_of(members, a: int, m, transmission):
    """([W_b], error bits) of a venue's members for the infected agent a and the transmitting-side weights m."""
    W, err = [], 0
    for b in members:
        w = 0.0 if b == a else float(m[b]) * float(transmission[b])
        if not w > 0.0:
            W.append(0)
            continue
        x = w * float(1 << WEIGHT_BITS)
        if x >= float(1 << WEIGHT_CAP):
            W.append(1 << WEIGHT_CAP)
            err |= ERR_VALUE
        else:
            W.append(int(math.floor(x)))
    return W, err


def pick_member(W, R: int):
    """The position in the row that R selects, or None when no member has a weight."""
    S = sum(W)
    if S == 0:
        return None
    target = (R * S) >> 64
    prefix = 0
    for j, w in enumerate(W):
        prefix += w
        if prefix > target:
            return j
    raise AssertionError("target < S")


def infection_tree(nets: Sequence[I.Net], edges, cum, s0, new_infected, transmission, cols: Sequence[int], n_cols: int,
                   background: int, seed: int, step: int, A: int, set_order: Sequence[str], agent_offset: int = 0,
                   row_value: int = 0, out=None):
    """Returns dict(infector, via, venue, row_of: int32 [A]; counts: int64 [n_cols]; unresolved, err: int) - on top of
    ``out`` (the arrays of an earlier call) when given."""
    rows = I.rows_of(edges, A)
    members = venue_members(edges, {s: c.shape[0] for s, c in cum.items()})
    if out is None:
        out = dict(infector=np.full(A, NEVER, np.int32), via=np.full(A, -1, np.int32), venue=np.full(A, -1, np.int32),
                   row_of=np.full(A, -1, np.int32), counts=np.zeros(n_cols, np.int64), unresolved=0, err=0)
    nu = np.asarray(new_infected)
    flagged = np.nonzero(nu != 0)[0]              # (NaN != 0 too)
    r1s, Rs = draw(seed, step, flagged + agent_offset) if len(flagged) else ([], [])
    for a, r1, R in zip(flagged, r1s, Rs):
        if nu[a] != 1:
            out["err"] |= ERR_VALUE
            continue
        pairs, _, err = pairs_of(nets, rows, cum, s0, a, set_order) if nets else (None, 0.0, 0)
        out["err"] |= err
        out["row_of"][a] = row_value
        if not pairs:
            out["infector"][a], out["via"][a], out["venue"][a] = NOBODY, background, -1
            out["counts"][background] += 1
            continue
        s, v, i, _, _, _ = pick_pair(pairs, r1)
        out["via"][a], out["venue"][a] = cols[i], v
        out["counts"][cols[i]] += 1
        W, err = weights_of(members[s][v], a, nets[i].m, transmission)
        out["err"] |= err
        j = pick_member(W, R)
        if j is None:
            out["infector"][a] = UNRESOLVED
            out["unresolved"] += 1
        else:
            out["infector"][a] = agent_offset + int(members[s][v][j])
    return out
