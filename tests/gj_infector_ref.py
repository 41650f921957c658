"""The infector attribution (include/gradjune_hip.h, gj_infector_scatter / gj_infector_gather) restated in numpy from COO
edge lists: float64 arithmetic, Python integers for the units, the same floor, remainder and tie rules.

A step is described by its networks in accumulation order - ``Net`` - and, per edge set, the COO edges, the per-venue
sums ``cum`` [V, stride] and ``pc`` [V].

Pass 1, for an agent a with new_infected[a] == 1 (rows in COO order):

    t_i      = (w_i[a] * s0[a]) * sum over a's row of cum_i[v]         (NaN or negative: 0, ERR_VALUE) - the location term
    T        = t_0 + t_1 + ...                                         (in that order)
    T finite and > 0:  for every network with t_i > 0 and every edge e of its row
                       t_ie = (w_i[a] * s0[a]) * cum_i[v_e]            (NaN or negative: 0, ERR_VALUE)
                       u_ie = min(floor(t_ie / T * 2^30), 2^30)        added to U_i[v_e]
                       the remainder 2^30 - sum u to the largest t_ie (lowest i, then lowest position in the row)
    otherwise:         unattributed += 1

Pass 2, for an agent b with transmission[b] > 0:

    credit[b] = sum_i sum over b's row, U_i[v] != 0, of U_i[v] / 2^30 * (beta_i * pc[v]) * (m_i[b] * transmission[b]) / cum_i[v]
    caused[b] += credit[b];  out[group[b]] += round_half_even(credit[b] * 2^30)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

U = 1 << 30
ERR_LABEL, ERR_VALUE, ERR_ROWS = 1, 2, 4


@dataclass
class Net:
    set: str                 # edge set the network lives on
    column: int              # its column of that set's cum / U
    beta: float              # as the kernel holds it: a float32 value
    w: np.ndarray            # receiving-side weight, float64 [A]
    m: np.ndarray            # transmitting-side weight, float64 [A]


def rows_of(edges: Dict[str, Tuple[np.ndarray, np.ndarray]], A: int) -> Dict[str, List[np.ndarray]]:
    """{set: [the venues of agent a's edges, in COO order]}: a stable sort by agent."""
    rows = {}
    for s, (agent, venue) in edges.items():
        agent, venue = np.asarray(agent, dtype=np.int64), np.asarray(venue, dtype=np.int64)
        order = np.argsort(agent, kind="stable")
        bounds = np.cumsum(np.bincount(agent, minlength=A))[:-1]
        rows[s] = np.split(venue[order], bounds)
    return rows


def location_terms(nets: Sequence[Net], rows, cum, s0, a: int) -> List[float]:
    """[t_i] of agent a before the NaN / negative rule, as gj_location_ref.network_term forms them."""
    t = []
    with np.errstate(invalid="ignore", over="ignore"):
        for net in nets:
            total = 0.0
            for v in rows[net.set][a]:
                total = total + float(cum[net.set][v, net.column])
            t.append(float((net.w[a] * float(s0[a])) * total))
    return t


def scatter(nets: Sequence[Net], edges, cum, s0, new_infected, A: int):
    """Returns (U {set: int64 [V, stride]}, unattributed, error bits, touched {set: int64 [V]}: the edges of attributed
    new infections that touch each venue - the floor's bound per cell)."""
    rows = rows_of(edges, A)
    units = {s: [[0] * c.shape[1] for _ in range(c.shape[0])] for s, c in cum.items()}
    touched = {s: np.zeros(c.shape[0], dtype=np.int64) for s, c in cum.items()}
    unattributed, err = 0, 0
    nu = np.asarray(new_infected)
    for a in np.nonzero(nu != 0)[0]:          # (NaN != 0 too)
        if nu[a] != 1:
            err |= ERR_VALUE
            continue
        t = location_terms(nets, rows, cum, s0, a)
        for i, x in enumerate(t):
            if not x >= 0.0:
                t[i], err = 0.0, err | ERR_VALUE
        T = 0.0
        for x in t:
            T = T + x
        if not (T > 0.0 and math.isfinite(T)):
            unattributed += 1
            continue
        given, best = 0, None                 # best: (t_ie, -i, -position) and its cell
        for i, net in enumerate(nets):
            if not t[i] > 0.0:
                continue
            ws = net.w[a] * float(s0[a])
            for pos, v in enumerate(rows[net.set][a]):
                with np.errstate(invalid="ignore", over="ignore"):
                    te = float(ws * float(cum[net.set][v, net.column]))
                if not te >= 0.0:
                    te, err = 0.0, err | ERR_VALUE
                r = te / T * float(U)
                u = U if r >= float(U) else int(math.floor(r))
                units[net.set][v][net.column] += u
                given += u
                key = (te, -i, -pos)
                if best is None or key > best[0]:
                    best = (key, net.set, v, net.column)
        for s in {net.set for i, net in enumerate(nets) if t[i] > 0.0}:
            np.add.at(touched[s], rows[s][a], 1)
        if best is not None and given < U:
            units[best[1]][best[2]][best[3]] += U - given
    return {s: np.array(u, dtype=np.int64).reshape(cum[s].shape) for s, u in units.items()}, unattributed, err, touched


def gather(nets: Sequence[Net], edges, cum, pc, units, transmission, A: int, group=None, n_groups: int = 1):
    """Returns (credit float64 [A], out [n_groups] as Python ints, error bits)."""
    rows = rows_of(edges, A)
    credit, out, err = np.zeros(A), [0] * n_groups, 0
    tr = np.asarray(transmission)
    for b in np.nonzero(tr > 0)[0]:
        g = 0 if group is None else int(group[b])
        if not 0 <= g < n_groups:
            err |= ERR_LABEL
            continue
        acc = 0.0
        for net in nets:
            for v in rows[net.set][b]:
                u = int(units[net.set][v, net.column])
                if u == 0:
                    continue
                c = float(cum[net.set][v, net.column])
                if not (c > 0.0 and math.isfinite(c)):
                    err |= ERR_VALUE
                    continue
                acc += u / float(U) * (float(np.float32(net.beta)) * float(pc[net.set][v])) * (net.m[b] * float(tr[b])) / c
        if acc == 0.0:
            continue
        if not (acc > 0.0 and acc < 2.0 ** 32):
            err |= ERR_VALUE
            continue
        credit[b] = acc
        out[g] += int(round(acc * float(U)))      # round half to even, as llrint
    return credit, out, err


def step_nets(world: dict, tables, active: Sequence[str], betas: Dict[str, float], day_type: int,
              qmask: Optional[np.ndarray]) -> List[Net]:
    """The ``Net`` list of a world as gj_testlib.world_from returns it and the reference's eleven networks."""
    import gj_testlib as L

    per_set: Dict[str, int] = {}
    nets = []
    for name in active:
        s = L.edge_set_name(name)
        m, w = L.network_weights(name, world, tables, day_type, qmask)
        nets.append(Net(s, per_set.get(s, 0), float(betas[name]), np.asarray(w, dtype=np.float64), np.asarray(m, dtype=np.float64)))
        per_set[s] = per_set.get(s, 0) + 1
    return nets
