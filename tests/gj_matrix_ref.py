"""The who-infects-whom matrix (include/gradjune_hip.h, gj_infection_matrix_scatter / gj_infection_matrix_gather) restated
in numpy on top of tests/gj_infector_ref.py: float64 arithmetic, Python integers for the units.

Pass 1 is the infector series' pass 1 with one more index: an infection of agent a scatters exactly what
``gj_infector_ref.scatter`` scatters for it, into the plane ``group[a]`` of ``UG`` [V, stride, G] - so ``UG.sum(-1)`` is that
function's ``U`` - and an infection nobody transmitted is counted by the group of ``a``.  It is formed group by group:
the agents of one group at a time through ``gj_infector_ref.scatter``, whose rule treats every agent on its own.

Pass 2, for an agent b with transmission[b] > 0, every network i, every edge of b's row at a venue v whose cell has units,
and every g' with UG_i[v][g'] != 0:

    matrix[group[b]][g'] += rint( UG_i[v][g'] / 2^30 * (beta_i * pc[v]) * (m_i[b] * transmission[b]) / cum_i[v] * 2^30 )

each term a chain of float64 products and quotients in that order, rounded half to even on its own.
"""
from __future__ import annotations

import math
from typing import Iterator, List, Sequence, Tuple

import numpy as np

import gj_infector_ref as I

U = I.U
ERR_LABEL, ERR_VALUE, ERR_ROWS = I.ERR_LABEL, I.ERR_VALUE, I.ERR_ROWS


def scatter_by_group(nets: Sequence[I.Net], edges, cum, s0, new_infected, A: int, group, G: int):
    """Returns (UG {set: int64 [V, stride, G]}, unattributed by group: int64 [G], error bits).  ``group`` None: every
    agent in group 0.  A flagged agent (new_infected == 1) with a label outside [0, G) is skipped and sets ERR_LABEL."""
    nu = np.asarray(new_infected)
    group = np.zeros(A, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    UG = {s: np.zeros(c.shape + (G,), dtype=np.int64) for s, c in cum.items()}
    lost, err = np.zeros(G, dtype=np.int64), 0
    valid = (group >= 0) & (group < G)
    if np.any((nu == 1) & ~valid):
        err |= ERR_LABEL
    if np.any((nu != 0) & (nu != 1)):          # (NaN too) refused before its label is looked at
        err |= ERR_VALUE
    for g in range(G):
        mine = np.where(valid & (group == g) & (nu == 1), nu, np.zeros_like(nu))
        if not mine.any():
            continue
        units, unattributed, e, _ = I.scatter(nets, edges, cum, s0, mine, A)
        err |= e
        lost[g] = unattributed
        for s, u in units.items():
            UG[s][:, :, g] = u
    return UG, lost, err


def matrix_terms(nets: Sequence[I.Net], edges, cum, pc, UG, transmission, A: int, group, G: int
                 ) -> Iterator[Tuple[int, int, int, int]]:
    """(b, group[b], g', units) for every term of pass 2 whose UG cell is not zero, in the order of the walk."""
    rows = I.rows_of(edges, A)
    tr = np.asarray(transmission)
    for b in np.nonzero(tr > 0)[0]:
        g = 0 if group is None else int(group[b])
        if not 0 <= g < G:
            continue
        for net in nets:
            for v in rows[net.set][b]:
                cell = UG[net.set][v, net.column]
                if not cell.any():             # U, the sum of non-negative cells, is zero: nothing else is read
                    continue
                c = float(cum[net.set][v, net.column])
                if not (c > 0.0 and math.isfinite(c)):
                    continue
                beta_pc = float(np.float32(net.beta)) * float(pc[net.set][v])
                w = float(net.m[b]) * float(tr[b])
                for h in np.nonzero(cell)[0]:
                    t = int(cell[h]) / float(U) * beta_pc * w / c * float(U)
                    if not (t >= 0.0 and t < 2.0 ** 62):
                        continue
                    yield int(b), g, int(h), int(np.rint(t))


def matrix(nets: Sequence[I.Net], edges, cum, pc, UG, transmission, A: int, group, G: int) -> List[List[int]]:
    """The [G, G] matrix of one step - [infector's group][infected's group] - as Python ints."""
    out = [[0] * G for _ in range(G)]
    for _, g, h, units in matrix_terms(nets, edges, cum, pc, UG, transmission, A, group, G):
        out[g][h] += units
    return out
