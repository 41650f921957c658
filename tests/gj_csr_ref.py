"""The two passes of the CSR layout - k_venue_reduce, k_combine_long and the sum loop of k_agent_gather in
csrc/gradjune_hip.hip - restated in numpy float32, bit for bit.  This file SPECIFIES the order of every sum of the layout.

The library is built with -ffp-contract=off: every product and every sum below is one float32 rounding, as on the device,
and group_sum (csrc/gj_device.h) is a fixed xor butterfly.  Ordered sums are taken by `ordered_sums` (an explicit
float32 loop, vectorised over the sums), never by np.sum / np.add.reduce, which add pairwise.

Inputs are a host plan's own arrays (v_rowptr, v_agent, v_pcontact, a_rowptr, a_venue, blocks, long_rows, agent_class), the
leisure tables and the launch's active networks in accumulation order.  The SCHEDULE is the plan's; which networks form a
set's columns is formed here as the launch code forms it (`launch_nets` = engine.params, `groups_of` = group_networks +
classify_group + check_group of gradjune_hip.hip).

Pass 1, per active set and per network k of it (column k of cum = the k-th ACTIVE network of the set):

    src     = transmission                      a set read raw (its first network is MASK_RAW), or quarantine off:
                                                then q_transmission is neither written nor read (engine._prep,
                                                do_venue_reduce: qtrans = has_quarantine ? q_transmission : transmission)
            = fp32(q * transmission)            otherwise, q = stage < q_threshold in {0, 1}; no clamp: 0 * inf is a NaN
    x[e]    = src[agent(e)]                     a set without tables
            = fp32(tab_k[day_type][cls[agent(e)]] * src[agent(e)])     a set with tables (then every network has one)
    y[v]    = fp32(beta_k * p_contact[v])
    term[e] = fp32(x[e] * y[venue(e)])
    STREAM block, lanes == 1:  cum[v] = the terms of row v added one after the other in row order, from +0.0
    STREAM block, lanes == G:  lane l adds the terms at row positions l, l + G, l + 2G, ...; then, on the G partials,
                               p = p + p[lane ^ off] for off = G/2 ... 1; cum[v] = p[0]
    LONG block (edges [e0, e1) of one venue, 256 threads):
                               thread t adds the terms at e0 + t, e0 + t + 256, ... (the unrolled and the remainder loop
                               of the kernel add in this one order); the 64-lane butterfly per wave; the four wave sums
                               added in wave order from +0.0 -> partial[slot]
    k_combine_long:            cum[v] = partial[slot0] ... partial[slot1 - 1] added in slot order from +0.0
A set with several networks and no table (accepted by the CSR launch: check_group(plain_is_single = false)) has
term = fp32(src * y_k) per network, in STREAM and in LONG blocks alike.
Not written: the columns k >= nk of an active set and every column of a set without an active network.

Pass 2, per owned agent a (c = cls[a] if any active set has a table, else 0; q as above, 1 with quarantine off):

    single-network branch (nk == 1 and the mask RAW or Q):
        w = susc  (RAW)  or  fp32(q * susc)  (Q);  acc = the fp32(cum[v][0] * w) of row a added in row order from +0.0
        ts = fp32(ts + acc)
    multi-network branch (everything else, a single QL network included):
        w_k = susc (RAW) or q;   mask >= QL: w_k = fp32(w_k * tab_k[day_type][c]);   mask != RAW: w_k = fp32(w_k * susc);
        QL_AGE75: w_k = fp32(w_k * ((c % 100) > 75));   acc_k = the fp32(cum[v][k] * w_k) of row a added in row order
        ts = fp32(ts + acc_k) for k = 0 ... nk - 1
    sets in the order of the launch's groups (first appearance among the active networks); ts starts at +0.0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

F32 = np.float32
THREADS = 256              # kThreads
WAVE = 64                  # kWave
STREAM_EDGES = 2048        # GJ_STREAM_EDGES = kEdgesPerThread * kThreads
MAX_SETS = 12              # GJ_MAX_SETS
MAX_NETS = 16              # GJ_MAX_NETS
MAX_NETS_PER_SET = 8       # GJ_MAX_NETS_PER_SET
TABLE_SIZE = 400           # GJ_TABLE_SIZE: [day type 2][class 200]
MASK_RAW, MASK_Q, MASK_QL, MASK_QL_AGE75 = 0, 1, 2, 3
LANES = (1, 4, 16, 64)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def f32_mul(a, b) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (np.asarray(a, dtype=np.float32) * np.asarray(b, dtype=np.float32)).astype(np.float32)


def ordered_sums(terms: np.ndarray, first: np.ndarray, count: np.ndarray, stride: int = 1) -> np.ndarray:
    """s_i = (..((+0.0 + t[first_i]) + t[first_i + stride]) + ..) over count_i terms, every add one float32 rounding.
    Vectorised ACROSS the sums (step j adds term j of every sum that has one), sequential inside each."""
    terms = np.asarray(terms, dtype=np.float32)
    first = np.asarray(first, dtype=np.int64).ravel()
    count = np.asarray(count, dtype=np.int64).ravel()
    n = len(first)
    out = np.zeros(n, dtype=np.float32)
    if n == 0 or count.max(initial=0) <= 0:
        return out
    order = np.argsort(-count, kind="stable")
    f, c = first[order], count[order]
    steps = int(c[0])
    alive = np.searchsorted(-c, -np.arange(steps), side="left")      # sums with more than j terms: a prefix
    acc = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(steps):
            m = int(alive[j])
            acc[:m] = acc[:m] + terms[f[:m] + j * stride]
    out[order] = acc
    return out


def butterfly(p: np.ndarray) -> np.ndarray:
    """group_sum<G> on [n, G] partials: p = p + p[lane ^ off] for off = G/2 ... 1; lane 0's value."""
    p = np.asarray(p, dtype=np.float32)
    G = p.shape[1]
    lane = np.arange(G)
    off = G // 2
    with np.errstate(all="ignore"):
        while off:
            p = (p + p[:, lane ^ off]).astype(np.float32)
            off >>= 1
    return p[:, 0]


def strided_counts(n, G: int) -> np.ndarray:
    """[len(n), G]: how many of the positions l, l + G, l + 2G, ... lie below n, per lane l."""
    n = np.asarray(n, dtype=np.int64)
    return np.maximum(0, -(-(n[:, None] - np.arange(G)[None, :]) // G))


# ---- the launch's networks and sets -------------------------------------------------------------------------------------------
@dataclass
class Net:
    """One active network as gj_step_params holds it."""
    set: int
    beta: float
    mask: int
    table: int            # row of the tables array, -1: none


@dataclass
class Group:
    """The active networks of one edge set (gradjune_hip.hip: Groups + NetGroup)."""
    set: int
    nk: int
    beta: List[np.float32]
    mask: List[int]
    table: List[int]      # -1: no table
    raw: bool
    leisure: bool


def tables_of(specs) -> Optional[np.ndarray]:
    """[n_tables, 2, 200] float32: one row per network that has a table, in the order of the plan's network list
    (DevicePlan.table_index)."""
    tabs = [np.asarray(s.table, dtype=np.float32).reshape(2, 200) for s in specs if s.table is not None]
    return np.stack(tabs) if tabs else None


def launch_nets(specs, active: Sequence[str], betas: Dict[str, float], set_index: Dict[str, int]) -> List[Net]:
    """engine.params: the active networks in the order given, beta as float32, the table row by the network's name."""
    by_name = {s.name: s for s in specs}
    table_index, n = {}, 0
    for s in specs:
        if s.table is not None:
            table_index[s.name] = n
            n += 1
    assert len(active) <= MAX_NETS
    return [Net(set_index[by_name[a].edge_set], float(F32(betas[a])), int(by_name[a].mask_kind), table_index.get(a, -1))
            for a in active]


def strides_of(specs, set_index: Dict[str, int]) -> List[int]:
    """cum_stride per set: the networks CONFIGURED on it, at least 1 (DevicePlan)."""
    out = [1] * len(set_index)
    count: Dict[str, int] = {}
    for s in specs:
        count[s.edge_set] = count.get(s.edge_set, 0) + 1
    for name, i in set_index.items():
        out[i] = max(1, count.get(name, 1))
    return out


def groups_of(nets: Sequence[Net], strides: Sequence[int]) -> List[Group]:
    """group_networks + classify_group + check_group(plain_is_single = false): sets in the order of their first active
    network; the networks of one set adjacent, at most `stride` of them, RAW and masked kinds not mixed; a set with a
    table has one for every network."""
    groups: List[Group] = []
    seen = set()
    for n in nets:
        assert MASK_RAW <= n.mask <= MASK_QL_AGE75
        tabled = n.mask >= MASK_QL
        assert n.table >= 0 or not tabled, "a table network has its row of the tables array"
        if groups and groups[-1].set == n.set:
            g = groups[-1]
            assert g.nk < strides[n.set], "more active networks than cum has columns"
            assert g.raw == (n.mask == MASK_RAW), "RAW and masked kinds on one set"
            g.nk += 1
        else:
            assert n.set not in seen, "networks of one set must be adjacent"
            seen.add(n.set)
            g = Group(n.set, 1, [], [], [], n.mask == MASK_RAW, False)
            groups.append(g)
        g.beta.append(F32(n.beta))
        g.mask.append(n.mask)
        g.table.append(n.table if tabled else -1)
        g.leisure = g.leisure or tabled
    for g in groups:
        assert g.nk <= MAX_NETS_PER_SET
        if g.leisure:
            assert all(t >= 0 for t in g.table), "a set with a table needs one per network"
    return groups


def source(transmission, stage_ext, q_thr: float, has_q: bool, raw: bool) -> np.ndarray:
    """What pass 1 gathers from: `transmission` itself for a raw set and whenever quarantine is off (q_transmission is
    then not read - and not written: gj_quarantine_transmission returns at once); fp32(q * transmission) otherwise."""
    x = np.ascontiguousarray(transmission, dtype=np.float32)
    if raw or not has_q:
        return x
    q = (np.asarray(stage_ext, dtype=np.float32) < F32(q_thr)).astype(np.float32)
    return f32_mul(q, x)


# ---- pass 1 ----------------------------------------------------------------------------------------------------------------------
def check_schedule(rp: np.ndarray, blocks: np.ndarray, long_rows: np.ndarray) -> None:
    """What the sums below rely on (asserted on build_schedule by tests/test_plan_host.py and tests/test_csr_ref.py)."""
    st = blocks[blocks[:, 1] == 0]
    assert (rp[st[:, 2]] == st[:, 4]).all() and (rp[st[:, 3]] == st[:, 5]).all()
    assert ((st[:, 5] - st[:, 4]) <= STREAM_EDGES).all() and np.isin(st[:, 7], LANES).all()
    lg = blocks[blocks[:, 1] == 1]
    assert (lg[:, 3] == lg[:, 2] + 1).all() and (lg[:, 4] < lg[:, 5]).all()
    assert (rp[lg[:, 2]] <= lg[:, 4]).all() and (lg[:, 5] <= rp[lg[:, 2] + 1]).all()


def cum_of_set(hs, blocks: np.ndarray, long_rows: np.ndarray, g: Group, src: np.ndarray, cls: np.ndarray,
               tables: Optional[np.ndarray], day_type: int) -> np.ndarray:
    """cum [V, nk] float32 of one active set.  `hs`: the plan's HostEdgeSet; `blocks`, `long_rows`: the rows of the plan's
    schedule that belong to this set; `src`: `source(...)` per agent, halo agents included."""
    rp = np.asarray(hs.v_rowptr, dtype=np.int64)
    va = np.asarray(hs.v_agent, dtype=np.int64)
    pc = np.asarray(hs.v_pcontact, dtype=np.float32)
    blocks, long_rows = np.asarray(blocks, dtype=np.int64), np.asarray(long_rows, dtype=np.int64)
    V = len(rp) - 1
    deg = np.diff(rp)
    check_schedule(rp, blocks, long_rows)
    venue_of_edge = np.repeat(np.arange(V), deg)
    cum = np.zeros((V, g.nk), dtype=np.float32)
    written = np.zeros(V, dtype=np.int64)
    stream, long_ = blocks[blocks[:, 1] == 0], blocks[blocks[:, 1] == 1]
    for k in range(g.nk):
        x = np.asarray(src, dtype=np.float32)[va]
        if g.leisure:
            tab = tables[g.table[k]][day_type]                       # [200]
            x = f32_mul(tab[np.asarray(cls, dtype=np.int64)[va]], x)
        y = f32_mul(g.beta[k], pc)
        term = f32_mul(x, y[venue_of_edge])
        for G in LANES:
            rows = stream[stream[:, 7] == G]
            if len(rows) == 0:
                continue
            vs = np.concatenate([np.arange(r[2], r[3]) for r in rows])
            if k == 0:
                written[vs] += 1
            if G == 1:
                cum[vs, k] = ordered_sums(term, rp[vs], deg[vs], 1)
            else:
                first = rp[vs][:, None] + np.arange(G)[None, :]
                part = ordered_sums(term, first, strided_counts(deg[vs], G), G).reshape(len(vs), G)
                cum[vs, k] = butterfly(part)
        if len(long_):
            first = long_[:, 4][:, None] + np.arange(THREADS)[None, :]
            part = ordered_sums(term, first, strided_counts(long_[:, 5] - long_[:, 4], THREADS), THREADS)
            waves = butterfly(part.reshape(-1, WAVE)).reshape(len(long_), THREADS // WAVE)
            s = np.zeros(len(long_), dtype=np.float32)
            with np.errstate(all="ignore"):
                for w in range(THREADS // WAVE):
                    s = (s + waves[:, w]).astype(np.float32)
            partial = dict(zip(long_[:, 6].tolist(), s))
            for (_, v, s0, s1) in long_rows.tolist():
                acc = F32(0.0)
                with np.errstate(all="ignore"):
                    for slot in range(s0, s1):
                        acc = F32(acc + partial[slot])
                cum[v, k] = acc
                if k == 0:
                    written[v] += 1
    assert (written == 1).all(), "every venue in exactly one STREAM block or one long row"
    return cum


def restate_cum(host, groups: Sequence[Group], tables, transmission, *, stage_ext, has_q: bool, q_thr: float,
                day_type: int) -> Dict[str, np.ndarray]:
    """{set name: cum [V, nk] float32} of the ACTIVE sets."""
    out = {}
    for g in groups:
        hs = host.sets[g.set]
        src = source(transmission, stage_ext, q_thr, has_q, g.raw)
        out[hs.name] = cum_of_set(hs, host.blocks[host.blocks[:, 0] == g.set], host.long_rows[host.long_rows[:, 0] == g.set],
                                  g, src, host.agent_class, tables, day_type)
    return out


# ---- pass 2 ----------------------------------------------------------------------------------------------------------------------
def agent_weights(g: Group, k: int, susc, q, c, tables, day_type: int) -> np.ndarray:
    """w_k of the multi-network branch, its multiplications in the kernel's order."""
    m = g.mask[k]
    w = susc if m == MASK_RAW else q
    if m >= MASK_QL:
        w = f32_mul(w, tables[max(g.table[k], 0)][day_type][c])
    if m != MASK_RAW:
        w = f32_mul(w, susc)
    if m == MASK_QL_AGE75:
        w = f32_mul(w, ((c % 100) > 75).astype(np.float32))
    return np.asarray(w, dtype=np.float32)


def ts_of_agents(host, groups: Sequence[Group], tables, cums: Dict[str, np.ndarray], *, susc, stage, has_q: bool,
                 q_thr: float, day_type: int) -> np.ndarray:
    """trans_susc [n_agents] float32 from the sets' cum arrays ([V, >= nk]; columns k >= nk are not read)."""
    A = host.n_agents
    susc = np.ascontiguousarray(susc, dtype=np.float32)
    assert len(susc) == A
    q = np.ones(A, dtype=np.float32)
    if has_q:
        q = (np.asarray(stage, dtype=np.float32)[:A] < F32(q_thr)).astype(np.float32)
    c = np.zeros(A, dtype=np.int64)
    if any(g.leisure for g in groups):
        c = np.asarray(host.agent_class, dtype=np.int64)[:A]
    ts = np.zeros(A, dtype=np.float32)
    for g in groups:
        hs = host.sets[g.set]
        rp = np.asarray(hs.a_rowptr, dtype=np.int64)
        av = np.asarray(hs.a_venue, dtype=np.int64)
        deg = np.diff(rp)
        agent_of_edge = np.repeat(np.arange(A), deg)
        cum = np.asarray(cums[hs.name], dtype=np.float32)
        if g.nk == 1 and g.mask[0] <= MASK_Q:
            ws = [susc if g.mask[0] == MASK_RAW else f32_mul(q, susc)]
        else:
            ws = [agent_weights(g, k, susc, q, c, tables, day_type) for k in range(g.nk)]
        for k, w in enumerate(ws):
            acc = ordered_sums(f32_mul(cum[av, k], w[agent_of_edge]), rp[:-1], deg, 1)
            with np.errstate(all="ignore"):
                ts = (ts + acc).astype(np.float32)
    return ts


# ---- the same sums in float64, for the CPU checks of tests/test_csr_ref.py ---------------------------------------------------
def cum_float64(host, groups: Sequence[Group], tables, transmission, *, stage_ext, has_q, q_thr, day_type):
    """{set: (sum [V, nk], sum of |terms| [V, nk], terms [V])} with every term x * y taken in float64 from the float32
    inputs src, tab_k and y = fp32(beta_k * p_contact) - no rounding inside a term, none in the sum (to float64)."""
    out = {}
    for g in groups:
        hs = host.sets[g.set]
        rp = np.asarray(hs.v_rowptr, dtype=np.int64)
        va = np.asarray(hs.v_agent, dtype=np.int64)
        V = len(rp) - 1
        ve = np.repeat(np.arange(V), np.diff(rp))
        src = source(transmission, stage_ext, q_thr, has_q, g.raw).astype(np.float64)
        s, sa = np.zeros((V, g.nk)), np.zeros((V, g.nk))
        for k in range(g.nk):
            x = src[va]
            if g.leisure:
                x = tables[g.table[k]][day_type][np.asarray(host.agent_class, dtype=np.int64)[va]].astype(np.float64) * x
            y = f32_mul(g.beta[k], hs.v_pcontact).astype(np.float64)
            t = x * y[ve]
            s[:, k] = np.bincount(ve, weights=t, minlength=V)
            sa[:, k] = np.bincount(ve, weights=np.abs(t), minlength=V)
        out[hs.name] = (s, sa, np.diff(rp))
    return out


def ts_float64(host, groups: Sequence[Group], tables, cums, *, susc, stage, has_q, q_thr, day_type):
    """(sum [A], sum of |terms| [A], terms [A]): every term cum[v][k] * w_k in float64, w_k the exact product of its
    float32 factors; `cums` as for ts_of_agents (the float32 values pass 2 reads)."""
    A = host.n_agents
    susc = np.asarray(susc, dtype=np.float64)
    q = np.ones(A)
    if has_q:
        q = (np.asarray(stage, dtype=np.float32)[:A] < F32(q_thr)).astype(np.float64)
    c = np.asarray(host.agent_class, dtype=np.int64)[:A]
    s, sa, n = np.zeros(A), np.zeros(A), np.zeros(A, dtype=np.int64)
    for g in groups:
        hs = host.sets[g.set]
        rp = np.asarray(hs.a_rowptr, dtype=np.int64)
        av = np.asarray(hs.a_venue, dtype=np.int64)
        ae = np.repeat(np.arange(A), np.diff(rp))
        for k in range(g.nk):
            m = g.mask[k]
            w = susc.copy() if m == MASK_RAW else q * susc
            if m >= MASK_QL:
                w = w * tables[g.table[k]][day_type][c].astype(np.float64)
            if m == MASK_QL_AGE75:
                w = w * ((c % 100) > 75)
            t = np.asarray(cums[hs.name], dtype=np.float32)[av, k].astype(np.float64) * w[ae]
            s += np.bincount(ae, weights=t, minlength=A)
            sa += np.bincount(ae, weights=np.abs(t), minlength=A)
            n += np.diff(rp)
    return s, sa, n
