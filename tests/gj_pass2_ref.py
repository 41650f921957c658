"""Pass 2 of the tiled step per agent - phase C + phase D of csrc/gj_tiled.h (k_tile_venues mode 0 / 2, k_tile_agents,
k_tile_epilogue) - restated in numpy float32 / int64 from the EDGE LISTS, bit for bit.

The library is built with -ffp-contract=off, so every float32 product and sum below is one rounding, as on the device.
Nothing here reads a tile table, a slot or a descriptor; the only inputs that come from a plan are the FORM each set
takes (``forms_of_plan``) and the test knob ``direct_table_floats``.

The step's network groups (``groups``) come in LAUNCH order: the order in which the edge sets first appear in the list
of active networks - that, not the set ids, is the order in which phase D takes the direct sets.

Workspace form (a set that is neither direct nor in the run form; and what the run form leaves in the tiled arrays).
Phase C writes one float32 per edge:

    plain set:    x = cum[v][0]
    leisure set:  a = 0;  a = fl(a + fl(w2_k[class] * cum[v][k]))   over the set's active networks k, in order

(w2: the receiving side's class weight - the table entry, times [age > 75] for a care-visit kind of network; with
``transpose`` the plain table entry).  Phase D converts each with rint(x * 2^32) (round half to even), adds the integers
exactly and reads back fl32(fp64(sum) * 2^-32).  A value with |x| > 262144 (compared on the bit patterns: 262144.0 itself
is inside), an infinity or a NaN raises the agent's POS (``not x < 0``) and / or NEG (``not x > 0``) flag instead of
adding.  One flag reads back +-1e30, both read back NaN.

Order of the sets.  The masked sets (raw == 0) first.  Under quarantine an agent with ``not stage < q_thr`` then has its
sum zeroed and a SINGLE flag cleared (both flags - a NaN - stay).  The raw sets (household) are added after that.

Direct and run forms.  No fixed point, no window.  With the workspace sums read back into ``acc``, every work item -
(direct set in launch order, venue group, pair of ELL columns), in that order - adds in float32

    acc = fl(acc + fl(fl(0 + (ok0 ? x0 : 0)) + (ok1 ? x1 : 0)))

x per entry as in phase C; an entry counts if its venue lies in the item's venue group and - for a masked set - its
agent is not quarantined.  The ELL column of an edge is its rank among the agent's edges of the set in COO order.  The
run form is one item: the agent's primary edge (the first edge in COO order to its smallest venue); its other edges go
through the workspace.  The venue groups follow from the launch layer's LDS rule, written out in ``venue_groups``.

``agent_sums`` is acc; ``trans_susc`` = fl(susceptibility * acc)."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

F32 = np.float32
WINDOW_BITS = 0x48800000            # the bit pattern of 262144.0f = 2^(50 - 32)
SATURATED = np.float32(1.0e30)
FX_SCALE = 2.0 ** 32
MAGIC = 6755399441055744.0          # 1.5 * 2^52
MAGIC_BITS = 0x4338000000000000
U32 = 2.0 ** -24                    # unit roundoff of float32
FX_AGENT_HALF = 2.0 ** -33
SLACK = 1.0 + 2.0 ** -20

# the launch layer's LDS budget for the venue tables of the direct form, in floats: 160 KiB, less two class-weight
# buffers of 8 x 200 floats and 64 floats of slack behind each of the two table regions
LDS_FLOATS = 160 * 1024 // 4
WEIGHT_FLOATS = 8 * 200
BUDGET = LDS_FLOATS - 2 * WEIGHT_FLOATS - 2 * 64
MIN_CAP0 = 8                        # GJ_MAX_NETS_PER_SET


# ---- fixed point ---------------------------------------------------------------------------------------------------------
def to_fx(x: np.ndarray) -> np.ndarray:
    """rint(x * 2^32) as int64 (round half to even); x float32 inside the window."""
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * FX_SCALE).astype(np.int64)


def to_fx_magic(x: np.ndarray) -> np.ndarray:
    """The device's conversion: the bit pattern of fma(x, 2^32, 1.5 * 2^52) minus the magic number's.  (x * 2^32 is
    exact in float64, so the fma's single rounding is the rounding of the sum.)"""
    d = np.asarray(x, dtype=np.float32).astype(np.float64) * FX_SCALE + MAGIC
    return d.view(np.int64) - np.int64(MAGIC_BITS)


def in_window(x: np.ndarray) -> np.ndarray:
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)) <= np.uint32(WINDOW_BITS)


def read_back(sums: np.ndarray, pos: np.ndarray, neg: np.ndarray) -> np.ndarray:
    """fl32(fp64(sum) * 2^-32); one flag: +-1e30, both: NaN."""
    v = (sums.astype(np.float64) * (1.0 / FX_SCALE)).astype(np.float32)
    return np.where(pos & neg, F32(np.nan), np.where(pos, SATURATED, np.where(neg, -SATURATED, v))).astype(np.float32)


# ---- the venue-group rule of the direct form -----------------------------------------------------------------------------
def venue_groups(tables: Sequence[tuple], direct_table_floats: int = 0) -> List[tuple]:
    """``tables``: (V, stride) of the direct sets in launch order (run form: V = the widest slice window).  Returns
    (region, group_venues) per set.  Region 0 holds ``cap0`` floats - the largest table, at most the budget - and region
    1 the rest of the budget; ``direct_table_floats`` > 0 caps both.  A set goes to region 1 if its predecessor sits in
    region 0 and its whole table fits region 1, else to region 0; a table larger than its region is staged in groups of
    cap // stride venues."""
    if not tables:
        return []
    largest = max(V * stride for V, stride in tables)
    cap0 = min(largest, BUDGET)
    if 0 < direct_table_floats < cap0:
        cap0 = direct_table_floats
    cap0 = max(cap0, MIN_CAP0)
    cap1 = BUDGET - cap0
    if 0 < direct_table_floats < cap1:
        cap1 = direct_table_floats
    out, prev = [], -1
    for V, stride in tables:
        sz = V * stride
        region = 1 if (prev == 0 and sz <= cap1) else 0
        cap = cap1 if region else cap0
        gv = V if sz <= cap else cap // stride
        if gv < 1:
            raise ValueError("a venue group of no venue: the launch refuses this plan")
        out.append((region, gv))
        prev = region
    return out


# ---- what a plan decides ---------------------------------------------------------------------------------------------------
def forms_of_plan(host) -> dict:
    """{set name: dict(form, ell_k, run_window)} from the host plan's own fields."""
    out = {}
    for s in host.sets:
        t = s.tiled
        if t.runs is not None:
            out[s.name] = dict(form="run", ell_k=0, run_window=int(t.runs.max_window))
        elif t.ell_k:
            out[s.name] = dict(form="direct", ell_k=int(t.ell_k), run_window=0)
        else:
            out[s.name] = dict(form="workspace", ell_k=0, run_window=0)
    return out


def make_group(agent, venue, cum, nets, raw: bool, form: str = "workspace", ell_k: int = 0, run_window: int = 0,
               name: str = "") -> dict:
    """One network group of the step.  ``cum``: float32 [V, stride] as given; ``nets``: the set's ACTIVE networks in
    order - network k reads column k of cum - each (table [2, 2, 100] or None, age75)."""
    cum = np.asarray(cum, dtype=np.float32)
    return dict(name=name, agent=np.asarray(agent, dtype=np.int64).ravel(), venue=np.asarray(venue, dtype=np.int64).ravel(),
                cum=cum.reshape(len(cum), -1), nets=list(nets), raw=bool(raw), form=form, ell_k=int(ell_k),
                run_window=int(run_window))


def groups_of(edge_sets: dict, specs: Sequence, active: Sequence[str], cums: dict, forms: Optional[dict] = None) -> List[dict]:
    """The step's network groups in launch order.  ``specs``: every configured network (``plan.NetworkSpec``: name,
    edge_set, mask_kind, table); ``active``: the step's network names in accumulation order (the networks of one set
    adjacent); ``cums``: {set name: float32 [V, stride]}; ``forms``: ``forms_of_plan`` (None: every set in the workspace
    form)."""
    from grad_june_amd import _native as N

    by_name = {s.name: s for s in specs}
    order = []
    for n in active:
        if by_name[n].edge_set not in order:
            order.append(by_name[n].edge_set)
    groups = []
    for es in order:
        nets = [by_name[n] for n in active if by_name[n].edge_set == es]
        d = edge_sets[es]
        form = dict((forms or {}).get(es) or dict(form="workspace", ell_k=0, run_window=0))
        groups.append(make_group(np.asarray(d["agent"]), np.asarray(d["venue"]), cums[es],
                                 [(None if s.table is None else np.asarray(s.table, dtype=np.float32).reshape(2, 2, 100),
                                   s.mask_kind == N.MASK_QL_AGE75) for s in nets],
                                 raw=nets[0].mask_kind == N.MASK_RAW, name=es, **form))
    return groups


def ell_columns(agent: np.ndarray, n_agents: int) -> np.ndarray:
    """The rank of every edge among its agent's edges, in COO order."""
    order = np.argsort(agent, kind="stable")
    deg = np.bincount(agent, minlength=n_agents)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    col = np.empty(len(agent), dtype=np.int64)
    col[order] = np.arange(len(agent)) - start[agent[order]]
    return col


def primary_edges(agent: np.ndarray, venue: np.ndarray, n_agents: int) -> np.ndarray:
    """bool [E]: the first edge in COO order to the agent's smallest venue (the run form's primary edge)."""
    vmin = np.full(n_agents, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(vmin, agent, venue)
    cand = np.flatnonzero(venue == vmin[agent])
    first = np.full(n_agents, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, agent[cand], cand)
    prim = np.zeros(len(agent), dtype=bool)
    prim[first[first != np.iinfo(np.int64).max]] = True
    return prim


# ---- the restatement -------------------------------------------------------------------------------------------------------
def receiving_weights(g: dict, age, sex, day_type: int, transpose: int) -> Optional[List[np.ndarray]]:
    """Per agent, the pass-2 class weight of each active network of a leisure group (None: a plain set).  class_weights
    of csrc/gj_tiled.h: l = the table entry, lw = fl(l * [age > 75]) for a care-visit kind, else l; pass 2 takes lw
    forward and l transposed."""
    if not any(tab is not None for tab, _ in g["nets"]):
        if len(g["nets"]) != 1:
            raise ValueError("a plain set carries one network")
        return None
    out = []
    for tab, age75 in g["nets"]:
        l = np.asarray(tab, dtype=np.float32)[day_type, sex, age]
        with np.errstate(all="ignore"):
            lw = (l * (age > 75).astype(np.float32)).astype(np.float32) if age75 else l
        out.append(l if transpose else lw)
    return out


def entry_values(g: dict, w2, a: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Phase C's (and the direct form's) float32 value of the entries (agent a, venue v)."""
    cum = g["cum"]
    if w2 is None:
        return cum[v, 0]
    x = np.zeros(len(a), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(len(g["nets"])):
            x = (x + (w2[k][a] * cum[v, k]).astype(np.float32)).astype(np.float32)
    return x


def restate(n_agents: int, groups: Sequence[dict], *, age, sex, day_type: int, transpose: int, susceptibility,
            stage=None, q_thr: float = math.inf, has_quarantine: bool = False, direct_table_floats: int = 0):
    """(agent_sums, trans_susc) as uint32 bit patterns [n_agents]."""
    A = n_agents
    age, sex = np.asarray(age, dtype=np.int64), np.asarray(sex, dtype=np.int64)
    quar = np.zeros(A, dtype=bool)
    if has_quarantine:
        quar = ~(np.asarray(stage, dtype=np.float32) < F32(q_thr))
    groups = [g for g in groups if len(g["agent"]) > 0 and len(g["nets"]) > 0]
    w2 = [receiving_weights(g, age, sex, day_type, transpose) for g in groups]
    prim = [primary_edges(g["agent"], g["venue"], A) if g["form"] == "run" else None for g in groups]

    # workspace form: fixed point, masked sets, quarantine, raw sets
    sums = np.zeros(A, dtype=np.int64)
    pos, neg = np.zeros(A, dtype=bool), np.zeros(A, dtype=bool)
    for raw in (False, True):
        for g, w, pr in zip(groups, w2, prim):
            if g["form"] == "direct" or g["raw"] != raw:
                continue
            a, v = (g["agent"], g["venue"]) if pr is None else (g["agent"][~pr], g["venue"][~pr])
            x = entry_values(g, w, a, v)
            ok = in_window(x)
            np.add.at(sums, a[ok], to_fx(x[ok]))
            with np.errstate(invalid="ignore"):
                pos[a[~ok & ~(x < 0)]] = True
                neg[a[~ok & ~(x > 0)]] = True
        if not raw and has_quarantine:
            sums[quar] = 0
            one = quar & (pos != neg)
            pos[one] = False
            neg[one] = False
    acc = read_back(sums, pos, neg)

    # direct and run forms: float32, item by item
    direct = [(g, w, pr) for g, w, pr in zip(groups, w2, prim) if g["form"] in ("direct", "run")]
    tables = [(g["run_window"] if g["form"] == "run" else g["cum"].shape[0], g["cum"].shape[1]) for g, _, _ in direct]
    everyone = np.arange(A)
    zero = np.zeros(A, dtype=np.float32)
    for (g, w, pr), (_, gv) in zip(direct, venue_groups(tables, direct_table_floats)):
        taken = ~quar if not g["raw"] else np.ones(A, dtype=bool)
        if g["form"] == "run":
            ell = np.full((A, 2), -1, dtype=np.int64)
            ell[g["agent"][pr], 0] = g["venue"][pr]
            starts = [None]                          # one item: the slice's window holds every primary venue
        else:
            K = g["ell_k"]
            col = ell_columns(g["agent"], A)
            if col.max() >= K:
                raise ValueError("an agent with more edges than ELL columns")
            ell = np.full((A, K), -1, dtype=np.int64)
            ell[g["agent"], col] = g["venue"]
            starts = range(0, g["cum"].shape[0], gv)
        for v0 in starts:
            for plane in range(ell.shape[1] // 2):
                sj = zero
                for c in (2 * plane, 2 * plane + 1):
                    lv = ell[:, c]
                    ok = (lv >= 0) & taken
                    if v0 is not None:
                        ok &= (lv >= v0) & (lv < v0 + gv)
                    x = entry_values(g, w, everyone, np.where(ok, lv, 0))
                    with np.errstate(all="ignore"):
                        sj = (sj + np.where(ok, x, F32(0.0))).astype(np.float32)
                with np.errstate(all="ignore"):
                    acc = (acc + sj).astype(np.float32)
    with np.errstate(all="ignore"):
        ts = (np.asarray(susceptibility, dtype=np.float32) * acc).astype(np.float32)
    return np.ascontiguousarray(acc).view(np.uint32), np.ascontiguousarray(ts).view(np.uint32)


# ---- float64 sums and the bound of the restatement against them (tests of the restatement itself) -----------------------
def fp64_sums(n_agents: int, groups: Sequence[dict], *, age, sex, day_type: int, transpose: int, stage=None,
              q_thr: float = math.inf, has_quarantine: bool = False):
    """Every agent's sum in float64 from the edge lists (finite cum inside the window), and the bound on
    |restatement - this| from the number formats alone.  With u = 2^-24, T the agent's entries, S_abs the sum of
    |w2 * cum| over them and nk the most networks on one of its sets:

        an entry of a leisure set: nk products (u |term| each) and nk - 1 roundings of partial sums   <= nk u S_abs
        workspace form: rint per entry (2^-33 each), exact integer adds, one rounding of the sum       <= T 2^-33 + u |sum|
        direct / run form: an entry into its item's pair, the pair into acc - two roundings of a
        partial sum per entry                                                                            <= 2 T u S_abs

    E = (1 + 2^-20) * ((nk + 2 T + 1) u S_abs + T 2^-33 + u |out|).  (``cum`` is given: no carried error.)"""
    A = n_agents
    age, sex = np.asarray(age, dtype=np.int64), np.asarray(sex, dtype=np.int64)
    quar = np.zeros(A, dtype=bool)
    if has_quarantine:
        quar = ~(np.asarray(stage, dtype=np.float32) < F32(q_thr))
    out, s_abs, terms, nk_max = np.zeros(A), np.zeros(A), np.zeros(A), np.ones(A)
    for g in groups:
        if not len(g["agent"]) or not g["nets"]:
            continue
        a, v = g["agent"], g["venue"]
        w = receiving_weights(g, age, sex, day_type, transpose)
        q = np.ones(A) if g["raw"] else (~quar).astype(np.float64)
        for k in range(len(g["nets"])):
            wk = np.ones(A) if w is None else w[k].astype(np.float64)
            t = q[a] * wk[a] * g["cum"][v, k].astype(np.float64)
            out += np.bincount(a, weights=t, minlength=A)
            s_abs += np.bincount(a, weights=np.abs(t), minlength=A)
        terms += np.bincount(a, minlength=A)
        has = np.bincount(a, minlength=A) > 0
        nk_max = np.where(has, np.maximum(nk_max, len(g["nets"])), nk_max)
    bound = SLACK * ((nk_max + 2 * terms + 1) * U32 * s_abs + terms * FX_AGENT_HALF + U32 * np.abs(out))
    return out, bound
