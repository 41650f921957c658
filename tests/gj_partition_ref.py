"""One rank's part of a partitioned world (grad_june_amd.distributed: classify_venues, RankPartitioner, order_halo) restated
from their docstrings in plain Python: loops, dicts and ``sorted()`` over edge lists, Python integers throughout.  Nothing
of the partitioner is imported but its constants and ``partition_bounds``.

A world is cut into the agent ranges [b[r], b[r+1]).  An edge set arrives as one *part* or - a split set - as two
(``split_set``), each with the exchange mode it runs in; which mode a set gets is not restated here (it has tests of its
own), the venue classes the decision starts from are (``venue_classes``).  For rank r:

* its OWNED edges of a part are those whose agent lies in [b[r], b[r+1]), in COO order;
* a ``partial`` or ``local`` part keeps the owned edges: venue ids unchanged, ``people`` whole, ``venue_global`` the
  part's venue ids in the whole set (``None`` when the part is the whole set);
* a ``halo`` part keeps EVERY edge of every venue an owned edge touches, in COO order; those venues are numbered in
  ascending order, ``people`` and ``venue_global`` follow that numbering, and every remote attendee is listed once with
  its smallest local venue;
* the halo agents are the union of those lists over the halo parts in the order the parts were added; an agent carries
  the first part that lists it and its venue there, and they are ordered by (owner, part, venue, id);
* ``n_local_pad`` is ``n_local`` rounded up to ``slice_agents`` when there is a halo, else ``n_local``;
  ``n_ext = n_local_pad + n_halo`` and ``n_slices = max(1, ceil(n_ext / slice_agents))``;
* the extended index of an owned agent g is ``g - b[r]``, of a halo agent ``n_local_pad`` + its position in the halo list;
* ``age`` and ``sex`` cover the extended range, the padding rows hold agent 0's values;
* ``halo_from[o]`` counts the halo agents owned by rank o.
"""
from __future__ import annotations

from bisect import bisect_right
from typing import Dict, List, Optional, Sequence

from grad_june_amd.distributed import HALO_MAX_MEAN_DEGREE, PARTIAL_COST_FACTOR, SPLIT_SUFFIX, partition_bounds


def _ints(a) -> List[int]:
    return [int(x) for x in (a.tolist() if hasattr(a, "tolist") else a)]


def venue_classes(agent, venue, n_venues: int, bounds, nets_on_set: int = 1) -> List[bool]:
    """Per venue: does it go the partial-sum way?  With n attendees living on T of the R ranks: when n is above
    HALO_MAX_MEAN_DEGREE and the halo form's n (T - 1) floats exceed the all-reduce's 2 k (R - 1)."""
    b = _ints(bounds)
    R = len(b) - 1
    n = [0] * n_venues
    owners = [set() for _ in range(n_venues)]
    for g, v in zip(_ints(agent), _ints(venue)):
        n[v] += 1
        owners[v].add(bisect_right(b, g) - 1)
    return [n[v] > HALO_MAX_MEAN_DEGREE and n[v] * (len(owners[v]) - 1) > PARTIAL_COST_FACTOR * 2.0 * max(1, nets_on_set) * (R - 1)
            for v in range(n_venues)]


def part(name: str, agent, venue, people, mode: str, venue_ids: Optional[Sequence[int]] = None) -> dict:
    return {"name": name, "agent": _ints(agent), "venue": _ints(venue), "people": _ints(people), "mode": mode,
            "venue_ids": None if venue_ids is None else _ints(venue_ids)}


def split_set(name: str, agent, venue, people, big: Sequence[bool]) -> List[dict]:
    """The two parts of a split set: ``name`` with the venues that are not ``big`` (halo), ``name~big`` with the others
    (partial sums), each with its venues renumbered in ascending order and its edges in COO order."""
    agent, venue, people = _ints(agent), _ints(venue), _ints(people)
    out = []
    for part_name, want, mode in ((name, False, "halo"), (name + SPLIT_SUFFIX, True, "partial")):
        ids = [v for v in range(len(people)) if bool(big[v]) == want]
        new_id = {v: i for i, v in enumerate(ids)}
        edges = [(g, new_id[v]) for g, v in zip(agent, venue) if v in new_id]
        out.append(part(part_name, [g for g, _ in edges], [v for _, v in edges], [people[v] for v in ids], mode, ids))
    return out


def rank_world(n_agents: int, age, sex, parts: Sequence[dict], rank: int, world_size: int, slice_agents: int) -> Dict:
    """The part of ``rank``: a dict with the fields of ``distributed.RankWorld`` as Python lists / ints / dicts."""
    b = _ints(partition_bounds(n_agents, world_size))
    a0, a1 = b[rank], b[rank + 1]
    owner = lambda g: bisect_right(b, g) - 1
    edge_sets, venue_global, modes, halo_lists = {}, {}, {}, []
    for p in parts:
        modes[p["name"]] = p["mode"]
        edges = list(zip(p["agent"], p["venue"]))
        owned = [(g, v) for g, v in edges if a0 <= g < a1]
        if p["mode"] in ("partial", "local"):
            edge_sets[p["name"]] = {"agent_global": [g for g, _ in owned], "venue": [v for _, v in owned],
                                    "people": list(p["people"])}
            venue_global[p["name"]] = p["venue_ids"]
            continue
        touched = sorted({v for _, v in owned})
        local = {v: i for i, v in enumerate(touched)}
        kept = [(g, local[v]) for g, v in edges if v in local]
        edge_sets[p["name"]] = {"agent_global": [g for g, _ in kept], "venue": [v for _, v in kept],
                                "people": [p["people"][v] for v in touched]}
        venue_global[p["name"]] = touched if p["venue_ids"] is None else [p["venue_ids"][v] for v in touched]
        smallest = {}
        for g, v in kept:
            if not a0 <= g < a1:
                smallest[g] = min(v, smallest.get(g, v))
        halo_lists.append(smallest)
    first = {}
    for i, smallest in enumerate(halo_lists):
        for g, v in smallest.items():
            if g not in first:
                first[g] = (i, v)
    halo = sorted(first, key=lambda g: (owner(g), first[g][0], first[g][1], g))
    n_local = a1 - a0
    n_local_pad = -(-n_local // slice_agents) * slice_agents if halo else n_local
    n_ext = n_local_pad + len(halo)
    position = {g: i for i, g in enumerate(halo)}
    for es in edge_sets.values():
        es["agent"] = [g - a0 if a0 <= g < a1 else n_local_pad + position[g] for g in es.pop("agent_global")]

    def extended(values):
        values = list(values.tolist() if hasattr(values, "tolist") else values)
        out = [values[0]] * n_ext
        out[:n_local] = values[a0:a1]
        out[n_local_pad:] = [values[g] for g in halo]
        return out

    halo_from = [0] * world_size
    for g in halo:
        halo_from[owner(g)] += 1
    return {"rank": rank, "world_size": world_size, "bounds": b, "n_local": n_local, "slice_agents": slice_agents,
            "n_local_pad": n_local_pad, "n_ext": n_ext, "n_slices": max(1, -(-n_ext // slice_agents)), "halo_global": halo,
            "halo_from": halo_from, "age": extended(age), "sex": extended(sex), "edge_sets": edge_sets, "modes": modes,
            "venue_global": venue_global}
