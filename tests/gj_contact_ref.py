"""numpy restatement of the contact-quarantine kernels (csrc/gj_contact.h: gj_contact_mark, gj_contact_mask), test
infrastructure only.  Integers and compares: ``until`` holds fp32 bit patterns of non-negative times as uint32, whose
unsigned order is the float order, so the mark is an integer maximum; the mask compares.  Nothing here calls the library.

A set is a dict ``{"rowptr": int32 [n + 1], "venue": int32 [edges], "until": uint32 [n_venues]}`` - the set's edges as
CSR by agent - plus ``"days"`` where a release time is formed."""
import numpy as np

import gj_philox_ref as P

QUARANTINE_STREAM = 1 << 59
ERR_ROWS = 4


def stream_of(policy: int) -> int:
    return QUARANTINE_STREAM | policy


def uniforms(seed: int, stream: int, agent_offset: int, n: int) -> np.ndarray:
    """The compliance uniform of the local agents 0 .. n: infection_uniform at the GLOBAL id."""
    return P.infection_uniform(seed, stream, agent_offset + np.arange(n, dtype=np.uint64)) if n else np.zeros(0, np.float32)


def release_bits(now: float, days: float) -> np.uint32:
    """bits(fp32(fp64(now) + days)): formed once, as the host forms it."""
    return np.float32(np.float64(now) + np.float64(days)).view(np.uint32)


def index_cases(stage, threshold) -> np.ndarray:
    """!(stage < threshold): a NaN stage is an index case."""
    return ~(np.asarray(stage, dtype=np.float32) < np.float32(threshold))


def csr_by_agent(agent, venue, n: int):
    """COO -> (rowptr int32 [n + 1], venue int32): a stable sort by agent keeps the COO order inside a row."""
    agent, venue = np.asarray(agent, dtype=np.int64), np.asarray(venue, dtype=np.int64)
    order = np.argsort(agent, kind="stable")
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(agent, minlength=n)))).astype(np.int32)
    return rowptr, venue[order].astype(np.int32)


def _walk(s, n: int, agents: np.ndarray):
    """(agent of every edge walked, its venue id, error word): the rows of ``agents`` in set ``s``; a row that is
    negative, decreasing or beyond rowptr[n], and a venue id outside the set, is skipped and reported."""
    rowptr, venue = s["rowptr"].astype(np.int64), s["venue"].astype(np.int64)
    r0, r1 = rowptr[agents], rowptr[agents + 1]
    ok = (r0 >= 0) & (r1 >= r0) & (r1 <= rowptr[n])
    err = ERR_ROWS if (~ok).any() else 0
    agents, r0, r1 = agents[ok], r0[ok], r1[ok]
    length = r1 - r0
    owner = np.repeat(agents, length)
    edge = np.repeat(r0 - np.concatenate(([0], np.cumsum(length)[:-1])), length) + np.arange(length.sum())
    v = venue[edge.astype(np.int64)]
    inside = (v >= 0) & (v < len(s["until"]))
    if (~inside).any():
        err |= ERR_ROWS
    return owner[inside], v[inside], err


def mark(stage, threshold, sets, now: float):
    """([until after the launch, one per set], error word); the inputs stay as they are."""
    n = len(stage)
    idx = np.nonzero(index_cases(stage, threshold))[0]
    out, err = [], 0
    for s in sets:
        until = s["until"].astype(np.uint32).copy()
        _, v, e = _walk(s, n, idx)
        err |= e
        np.maximum.at(until, v, release_bits(now, s["days"]))
        out.append(until)
    return out, err


def mask(stage, q_threshold, sets, now: float, compliance: float, u):
    """(qstate float32 [n]: 0 free, 1 index case, 2 contact; error word).  ``u``: ``uniforms`` of the agents.  Only a
    complying agent that is no index case walks its rows (and can report a bad one)."""
    n = len(stage)
    idx = index_cases(stage, q_threshold)
    walkers = np.nonzero(~idx & (np.asarray(u, dtype=np.float32) < np.float32(compliance)))[0]
    held, err = np.zeros(n, dtype=bool), 0
    for s in sets:
        owner, v, e = _walk(s, n, walkers)
        err |= e
        marked = s["until"].astype(np.uint32)[v].view(np.float32) > np.float32(now)
        held[owner[marked]] = True
    return np.where(idx, 1.0, np.where(held, 2.0, 0.0)).astype(np.float32), err
