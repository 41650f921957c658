"""numpy restatement of the testing kernels (csrc/gj_testing.h: gj_testing_step, gj_adjoint_testing), test infrastructure
only - and the specification of the rule.  Compares, one fp32 add and one fp32 divide: the restatement gives the kernels'
bits.  Nothing here calls the library.

State: a dict ``{"decided": uint32 [n], "result_time", "positive", "isolate_until", "confirmed_time": float32 [n]}``.
Per agent and launch, in this order (g = agent_offset + a, age = agent_class % 100):

  decide   if active and !(stage < stage_threshold) and bits(infection_time) != decided:
             decided = bits(infection_time)
             r = Philox4x32-10(counter = (g, decide_stream | bits(infection_time)), key = seed)   - the agent's own block
             positive = u01(r[0]) < probability[age]
             k = the first delay entry with cum[k] > u01(r[1]), the last where there is none
             result_time = fp32(now) + days[k]                                                     - one fp32 add
  report   if result_time <= now:  result_time = +inf;  where positive: newly confirmed, confirmed_time = now, and - for
             a policy that isolates, where infection_uniform(seed, comply_stream, g) < compliance - isolate_until = release
  mask     (a policy that isolates)  qstate = 1 if !(stage < q_threshold), else 3 if now < isolate_until, else 0
"""
import numpy as np

import gj_philox_ref as P

TESTING_STREAM = 1 << 58
COMPLY_STREAM = TESTING_STREAM | 1 << 57
DECIDED, POSITIVE, DUE = 1, 2, 4
MAX_DELAYS = 16


def decide_stream(policy: int) -> int:
    return TESTING_STREAM | policy << 32


def comply_stream(policy: int) -> int:
    return COMPLY_STREAM | policy


def initial_state(n: int, isolates: bool = True):
    return {"decided": np.full(n, 0xFFFFFFFF, np.uint32), "result_time": np.full(n, np.inf, np.float32),
            "positive": np.zeros(n, np.float32), "isolate_until": np.zeros(n, np.float32) if isolates else None,
            "confirmed_time": np.full(n, -1.0, np.float32)}


def probability_table(bands: dict) -> np.ndarray:
    """float32 [100]: ``{"lo-hi": p}`` -> p for lo <= age < hi, 0 for an age in no band; each value rounded once."""
    table = np.zeros(100, np.float32)
    for key, p in bands.items():
        lo, hi = (int(x) for x in str(key).split("-"))
        table[lo:min(hi, 100)] = np.float32(p)
    return table


def delay_tables(delay):
    """(cum float32 [k], days float32 [k]): the cumulative shares as running fp64 sums in file order, each rounded once."""
    entries = list(delay.items()) if isinstance(delay, dict) else [(delay, 1.0)]
    days = np.array([float(d) for d, _ in entries], np.float32)
    cum = np.array([sum(float(s) for _, s in entries[:k + 1]) for k in range(len(entries))], np.float64).astype(np.float32)
    return cum, days


def decision_words(seed: int, stream: int, g, bits):
    """(u01(r[0]), u01(r[1])) of the decisions' own blocks: counter low = g, high = stream | bits, key = seed."""
    g, bits = np.asarray(g, np.uint64), np.asarray(bits, np.uint64)
    if len(g) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    hi = np.uint64(stream) | bits
    r = P.philox4x32_10(g.astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32), hi.astype(np.uint32),
                        (hi >> np.uint64(32)).astype(np.uint32), seed & 0xFFFFFFFF, seed >> 32)
    return P.u01(r[0]), P.u01(r[1])


def step(state, agent_class, stage, infection_time, *, probability, delay_cum, delay_days, stage_threshold, active, now,
         seed, policy=0, agent_offset=0, q_threshold=np.inf, isolation_days=None, compliance=1.0, ids=None):
    """One launch: ``state`` is updated in place.  Returns ``{"newly": float32 [n], "qstate": float32 [n] or None,
    "flags": uint8 [n], "counts": (newly confirmed, decisions)}``.  ``ids``: the agents' global ids where they are not
    ``agent_offset + a`` (a permuted population)."""
    n = len(stage)
    ids = agent_offset + np.arange(n, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    stage = np.asarray(stage, np.float32)
    it = np.asarray(infection_time, np.float32)
    now32 = np.float32(now)
    age = np.asarray(agent_class).astype(np.int64) % 100
    bits = it.view(np.uint32)
    flags = np.zeros(n, np.uint8)
    deciding = np.zeros(n, bool)
    if active:
        deciding = ~(stage < np.float32(stage_threshold)) & (bits != state["decided"])
    idx = np.nonzero(deciding)[0]
    u0, u1 = decision_words(seed, decide_stream(policy), ids[idx], bits[idx])
    cum, days = np.asarray(delay_cum, np.float32), np.asarray(delay_days, np.float32)
    k = np.full(len(idx), len(days) - 1)
    for j in range(len(days) - 2, -1, -1):      # the FIRST entry whose threshold exceeds u
        k = np.where(cum[j] > u1, j, k)
    state["decided"][idx] = bits[idx]
    state["positive"][idx] = (u0 < np.asarray(probability, np.float32)[age[idx]]).astype(np.float32)
    state["result_time"][idx] = now32 + days[k]
    flags[idx] |= DECIDED
    due = state["result_time"] <= now32
    state["result_time"][due] = np.inf
    flags[due] |= DUE
    flags[(deciding | due) & (state["positive"] != 0)] |= POSITIVE
    newly = due & (state["positive"] != 0)
    state["confirmed_time"][newly] = now32
    qstate = None
    if isolation_days is not None:
        who = np.nonzero(newly)[0]
        u = (P.infection_uniform(seed, comply_stream(policy), ids[who]) if len(who)
             else np.zeros(0, np.float32))
        release = np.float32(np.float64(now) + np.float64(isolation_days))      # formed once, as the host forms it
        state["isolate_until"][who[u < np.float32(compliance)]] = release
        qstate = np.where(~(stage < np.float32(q_threshold)), 1.0,
                          np.where(now32 < state["isolate_until"], 3.0, 0.0)).astype(np.float32)
    return {"newly": newly.astype(np.float32), "qstate": qstate, "flags": flags,
            "counts": (int(newly.sum()), int(deciding.sum()))}


def seed_plan_sum(contrib, band, n_bands: int, chunk: int = 1024, wave: int = 64):
    """float64 [n_bands]: the per-band sums in the kernels' fixed order - the agents of a band in index order, cut into
    chunks of ``chunk``; in a chunk every lane adds its terms (lane, lane + 64, ..) in order and the lanes are added by a
    butterfly; a band's chunk sums are added the same way."""
    def butterfly(lanes):
        lanes = lanes.copy()
        off = wave // 2
        while off:
            lanes = lanes + lanes[np.arange(wave) ^ off]
            off >>= 1
        return lanes[0]

    def wave_sum(values):
        lanes = np.zeros(wave, np.float64)
        for j0 in range(0, len(values), wave):
            part = values[j0:j0 + wave]
            lanes[:len(part)] += part
        return butterfly(lanes)

    out = np.zeros(n_bands, np.float64)
    contrib, band = np.asarray(contrib, np.float64), np.asarray(band)
    for b in range(n_bands):
        terms = contrib[band == b]
        partial = np.array([wave_sum(terms[c:c + chunk]) for c in range(0, len(terms), chunk)], np.float64)
        out[b] = wave_sum(partial)
    return out


def adjoint(flags, stage, g_y, g_row, band, n_bands: int):
    """(grad_probability float64 [n_bands], g_stage float32 [n], g_y_in float32 [n]) of one launch: with g = g_y + (due ?
    g_row : 0), a deciding agent gives g to its band and g * hard / stage to its stage; everybody else hands g on."""
    flags = np.asarray(flags, np.uint8)
    stage = np.asarray(stage, np.float32)
    g = np.asarray(g_y, np.float32) + np.where(flags & DUE, np.float32(g_row), np.float32(0)).astype(np.float32)
    decided = (flags & DECIDED) != 0
    hard = ((flags & POSITIVE) != 0).astype(np.float32)
    band = np.asarray(band)
    in_band = (band >= 0) & (band < n_bands)
    contrib = np.where(decided & in_band, g.astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        g_stage = np.where(decided, g * hard / stage, np.float32(0)).astype(np.float32)
    g_y_in = np.where(decided, np.float32(0), g).astype(np.float32)
    return seed_plan_sum(contrib, np.where(in_band, band, -1), n_bands), g_stage, g_y_in
