"""numpy restatement of gj_immunity_step / gj_adjoint_immunity (include/gradjune_hip.h), test infrastructure only.

After a step, a recovered agent that is not newly infected relaxes towards ``cap[age]``: ``s' = cap - (cap - s) * keep`` in
three float32 operations; a newly infected agent that had an infection before gets the step's increment of ``is_infected``
undone.  The tables are fp32 values the host rounds once and the kernel only subtracts and multiplies, so the float32
restatement is exact.  ``step64`` is the same rule in float64 (what the closed form is compared with); the adjoint's
per-band sums are restated in float64, both as plain sums and in the order the seed plan's two kernels add them."""
import numpy as np

N_AGES = 100
WANED, REINFECTED = 1, 2
UNIT = float(1 << 30)
CHUNK, WAVE = 1024, 64


def tables(band_of_age, half_life, residual, dt: float):
    """(cap, keep), float32 [100] each: keep = fp32(2 ** (-dt / h)) in Python doubles and cap = fp32(1 - fp64(fp32(r))),
    both 1 for an age in no band (band < 0).  ``half_life`` / ``residual``: one value per band."""
    h = [float(np.float32(v)) for v in half_life]
    r = [float(np.float32(v)) for v in residual]
    cap, keep = np.ones(N_AGES, dtype=np.float32), np.ones(N_AGES, dtype=np.float32)
    for age, b in enumerate(band_of_age):
        if b >= 0:
            keep[age] = np.float32(2.0 ** (-float(dt) / h[b]))
            cap[age] = np.float32(1.0 - r[b])
    return cap, keep


def step(tabs, age, stage, recovered, new_infected, susceptibility, is_infected, dtype=np.float32):
    """{"susceptibility", "is_infected" (updated, ``dtype``), "flags" uint8, "reinfected" float32 0 / 1, "count",
    "susc_sum" (the launch's int64 term)}.  ``new_infected`` None: nobody."""
    cap_t, keep_t = tabs
    age = np.asarray(age, dtype=np.int64) % N_AGES
    n = len(age)
    s, inf = np.asarray(susceptibility, dtype=dtype), np.asarray(is_infected, dtype=dtype)
    nw = np.zeros(n, dtype=dtype) if new_infected is None else np.asarray(new_infected, dtype=dtype)
    nu = nw != 0
    cap, keep = cap_t[age].astype(dtype), keep_t[age].astype(dtype)
    waned = (np.asarray(stage, dtype=np.float32) == np.float32(recovered)) & ~nu & (keep_t[age] != 1)
    with np.errstate(invalid="ignore"):
        gap = (cap - s).astype(dtype)
        relaxed = (cap - (gap * keep).astype(dtype)).astype(dtype)
        before = (inf - nw).astype(dtype)
        reinfected = nu & (before >= 1)
    s1 = np.where(waned, relaxed, s).astype(dtype)
    inf1 = np.where(reinfected, before, inf).astype(dtype)
    with np.errstate(invalid="ignore"):
        clamped = np.fmin(np.fmax(s1.astype(np.float32), np.float32(0)), np.float32(4))      # (fmax: a NaN counts 0)
    fixed = (clamped.astype(np.float32) * np.float32(UNIT)).astype(np.int64)
    return {"susceptibility": s1, "is_infected": inf1,
            "flags": (waned * WANED + reinfected * REINFECTED).astype(np.uint8),
            "reinfected": reinfected.astype(np.float32), "count": int(reinfected.sum()), "susc_sum": int(fixed.sum())}


def step64(tabs, age, stage, recovered, new_infected, susceptibility, is_infected):
    return step(tabs, age, stage, recovered, new_infected, susceptibility, is_infected, dtype=np.float64)


def closed_form(cap, t, half_life):
    """cap * (1 - 2^(-t / h)) in float64: the susceptibility ``t`` days after a recovery at 0."""
    return float(cap) * (1.0 - 2.0 ** (-float(t) / float(half_life)))


def wave_sum(v):
    """The butterfly of wave_sum over 64 lanes (xor 32, 16, .. 1), float64; lane 0's total."""
    v = np.asarray(v, dtype=np.float64).copy()
    off = WAVE // 2
    while off:
        v = v + v[np.arange(WAVE) ^ off]
        off //= 2
    return v[0]


def plan_sum(terms, band, n_bands):
    """float64 [B]: per band the sum of ``terms`` in the order gj_seed_plan fixes - the band's agents in index order
    (stable sort), cut into chunks of 1024; a chunk: every lane its terms j = lane, lane + 64, .. in order, then the
    butterfly; the band: every lane its chunks' partials c = lane, lane + 64, .., then the butterfly."""
    terms, band = np.asarray(terms, dtype=np.float64), np.asarray(band, dtype=np.int64)
    out = np.zeros(n_bands, dtype=np.float64)
    for b in range(n_bands):
        mine = terms[band == b]
        partials = []
        for c0 in range(0, len(mine), CHUNK):
            chunk = mine[c0:c0 + CHUNK]
            lanes = np.zeros(WAVE, dtype=np.float64)
            for j0 in range(0, len(chunk), WAVE):      # lane l adds chunk[j0 + l] in order of j0
                row = chunk[j0:j0 + WAVE]
                lanes[:len(row)] = lanes[:len(row)] + row
            partials.append(wave_sum(lanes))
        lanes = np.zeros(WAVE, dtype=np.float64)
        for j0 in range(0, len(partials), WAVE):
            row = np.asarray(partials[j0:j0 + WAVE])
            lanes[:len(row)] = lanes[:len(row)] + row
        out[b] = wave_sum(lanes)
    return out


def adjoint(tabs, flags, age, susceptibility0, g_susc, g_inf, band, n_bands):
    """{"g_susc_in", "g_inf_in", "g_new" float32 [n]; "term_A", "term_B" float64 [n]; "sum_A", "sum_B" float64 [B] in the
    plan's order}.  ``g_susc`` / ``g_inf`` None = zeros; a band outside [0, n_bands) is no band."""
    cap_t, keep_t = tabs
    age = np.asarray(age, dtype=np.int64) % N_AGES
    n = len(age)
    flags = np.asarray(flags, dtype=np.uint8)
    waned, reinfected = (flags & WANED) != 0, (flags & REINFECTED) != 0
    gs = np.zeros(n, dtype=np.float32) if g_susc is None else np.asarray(g_susc, dtype=np.float32)
    gi = np.zeros(n, dtype=np.float32) if g_inf is None else np.asarray(g_inf, dtype=np.float32)
    s0 = np.asarray(susceptibility0, dtype=np.float32)
    band = np.asarray(band, dtype=np.int64)
    term = waned & (band >= 0) & (band < n_bands)
    with np.errstate(invalid="ignore"):
        g_susc_in = np.where(waned, (gs * keep_t[age]).astype(np.float32), gs).astype(np.float32)
        gap = (cap_t[age] - s0).astype(np.float32)
        term_a = np.where(term, gs.astype(np.float64) * gap.astype(np.float64), 0.0)
    term_b = np.where(term, gs.astype(np.float64), 0.0)
    g_new = np.where(reinfected, -gi, np.float32(0)).astype(np.float32)
    where = np.where((band >= 0) & (band < n_bands), band, -1)      # (a band's agents without a term add 0 in their place)
    return {"g_susc_in": g_susc_in, "g_inf_in": gi.copy(), "g_new": g_new, "term_A": term_a, "term_B": term_b,
            "sum_A": plan_sum(term_a, where, n_bands), "sum_B": plan_sum(term_b, where, n_bands)}
