"""numpy restatement of gj_vaccinate / gj_adjoint_vaccinate (include/gradjune_hip.h), test infrastructure only.

A campaign gives every agent one uniform for the whole run, ``u = infection_uniform(seed, (1 << 61) | campaign, global
id)`` (gj_philox_ref); a launch moves the agents with ``thr_lo[age] <= u < thr_hi[age]`` and multiplies their
susceptibility by ``factor[age]`` in fp32.  The tables are fp32 values the host rounds once, the kernel only compares
and multiplies, so the restatement is exact.  The adjoint's per-band sums are restated in float64."""
import numpy as np

from gj_philox_ref import infection_uniform

VACCINE_STREAM = 1 << 61
N_AGES = 100


def stream_of(campaign: int) -> int:
    return VACCINE_STREAM | int(campaign)


def uniforms(seed: int, stream: int, agent_offset: int, n: int):
    """u of the local agents 0 .. n-1 (global ids agent_offset + a), float32."""
    return infection_uniform(seed, stream, np.arange(n, dtype=np.uint64) + np.uint64(agent_offset))


def ramp(date, start, end) -> float:
    """clamp((date - start) / (end - start), 0, 1) in Python doubles; 1 from ``end`` on (also when start == end)."""
    if date >= end:
        return 1.0
    if date <= start:
        return 0.0
    return (date - start).total_seconds() / (end - start).total_seconds()


def tables(coverage, band_of_age, efficacy, lo: float, hi: float):
    """(thr_lo, thr_hi, factor), float32 [100] each: fp32(fp64(coverage[age]) * ramp) and fp32(1 - fp64(efficacy of the
    age's band)), 1 for an age in no band (band < 0).  ``efficacy``: the float32 values, one per band."""
    cov = np.asarray(coverage, dtype=np.float64)
    band = np.asarray(band_of_age, dtype=np.int64)
    eff = np.asarray(efficacy, dtype=np.float32).astype(np.float64)
    factor = np.where(band >= 0, 1.0 - eff[np.maximum(band, 0)], 1.0)
    return (cov * float(lo)).astype(np.float32), (cov * float(hi)).astype(np.float32), factor.astype(np.float32)


def newly(u, age, thr_lo, thr_hi):
    age = np.asarray(age, dtype=np.int64) % N_AGES
    return (thr_lo[age] <= u) & (u < thr_hi[age])


def vaccinate(susceptibility, age, tabs, u):
    """(updated susceptibility float32, newly bool): the fp32 multiply where newly, the value as it is elsewhere."""
    thr_lo, thr_hi, factor = tabs
    age = np.asarray(age, dtype=np.int64) % N_AGES
    nw = newly(u, age, thr_lo, thr_hi)
    s = np.asarray(susceptibility, dtype=np.float32)
    return np.where(nw, s * factor[age], s).astype(np.float32), nw


def adjoint(susceptibility0, g_out, age, band, n_bands, tabs, u):
    """{"g_in": float32 [n], "grad_efficacy": float64 [B], "abs_sum": float64 [B] (sum |c_a| per band), "newly"}.
    ``g_out`` None = zeros; a band outside [0, n_bands) is no band."""
    thr_lo, thr_hi, factor = tabs
    age = np.asarray(age, dtype=np.int64) % N_AGES
    n = len(age)
    nw = newly(u, age, thr_lo, thr_hi)
    g = np.zeros(n, dtype=np.float32) if g_out is None else np.asarray(g_out, dtype=np.float32)
    g_in = (g * np.where(nw, factor[age], np.float32(1.0)).astype(np.float32)).astype(np.float32)
    band = np.asarray(band, dtype=np.int64)
    valid = nw & (band >= 0) & (band < n_bands)
    c = np.where(valid, -(g.astype(np.float64) * np.asarray(susceptibility0, dtype=np.float32).astype(np.float64)), 0.0)
    idx = np.where(valid, band, 0)
    grad = np.bincount(idx, weights=c, minlength=n_bands)[:n_bands]
    abs_sum = np.bincount(idx, weights=np.abs(c), minlength=n_bands)[:n_bands]
    return {"g_in": g_in, "grad_efficacy": grad, "abs_sum": abs_sum, "newly": nw}
