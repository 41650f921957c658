"""numpy restatement of the seed by agent group and of its adjoint (include/gradjune_hip.h, gj_adjoint_seed), test
infrastructure only.  float64 by default; ``dtype=np.float32`` runs the same formulas in the kernel's precision (what
the tolerance of a comparison with the reference is measured with).

Forward: agent a is infected with probability fraction[labels[a]]; p = 1 - that.  With injected Exponential(1) draws
(e0, e1) the decision is the argmax of the tau = 0.1 Gumbel-softmax (ties: not infected), with the library's own noise
it is p < theta (tests/gj_philox_ref.py).  Then infect_people: susceptibility = max(0, s - nu), is_infected += nu,
infection_time += nu * (now - infection_time).

Adjoint: c_a = -nu_bar * d nu / d p with nu_bar = g_inf + g_time * (now - time0) - g_susc * h + g_new, h the subgradient
of max(0, s0 - nu) (0.5 at the tie) and d nu / d p = -(y0 * y1 / 0.1) * (1/p + 1/(1-p)) (0 where not finite);
d loss / d fraction[g] = sum of c_a over the group."""
import numpy as np

import gj_philox_ref as P

TAU = 0.1


def library_draws(seed: int, step: int, agent_offset: int, n: int):
    """(e0, e1, theta) of local agents 0 .. n-1: the forward's uniform theta (float32) and the backward's pair of draws as
    gj_adjoint_seed forms it - theta and s = -log(u1) - log(u2) in float32 (exp_pair of gj_philox_ref.py), the products
    theta * s and (1 - theta) * s in float64, where they are exact."""
    ids = np.arange(n, dtype=np.uint64) + np.uint64(agent_offset)
    theta = P.infection_uniform(seed, step, ids)
    r = P._block(seed, step | (1 << 62), ids >> np.uint64(1))
    odd = (ids & np.uint64(1)).astype(bool)
    u1, u2 = P.u01(np.where(odd, r[2], r[0])), P.u01(np.where(odd, r[3], r[1]))
    s = (-np.log(u1) - np.log(u2)).astype(np.float64)
    return theta.astype(np.float64) * s, (np.float32(1.0) - theta).astype(np.float64) * s, theta


def softmax_terms(p, e0, e1, dtype):
    """y0, y1 of the tau = 0.1 softmax in ``dtype``, op for op as csrc/gj_device.h:sampler_softmax"""
    p, e0, e1 = (np.asarray(v, dtype=dtype) for v in (p, e0, e1))
    tau = dtype(TAU)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z0 = (np.log(p) + (-np.log(e0))) / tau
        z1 = (np.log(dtype(1.0) - p) + (-np.log(e1))) / tau
        m = np.maximum(z0, z1)
        x0, x1 = np.exp(z0 - m), np.exp(z1 - m)
        return x0 / (x0 + x1), x1 / (x0 + x1)


def decisions(p, e0=None, e1=None, theta=None, dtype=np.float64):
    """nu per agent, as the forward (a float32 kernel) decides: the argmax rule in float32 for injected draws,
    p < theta for the library's.  Returned as ``dtype``."""
    if theta is not None:
        return (np.asarray(p, dtype=np.float32) < np.asarray(theta, dtype=np.float32)).astype(dtype)
    y0, y1 = softmax_terms(p, e0, e1, np.float32)
    return (y1 > y0).astype(dtype)


def seed_forward(p_not_by_group, labels, susc0, inf0, time0, now, e0=None, e1=None, theta=None, dtype=np.float64):
    """Returns (new_infected, susceptibility, is_infected, infection_time)."""
    p = np.asarray(p_not_by_group, dtype=dtype)[np.asarray(labels)]
    nu = decisions(p, e0, e1, theta, dtype)
    s0, i0, t0 = (np.asarray(v, dtype=dtype) for v in (susc0, inf0, time0))
    return nu, np.maximum(dtype(0.0), s0 - nu), i0 + nu, t0 + nu * (dtype(now) - t0)


def sampler_adjoint_terms(p, s0, t0, y0, y1, nu, now, gs, gi, gt, gn, dtype):
    """(h, nu_bar, d nu / d p) of one agent's a8 + a9 adjoint, every argument an array of ``dtype`` (csrc/gj_device.h,
    sample_adjoint): shared by the seed's adjoint below and by the sampler's (tests/gj_sampler_ref.py)."""
    x = s0 - nu
    h = np.where(x > 0, dtype(1.0), np.where(x == 0, dtype(0.5), dtype(0.0)))
    nu_bar = gi + gt * (dtype(now) - t0) - gs * h + gn
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dnu_dp = -(y0 * y1 / dtype(TAU)) * (dtype(1.0) / p + dtype(1.0) / (dtype(1.0) - p))
        dnu_dp = np.where(np.abs(dnu_dp) < 3.0e38, dnu_dp, dtype(0.0))
    return h, nu_bar, dnu_dp


def seed_adjoint(p_not_by_group, labels, n_groups, susc0, time0, now, e0, e1, theta=None, g_susc=None, g_inf=None,
                 g_time=None, g_new=None, dtype=np.float64, nu=None):
    """Returns a dict: ``grad_fraction`` [n_groups] (summed in float64 whatever ``dtype``), ``contrib`` (c_a),
    ``abs_sum`` (sum |c_a| per group), ``nu``, ``grad_susc`` = g_susc * h, ``grad_time`` = g_time * (1 - nu).
    ``labels`` None: every agent in group 0.  A label outside [0, n_groups): no term, nu = 0.  ``nu``: the forward's
    decisions when the caller has them (default: ``decisions``)."""
    n = len(np.asarray(susc0))
    labels = np.zeros(n, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    valid = (labels >= 0) & (labels < n_groups)
    lab = np.where(valid, labels, 0)
    zeros = np.zeros(n, dtype=dtype)
    gs, gi, gt, gn = (zeros if g is None else np.asarray(g, dtype=dtype) for g in (g_susc, g_inf, g_time, g_new))
    s0, t0 = np.asarray(susc0, dtype=dtype), np.asarray(time0, dtype=dtype)
    p = np.asarray(p_not_by_group, dtype=dtype)[lab]
    y0, y1 = softmax_terms(p, e0, e1, dtype)
    nu = decisions(p, e0, e1, theta, dtype) if nu is None else np.asarray(nu, dtype=dtype)
    nu = np.where(valid, nu, dtype(0.0))
    h, nu_bar, dnu_dp = sampler_adjoint_terms(p, s0, t0, y0, y1, nu, now, gs, gi, gt, gn, dtype)
    c = np.where(valid, -(nu_bar * dnu_dp), dtype(0.0))
    c64 = c.astype(np.float64)
    return {"grad_fraction": np.bincount(lab, weights=c64, minlength=n_groups)[:n_groups],
            "abs_sum": np.bincount(lab, weights=np.abs(c64), minlength=n_groups)[:n_groups],
            "contrib": c, "nu": nu, "grad_susc": gs * h, "grad_time": gt * (dtype(1.0) - nu)}
