"""Waning immunity (not in the reference, where an infected agent's susceptibility stays 0 for good): after every step
one launch, ``gj_immunity_step`` (include/gradjune_hip.h), relaxes the susceptibility of the recovered agents towards
``1 - residual_protection`` with the half-life of their age band, and undoes the step's increment of ``is_infected`` for an
agent that was infected before, so that the flag the transmission profile multiplies by stays 0 / 1.

    immunity:
      half_life: 180              # days; a number, or {"lo-hi": days} by age band; .inf = never wanes
      residual_protection: 0.2    # a number, or {"lo-hi": value} in [0, 1]: the protection that never goes away

Without the key nothing is allocated, launched or changed (``Immunity.from_parameters`` returns None).
"""
from __future__ import annotations

import math

import torch

from .policies import N_AGES, _age_band

LN2 = math.log(2.0)


def _values(v):
    return list(v.values()) if isinstance(v, dict) else [v]


class Immunity(torch.nn.Module):
    """``half_life`` and ``residual_protection``: float32 tensors [B], one value per age band in file order;
    ``band_of_age`` maps an age to its band (-1: none - the age does not wane).  A plain number is one band for every
    age; two dicts must name the same bands in the same order; a number beside a dict is broadcast over the dict's
    bands.  Either tensor may be replaced by an ``nn.Parameter`` of the same shape: a loss on the results then leaves
    its gradient in ``.grad``.  ``stages``: the model's symptom stages, which must hold ``recovered``."""

    def __init__(self, half_life, residual_protection=0.0, stages=("recovered",)):
        super().__init__()
        from .utils import parse_age_probabilities

        stages = [str(s) for s in stages]
        if "recovered" not in stages:
            raise ValueError(f"immunity: the symptom stages {stages} hold no 'recovered' stage")
        self.recovered_stage = stages.index("recovered")
        dicts = [v for v in (half_life, residual_protection) if isinstance(v, dict)]
        if dicts:
            keys = [str(k) for k in dicts[0]]
            if len(dicts) == 2 and [str(k) for k in dicts[1]] != keys:
                raise ValueError(f"immunity: mismatched bands: half_life names {[str(k) for k in half_life]}, "
                                 f"residual_protection {[str(k) for k in residual_protection]} (the same bands in the "
                                 "same order, or a plain number)")
            by_lo = sorted(_age_band(k) for k in keys)
            for (_, hi), (lo, _) in zip(by_lo, by_lo[1:]):
                if lo < hi:
                    raise ValueError(f"immunity: overlapping bands ({keys})")
            self.band_of_age = [int(b) for b in parse_age_probabilities({k: i for i, k in enumerate(keys)}, fill_value=-1)]
            n_bands = len(keys)
        else:
            self.band_of_age, n_bands = [0] * N_AGES, 1
        h, r = _values(half_life), _values(residual_protection)
        h, r = (h * n_bands if len(h) == 1 else h), (r * n_bands if len(r) == 1 else r)
        self.half_life = torch.tensor([float(v) for v in h], dtype=torch.float32)
        self.residual_protection = torch.tensor([float(v) for v in r], dtype=torch.float32)
        self._host_values()
        self._bands = self._cls = None

    @classmethod
    def from_parameters(cls, params):
        """The top-level ``immunity`` key of the YAML schema, or None without it."""
        cfg = params.get("immunity")
        if cfg is None:
            return None
        if "half_life" not in cfg:
            raise ValueError("immunity: half_life is required (days; .inf = never wanes)")
        stages = (params.get("symptoms") or {}).get("stages", ("recovered",))
        return cls(cfg["half_life"], cfg.get("residual_protection", 0.0), stages=stages)

    @property
    def n_bands(self) -> int:
        return max(self.band_of_age) + 1

    def requires_grad(self) -> bool:
        return bool(self.half_life.requires_grad or self.residual_protection.requires_grad)

    def _host_values(self):
        """(half-lives, residual protections) as Python doubles of the float32 values, checked."""
        h = [float(v) for v in self.half_life.detach().to(torch.float32).cpu().tolist()]
        r = [float(v) for v in self.residual_protection.detach().to(torch.float32).cpu().tolist()]
        if len(h) != self.n_bands or len(r) != self.n_bands:
            raise ValueError(f"immunity: half_life of shape {tuple(self.half_life.shape)} and residual_protection of "
                             f"shape {tuple(self.residual_protection.shape)}, expected [{self.n_bands}] (one value per band)")
        if any(not v > 0.0 for v in h):
            raise ValueError(f"immunity: half_life {h}: expected days > 0 (.inf = never wanes)")
        if any(not 0.0 <= v <= 1.0 for v in r):
            raise ValueError(f"immunity: residual_protection {r}: expected values in [0, 1]")
        return h, r

    @staticmethod
    def keep_of(dt: float, half_life: float) -> float:
        """2^(-dt / half_life) in Python doubles (1 for an infinite half-life)."""
        return 2.0 ** (-float(dt) / half_life)

    def tables(self, dt: float):
        """The launch's per-age tables (``gj_immunity_tables``), each value rounded once: keep = fp32(2^(-dt / h)), 1 for
        h = inf and for an age in no band; cap = fp32(1 - fp64(fp32(r))), 1 for an age in no band."""
        from . import _native as N

        h, r = self._host_values()
        t = N.ImmunityTables()
        for age in range(N_AGES):
            b = self.band_of_age[age]
            t.keep[age] = self.keep_of(dt, h[b]) if b >= 0 else 1.0      # (ctypes rounds the double to fp32: once)
            t.cap[age] = 1.0 - r[b] if b >= 0 else 1.0
        return t

    def measure(self, data, susc_sum_out):
        """One launch with every keep = 1 and ``new_infected`` NULL: nobody moves, ``data`` stays as it is, and
        ``susc_sum_out`` (device int64 [1]) gains the population's susceptibility in units of 2^-30 - the Runner's row 0."""
        from . import _native as N
        from .world import require_hip

        ag = data["agent"]
        dev = require_hip(ag["susceptibility"].device)
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        t = N.ImmunityTables()
        for age in range(N_AGES):
            t.keep[age] = t.cap[age] = 1.0
        susc, inf, stage = f32(ag["susceptibility"]), f32(ag["is_infected"]), f32(ag["symptoms"]["current_stage"])
        N.check(N.load().gj_immunity_step(susc.numel(), N.ptr(self._agent_class(ag, dev)), t, N.ptr(stage),
                                          self.recovered_stage, None, N.ptr(susc), N.ptr(inf), None, None, None,
                                          N.ptr(susc_sum_out), N.current_stream()), "gj_immunity_step")

    def bands(self, ages: torch.Tensor):
        """(int32 band per agent on the agents' device, its ``groups.SeedPlan``): what the adjoint sums through; built
        once per world."""
        if self._bands is None or self._bands[0].numel() != ages.numel() or self._bands[0].device != ages.device:
            from .groups import SeedPlan

            table = torch.tensor(self.band_of_age, dtype=torch.int32, device=ages.device)
            band = table[ages.long().clamp(0, N_AGES - 1)].contiguous()
            self._bands = (band, SeedPlan(band, self.n_bands, device=ages.device))
        return self._bands

    def _agent_class(self, ag, device):
        n = ag["age"].numel()
        if self._cls is None or self._cls.numel() != n or self._cls.device != device:
            sex = ag["sex"] if "sex" in ag else torch.zeros_like(ag["age"])
            self._cls = (sex.to(device).long() * 100 + ag["age"].to(device).long()).to(torch.uint8).contiguous()
        return self._cls

    def step(self, data, dt, new_infected, reinfected_out=None, count_out=None, susc_sum_out=None, all_reduce=None):
        """One ``gj_immunity_step`` on ``data["agent"]``: in place when nothing requires a gradient, through
        ``autograd.ImmunityStep`` otherwise.  ``dt``: the step's length in days; ``new_infected``: the step's 0 / 1
        outcome, or None for nobody; the optional outputs as the entry point takes them; ``all_reduce``: the sum over the
        ranks of the two gradient sums, on a rank of a partitioned world."""
        from . import _native as N
        from .world import require_hip

        ag = data["agent"]
        susc, inf = ag["susceptibility"], ag["is_infected"]
        dev = require_hip(susc.device)
        n = susc.numel()
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        env = {"cls": self._agent_class(ag, dev), "tables": self.tables(dt),
               "stage": f32(ag["symptoms"]["current_stage"]), "recovered": self.recovered_stage, "dt": float(dt),
               "reinfected": reinfected_out, "count": count_out, "susc_sum": susc_sum_out, "all_reduce": all_reduce}
        if torch.is_grad_enabled() and (self.requires_grad() or susc.requires_grad or inf.requires_grad or (
                new_infected is not None and new_infected.requires_grad)):
            from .autograd import ImmunityStep

            env["band"], env["plan"] = self.bands(ag["age"].to(dev))
            nw = new_infected if new_infected is not None else torch.zeros(n, dtype=torch.float32, device=dev)
            ag["susceptibility"], ag["is_infected"] = ImmunityStep.apply(
                env, self.half_life, self.residual_protection, susc, inf, nw)
            return
        for key in ("susceptibility", "is_infected"):
            t = ag[key]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.requires_grad or t.device != dev:
                ag[key] = f32(t)
        nw = None if new_infected is None else f32(new_infected)
        N.check(N.load().gj_immunity_step(n, N.ptr(env["cls"]), env["tables"], N.ptr(env["stage"]), env["recovered"],
                                          N.ptr(nw), N.ptr(ag["susceptibility"]), N.ptr(ag["is_infected"]), None,
                                          N.ptr(reinfected_out), N.ptr(count_out), N.ptr(susc_sum_out),
                                          N.current_stream()), "gj_immunity_step")
