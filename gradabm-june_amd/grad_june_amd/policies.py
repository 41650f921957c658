"""Date-windowed interventions: host-side logic whose OUTPUTS are hot-path inputs.

Mirror of the reference's policy classes (grad_june/policies/*.py): same class names, constructor
arguments, YAML schema and ``apply`` signatures.  What reaches the kernels per step:
  * SocialDistancing  -> a scalar factor on a network's beta      (interaction_policies.py:25-31)
  * Quarantine        -> ``q[a] = current_stage[a] < threshold``   (quarantine_policies.py:13-33);
                         the product over active policies is ``stage < min(thresholds)``, so the
                         kernels take one threshold (+inf when no policy is active)
  * CloseVenue        -> networks dropped from the step's list     (close_venue_policies.py:11-22)
Not in the reference:
  * ContactQuarantine -> a per-agent mask ``qstate`` (index cases and the complying members of the venues they marked,
                         ``gj_contact_mark`` / ``gj_contact_mask``) that the step takes in the place of the stage, with
                         the threshold 0.5
  * Vaccination       -> ``susceptibility[a] *= 1 - efficacy[band]`` for the agents a campaign's age-banded rollout
                         reaches in the step (``gj_vaccinate``); differentiable in the efficacy
  * Testing           -> confirmed cases - a share of the infections that reach a stage, by age, reported some days
                         later (``gj_testing_step``) - and, with ``isolation``, the mask ``qstate`` (3: isolating on a
                         positive result) that the step takes as it takes a ContactQuarantine's; differentiable in the
                         probability
"""
from __future__ import annotations

import math
import sys
from typing import List, Optional

import torch
import yaml

from .utils import read_date


class Policy(torch.nn.Module):
    spec: Optional[str] = None

    def __init__(self, start_date, end_date, device="cpu"):
        super().__init__()
        self.start_date = read_date(start_date)
        self.end_date = read_date(end_date)
        self.device = device

    def is_active(self, date) -> bool:
        return self.start_date <= date < self.end_date

    def apply(self, *args, **kwargs):
        raise NotImplementedError


class PolicyCollection(torch.nn.Module):
    """Policies of one kind.  Always truthy, like the reference's (an ``nn.Module``)."""

    def __init__(self, policies):
        super().__init__()
        self.policies = torch.nn.ModuleList(policies)

    def __getitem__(self, idx):
        return self.policies[idx]


# ---- interaction -------------------------------------------------------------------------------
class InteractionPolicy(Policy):
    spec = "interaction"


class SocialDistancing(InteractionPolicy):
    def __init__(self, start_date, end_date, beta_factors, device="cpu"):
        super().__init__(start_date, end_date, device)
        # factors live on the host: beta is a launch scalar, never a device tensor
        self.beta_factors = {k: torch.tensor(float(v)) for k, v in beta_factors.items()}

    def apply(self, beta, name, timer):
        if not self.is_active(timer.date):
            return beta
        factor = self.beta_factors.get(name)
        if factor is None:
            factor = self.beta_factors.get("all", torch.tensor(1.0))
        return beta * factor


class InteractionPolicies(PolicyCollection):
    def apply(self, beta, name, timer):
        for policy in self.policies:
            beta = policy.apply(beta=beta, name=name, timer=timer)
        return beta


# ---- quarantine --------------------------------------------------------------------------------
class Quarantine(Policy):
    spec = "quarantine"

    def __init__(self, start_date, end_date, stage_threshold, device="cpu"):
        super().__init__(start_date, end_date, device)
        self.stage_threshold = stage_threshold

    def apply(self, symptom_stages, timer):
        if self.is_active(timer.date):
            return (symptom_stages < self.stage_threshold).to(torch.float)
        return torch.ones(symptom_stages.shape, device=symptom_stages.device)


#: Philox stream of ContactQuarantine policy c: bit 59 set, c below (bits 60 to 63 are the tree's, the vaccination's,
#: the sampler's and the symptoms')
QUARANTINE_STREAM = 1 << 59


class ContactQuarantine(Quarantine):
    """Not in the reference: a ``Quarantine`` that also keeps the contacts of its index cases away.  While it is active,
    an agent with ``!(stage < stage_threshold)`` marks the venues it belongs to in the edge sets of ``contacts``
    (``{edge set: days}``, e.g. ``{"household": 14}``) for ``days`` days from the step's ``timer.now`` - a venue stays
    marked for ``days`` after the last step in which a member was symptomatic - and every complying member of a marked
    venue is quarantined with the index cases.  ``compliance``: the share of agents who comply, a plain number in
    [0, 1]; who complies is one Philox uniform per agent for the whole run (``u < fp32(compliance)``), not
    differentiable.  The launches and their state live in ``QuarantinePolicies``."""

    def __init__(self, start_date, end_date, stage_threshold, contacts, compliance=1.0, device="cpu"):
        super().__init__(start_date, end_date, stage_threshold, device)
        if not isinstance(contacts, dict) or not contacts:
            raise ValueError("contact_quarantine: contacts is a non-empty mapping {edge set: days}")
        self.contacts = {}
        for name, days in contacts.items():
            days = float(days)
            if not days > 0.0:
                raise ValueError(f"contact_quarantine: contacts['{name}'] = {days}, expected days > 0")
            self.contacts[str(name)] = days
        if isinstance(compliance, torch.Tensor) and compliance.requires_grad:
            raise NotImplementedError("contact_quarantine: gradients w.r.t. the compliance are not implemented (pass a "
                                      "plain number)")
        self.compliance = float(compliance)
        if not 0.0 <= self.compliance <= 1.0:
            raise ValueError(f"contact_quarantine: compliance = {self.compliance}, expected a share in [0, 1]")

    def window(self) -> str:
        return f"[{self.start_date:%Y-%m-%d}, {self.end_date:%Y-%m-%d})"


class ContactQuarantineError(RuntimeError):
    """gj_contact_mark / gj_contact_mask met a row pointer or venue id outside its edge set."""


class QuarantinePolicies(PolicyCollection):
    """``apply`` records the step's threshold; ``contact_step`` - called next, by whoever launches the step - runs the
    active ``ContactQuarantine`` (at most one: their windows must not overlap) and leaves the step's mask in
    ``qstate`` (fp32 per agent: 0 free, 1 index case, 2 contact; None while no ``ContactQuarantine`` is active).  The
    step then runs with ``launch_stage`` / ``launch_threshold`` in the place of the symptom stage and ``threshold``."""

    def __init__(self, policies):
        super().__init__(policies)
        self._stages = None
        self.threshold = math.inf
        self.qstate = None
        self.contact_policies = [p for p in self.policies if isinstance(p, ContactQuarantine)]
        for i, a in enumerate(self.contact_policies):
            for b in self.contact_policies[i + 1:]:
                if a.start_date < b.end_date and b.start_date < a.end_date:
                    raise ValueError(f"contact_quarantine: the windows {a.window()} and {b.window()} overlap")
        self._contact = {}          # policy index -> what its launches need, allocated at its first active step
        self._qstate_buffer = None
        self._err = None

    def apply(self, symptom_stages, timer):
        """Records the step's threshold; the per-agent mask itself is formed inside the kernels
        (and lazily by :attr:`quarantine_mask` for callers that want the tensor)."""
        self._stages = symptom_stages
        active = [float(p.stage_threshold) for p in self.policies if p.is_active(timer.date)]
        self.threshold = min(active) if active else math.inf
        self.qstate = None

    @property
    def launch_threshold(self) -> float:
        """The step's ``q_threshold``: 0.5 on ``qstate`` while a ``ContactQuarantine`` is active, else ``threshold``."""
        return 0.5 if self.qstate is not None else self.threshold

    def reset(self):
        """Forget what a run marked: every ``until`` back to zero (never marked)."""
        for held in self._contact.values():
            for until in held["until"]:
                until.zero_()
        self.qstate = None

    def _contact_state(self, c, policy, plan, edges):
        held = self._contact.get(c)
        if held is None or held["plan"] is not plan:
            from . import _native as N

            rows = plan.contact_rows(list(policy.contacts), edges() if callable(edges) else edges)
            until = [torch.zeros(max(1, n_venues), dtype=torch.int32, device=plan.device) for _, _, n_venues in rows]
            sets = (N.ContactSet * len(rows))()
            for k, ((rowptr, venue, n_venues), u) in enumerate(zip(rows, until)):
                sets[k].a_rowptr, sets[k].a_venue, sets[k].until = rowptr.data_ptr(), venue.data_ptr(), u.data_ptr()
                sets[k].n_venues = n_venues
            held = self._contact[c] = {"plan": plan, "rows": rows, "until": until, "sets": sets,
                                       "days": list(policy.contacts.values())}
        return held

    def contact_step(self, plan, timer, seed, agent_offset=0, edges=None):
        """Mark, then mask, for the ``ContactQuarantine`` active at ``timer.date``: returns ``qstate`` (and keeps it
        until the next ``apply``), or None - nothing launched, nothing allocated - when none is active.  Call it after
        ``apply``, on the ``current_stage`` the step starts from.  ``plan``: the step's ``DevicePlan``; ``seed``: the
        run's Philox key; ``agent_offset``: the global id of local agent 0; ``edges``: the world's COO edge lists by set
        name, or a callable that returns them (asked for only when the policy's by-agent rows have to be built)."""
        self.qstate = None
        for c, policy in enumerate(self.contact_policies):
            if policy.is_active(timer.date):
                break
        else:
            return None
        from . import _native as N

        now = float(timer.now)
        if now < 0.0:
            raise ValueError(f"contact_quarantine: timer.now = {now}, expected a time >= 0")
        held = self._contact_state(c, policy, plan, edges)
        dev, n = plan.device, plan.host.n_agents
        stage = self._stages
        if stage.dtype != torch.float32 or stage.device != dev or not stage.is_contiguous() or stage.requires_grad:
            stage = stage.detach().to(device=dev, dtype=torch.float32).contiguous()
        if stage.numel() != n:
            raise ValueError(f"contact_quarantine: {stage.numel()} stages for {n} agents")
        if self._qstate_buffer is None or self._qstate_buffer.numel() != n or self._qstate_buffer.device != dev:
            self._qstate_buffer = torch.empty(n, dtype=torch.float32, device=dev)
        if self._err is None or self._err.device != dev:
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        sets = held["sets"]
        for k, days in enumerate(held["days"]):
            sets[k].release = now + days          # (ctypes rounds the double to fp32: once)
        lib, stream = N.load(), N.current_stream()
        N.check(lib.gj_contact_mark(n, N.ptr(stage), float(policy.stage_threshold), sets, len(sets), N.ptr(self._err),
                                    stream), "gj_contact_mark")
        N.check(lib.gj_contact_mask(n, N.ptr(stage), float(self.threshold), sets, len(sets), now, policy.compliance,
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, QUARANTINE_STREAM | c, int(agent_offset),
                                    N.ptr(self._qstate_buffer), N.ptr(self._err), stream), "gj_contact_mask")
        self.qstate = self._qstate_buffer
        return self.qstate

    def check(self, what: str = "contact quarantine") -> None:
        """Raise if a launch since the last check met a row outside its edge set (one device read)."""
        if self._err is None:
            return
        err = int(self._err.item()) & 0xFFFFFFFF
        if err:
            self._err.zero_()
            raise ContactQuarantineError(f"{what}: a row pointer or venue id outside its edge set (it was skipped)")

    @property
    def quarantine_mask(self):
        if self._stages is None:
            return 1.0
        if self.qstate is not None:
            return (self.qstate < 0.5).to(torch.float)
        if math.isinf(self.threshold):
            return torch.ones(self._stages.shape, device=self._stages.device)
        return (self._stages < self.threshold).to(torch.float)


# ---- close venue -------------------------------------------------------------------------------
class CloseVenue(Policy):
    spec = "close_venue"

    def __init__(self, start_date, end_date, names, device="cpu"):
        super().__init__(start_date, end_date, device)
        self.edge_type_to_close = {str(n) for n in names}

    def apply(self, edge_types, timer):
        if not self.is_active(timer.date):
            return edge_types
        return [e for e in edge_types if e not in self.edge_type_to_close]


class CloseVenuePolicies(PolicyCollection):
    def apply(self, edge_types, timer):
        for policy in self.policies:
            edge_types = policy.apply(edge_types=edge_types, timer=timer)
        return edge_types


# ---- vaccination (not in the reference) --------------------------------------------------------
#: Philox stream of campaign c: bit 61 set, c below (bits 62 and 63 and the 1 << 40 counter are the steps' and symptoms')
VACCINE_STREAM = 1 << 61
N_AGES = 100


def _plain_number(v, what):
    """A YAML number or a tensor without a gradient as a Python double; one that requires a gradient is refused."""
    if isinstance(v, torch.Tensor):
        if v.requires_grad:
            raise NotImplementedError(f"{what}: gradients w.r.t. the vaccination coverage are not implemented "
                                      "(pass plain numbers; the efficacy is the differentiable input)")
        return float(v.detach())
    return float(v)


def _age_band(key):
    lo, hi = (int(x) for x in str(key).split("-"))
    if not 0 <= lo < hi:
        raise ValueError(f"age band '{key}': expected 'lo-hi' with 0 <= lo < hi")
    return lo, hi


class Vaccination(Policy):
    """One campaign: between ``start_date`` and ``end_date`` the share ``coverage[age] * ramp(date)`` of every age is
    vaccinated, and an agent's vaccination multiplies its susceptibility by ``1 - efficacy[band of its age]``, once and
    for good (the effect persists after ``end_date``).

    ``coverage``: a number (every age) or ``{"lo-hi": fraction}`` (``parse_age_probabilities``: lo <= age < hi, gaps 0);
    kept as 100 Python doubles; not differentiable.  ``efficacy``: a number (one band, every age) or ``{"lo-hi":
    value}``: ``self.efficacy`` is a float32 tensor [B], one value per band in file order, and ``band_of_age`` maps an
    age to its band (-1: none, efficacy 0).  ``self.efficacy`` may be replaced by an ``nn.Parameter`` of the same shape:
    a loss on the results then leaves ``d loss / d efficacy`` in its ``.grad``.

    Who is vaccinated when is decided without per-agent state: campaign ``c`` (its index in ``VaccinationPolicies``)
    gives agent ``a`` one uniform ``u`` for the whole run, and the campaign has reached the agent by ``date`` iff
    ``u < coverage[age] * ramp(date)``.  ``applied`` is the ramp applied so far in this run (``reset`` zeroes it)."""

    spec = "vaccination"

    def __init__(self, start_date, end_date, coverage, efficacy, device="cpu"):
        super().__init__(start_date, end_date, device)
        if self.end_date < self.start_date:
            raise ValueError(f"vaccination: end_date {self.end_date:%Y-%m-%d} before start_date {self.start_date:%Y-%m-%d}")
        from .utils import parse_age_probabilities

        if isinstance(coverage, dict):
            for key in coverage:
                _age_band(key)
            self.coverage = [float(v) for v in parse_age_probabilities(
                {str(k): _plain_number(v, f"coverage['{k}']") for k, v in coverage.items()})]
        else:
            self.coverage = [_plain_number(coverage, "coverage")] * N_AGES
        if isinstance(efficacy, dict):
            bands = [_age_band(k) for k in efficacy]
            by_lo = sorted(bands)
            for (_, hi), (lo, _) in zip(by_lo, by_lo[1:]):
                if lo < hi:
                    raise ValueError(f"vaccination: overlapping efficacy bands ({sorted(map(str, efficacy))})")
            values = list(efficacy.values())
            self.band_of_age = [int(b) for b in parse_age_probabilities(
                {str(k): i for i, k in enumerate(efficacy)}, fill_value=-1)]
        else:
            values, self.band_of_age = [efficacy], [0] * N_AGES
        if any(isinstance(v, torch.Tensor) and v.requires_grad for v in values):
            self.efficacy = torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(()) for v in values])
        else:
            self.efficacy = torch.tensor([float(v) for v in values], dtype=torch.float32)
        self.applied = 0.0
        self._bands = None

    def reset(self):
        self.applied = 0.0

    def ramp(self, date) -> float:
        """clamp((date - start) / (end - start), 0, 1) in Python doubles; 1 from ``end_date`` on (also when the window
        is empty: everybody the campaign covers is vaccinated at once)."""
        if date >= self.end_date:
            return 1.0
        if date <= self.start_date:
            return 0.0
        return ((date - self.start_date).total_seconds() / (self.end_date - self.start_date).total_seconds())

    def tables(self, lo: float, hi: float):
        """The launch's per-age tables (``gj_vaccinate_tables``), each value rounded once: thresholds fp32(fp64(coverage)
        * ramp) for the ramps ``lo`` and ``hi``, factors fp32(1 - fp64(efficacy of the age's band)), 1 without a band."""
        from . import _native as N

        eff = [float(v) for v in self.efficacy.detach().to(torch.float32).cpu().tolist()]
        if len(eff) != max(self.band_of_age) + 1:
            raise ValueError(f"vaccination: efficacy of shape {tuple(self.efficacy.shape)}, expected "
                             f"[{max(self.band_of_age) + 1}] (one value per band)")
        t = N.VaccinateTables()
        for age in range(N_AGES):
            t.thr_lo[age] = self.coverage[age] * lo          # (ctypes rounds the double to fp32: once)
            t.thr_hi[age] = self.coverage[age] * hi
            b = self.band_of_age[age]
            t.factor[age] = 1.0 - eff[b] if b >= 0 else 1.0
        return t

    def bands(self, ages: torch.Tensor):
        """(int32 band per agent on the agents' device, its ``groups.SeedPlan``): what the adjoint sums through; built
        once per world."""
        if self._bands is None or self._bands[0].numel() != ages.numel() or self._bands[0].device != ages.device:
            from .groups import SeedPlan

            table = torch.tensor(self.band_of_age, dtype=torch.int32, device=ages.device)
            band = table[ages.long().clamp(0, N_AGES - 1)].contiguous()
            self._bands = (band, SeedPlan(band, max(self.band_of_age) + 1, device=ages.device))
        return self._bands


class VaccinationPolicies(PolicyCollection):
    """The campaigns, in list order: a campaign's index is its Philox stream.  ``apply`` launches ``gj_vaccinate`` once
    for every campaign whose ramp rose since it was last applied (``lo`` = the ramp applied, ``hi`` = the ramp now); with
    none rising nothing is launched and nothing is allocated.  ``doses``: device int64 [C], the doses given so far in
    this run by campaign (None before the first launch); ``on_newly``: set by the Runner for its time loop - called with
    every launch's 0 / 1 mask of the newly vaccinated (without it the mask is not written)."""

    def __init__(self, policies):
        super().__init__(policies)
        self.doses = None
        self.on_newly = None
        self._cls = None

    def reset(self):
        for policy in self.policies:
            policy.reset()
        if self.doses is not None:
            self.doses.zero_()

    def requires_grad(self) -> bool:
        return any(isinstance(p.efficacy, torch.Tensor) and p.efficacy.requires_grad for p in self.policies)

    def _agent_class(self, ag, device):
        n = ag["age"].numel()
        if self._cls is None or self._cls.numel() != n or self._cls.device != device:
            sex = ag["sex"] if "sex" in ag else torch.zeros_like(ag["age"])
            self._cls = (sex.to(device).long() * 100 + ag["age"].to(device).long()).to(torch.uint8).contiguous()
        return self._cls

    def apply(self, data, timer, seed, agent_offset=0, all_reduce=None):
        from . import _native as N
        from .world import require_hip

        for c, policy in enumerate(self.policies):
            lo, hi = policy.applied, policy.ramp(timer.date)
            if not hi > lo:
                continue
            policy.applied = hi
            ag = data["agent"]
            susc = ag["susceptibility"]
            dev = require_hip(susc.device)
            n = susc.numel()
            cls = self._agent_class(ag, dev)
            if self.doses is None or self.doses.device != dev:
                self.doses = torch.zeros(len(self.policies), dtype=torch.int64, device=dev)
            newly = torch.empty(n, dtype=torch.float32, device=dev) if self.on_newly is not None else None
            env = {"cls": cls, "tables": policy.tables(lo, hi), "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                   "stream": VACCINE_STREAM | c, "agent_offset": int(agent_offset), "newly": newly,
                   "count": self.doses[c:c + 1], "all_reduce": all_reduce}
            eff = policy.efficacy
            if torch.is_grad_enabled() and (eff.requires_grad or susc.requires_grad):
                from .autograd import VaccinationStep

                env["band"], env["plan"] = policy.bands(ag["age"].to(dev))
                ag["susceptibility"] = VaccinationStep.apply(env, eff, susc)
            else:
                if susc.dtype != torch.float32 or not susc.is_contiguous() or susc.requires_grad:
                    susc = ag["susceptibility"] = susc.detach().to(torch.float32).contiguous()
                N.check(N.load().gj_vaccinate(n, N.ptr(cls), env["tables"], env["seed"], env["stream"],
                                              env["agent_offset"], N.ptr(susc), N.ptr(newly), N.ptr(env["count"]),
                                              N.current_stream()), "gj_vaccinate")
            if newly is not None:
                self.on_newly(c, newly)


# ---- testing (not in the reference) --------------------------------------------------------------
#: Philox streams of Testing policy c: bit 58 set; a decision's is ``c << 32 | bits(infection_time)`` below it, the
#: compliance uniform's has bit 57 set and c below (bits 59 to 63 are the other policies', the sampler's and the symptoms')
TESTING_STREAM = 1 << 58
TESTING_COMPLY_STREAM = TESTING_STREAM | 1 << 57
TESTING_MAX_DELAYS = 16


class Testing(Policy):
    """An observation model: while the policy is active, an infection that reaches ``stage_threshold`` (``!(stage <
    stage_threshold)``, the step's own rule) is tested and found with the probability of the agent's age, once per
    infection, and the result arrives ``delay`` days later.  A positive result is a confirmed case - what surveillance
    data count - and, with ``isolation``, keeps a complying agent away from the step for ``days`` days.

    ``probability``: ascertainment, a number (one band, every age) or ``{"lo-hi": p}``: ``self.probability`` is a float32
    tensor [B], one value per band in file order, and ``band_of_age`` maps an age to its band (-1: none, p = 0).  It may be
    replaced by an ``nn.Parameter`` of the same shape: a loss on the confirmed series then leaves its gradient in
    ``.grad`` (a straight-through estimator: every decision counts 1, so the sum is the exact derivative of the expected
    count).  ``delay``: a number of days >= 0, or ``{days: share}`` with at most 16 entries whose shares sum to 1;
    ``delay_days`` and ``delay_cum`` hold the days and the cumulative shares, each an fp32 value rounded once.
    ``isolation``: ``{days: > 0, compliance: share in [0, 1], default 1}`` or None; who complies is one Philox uniform per
    agent for the whole run (``u < fp32(compliance)``).  Neither the delay nor the compliance is differentiable, and the
    isolation mask is hard: no gradient flows from ``probability`` into the epidemic.  The launches and their state live
    in ``TestingPolicies``."""

    spec = "testing"

    def __init__(self, start_date, end_date, stage_threshold, probability, delay=0, isolation=None, device="cpu"):
        super().__init__(start_date, end_date, device)
        from .utils import parse_age_probabilities

        self.stage_threshold = float(stage_threshold)
        if isinstance(probability, dict):
            bands = [_age_band(k) for k in probability]
            by_lo = sorted(bands)
            for (_, hi), (lo, _) in zip(by_lo, by_lo[1:]):
                if lo < hi:
                    raise ValueError(f"testing: overlapping probability bands ({sorted(map(str, probability))})")
            values = list(probability.values())
            self.band_of_age = [int(b) for b in parse_age_probabilities(
                {str(k): i for i, k in enumerate(probability)}, fill_value=-1)]
        else:
            values, self.band_of_age = [probability], [0] * N_AGES
        if any(isinstance(v, torch.Tensor) and v.requires_grad for v in values):
            self.probability = torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(()) for v in values])
        else:
            self.probability = torch.tensor([float(v) for v in values], dtype=torch.float32)
        self._host_probability()
        entries = list(delay.items()) if isinstance(delay, dict) else [(delay, 1.0)]
        if not 1 <= len(entries) <= TESTING_MAX_DELAYS:
            raise ValueError(f"testing: delay has {len(entries)} entries, expected 1 to {TESTING_MAX_DELAYS}")
        days, shares = [float(d) for d, _ in entries], [float(s) for _, s in entries]
        for d in days:
            if not (d >= 0.0 and math.isfinite(d)):
                raise ValueError(f"testing: delay of {d} days, expected days >= 0")
        for s in shares:
            if not s >= 0.0:
                raise ValueError(f"testing: delay share {s}, expected a share >= 0")
        if abs(sum(shares) - 1.0) > 1e-6:
            raise ValueError(f"testing: the delay shares sum to {sum(shares)}, expected 1")
        self.delay_days = torch.tensor(days, dtype=torch.float32)
        self.delay_cum = torch.tensor([sum(shares[:k + 1]) for k in range(len(shares))], dtype=torch.float64).to(torch.float32)
        self.isolation_days, self.compliance = None, 1.0
        if isolation is not None:
            if not isinstance(isolation, dict) or "days" not in isolation or set(isolation) - {"days", "compliance"}:
                raise ValueError(f"testing: isolation = {isolation}, expected {{days: .., compliance: ..}}")
            self.isolation_days = float(isolation["days"])
            if not (self.isolation_days > 0.0 and math.isfinite(self.isolation_days)):
                raise ValueError(f"testing: isolation days = {self.isolation_days}, expected days > 0")
            compliance = isolation.get("compliance", 1.0)
            if isinstance(compliance, torch.Tensor) and compliance.requires_grad:
                raise NotImplementedError("testing: gradients w.r.t. the compliance are not implemented (pass a plain "
                                          "number)")
            self.compliance = float(compliance)
            if not 0.0 <= self.compliance <= 1.0:
                raise ValueError(f"testing: compliance = {self.compliance}, expected a share in [0, 1]")
        self._bands = None

    @property
    def isolates(self) -> bool:
        return self.isolation_days is not None

    @property
    def n_bands(self) -> int:
        return max(self.band_of_age) + 1

    def window(self) -> str:
        return f"[{self.start_date:%Y-%m-%d}, {self.end_date:%Y-%m-%d})"

    def _host_probability(self):
        """The probabilities as Python doubles of the float32 values, checked."""
        p = [float(v) for v in self.probability.detach().to(torch.float32).cpu().tolist()]
        if len(p) != self.n_bands:
            raise ValueError(f"testing: probability of shape {tuple(self.probability.shape)}, expected [{self.n_bands}] "
                             "(one value per band)")
        for v in p:
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"testing: probability = {v}, expected a value in [0, 1]")
        return p

    def tables(self):
        """The launch's tables (``gj_testing_tables``), each value rounded once: the probability per age (0 for an age in
        no band), the cumulative shares and the days of the delay."""
        from . import _native as N

        p = self._host_probability()
        t = N.TestingTables()
        for age in range(N_AGES):
            b = self.band_of_age[age]
            t.probability[age] = p[b] if b >= 0 else 0.0
        t.n_delays = self.delay_days.numel()
        for k in range(t.n_delays):
            t.delay_cum[k], t.delay_days[k] = float(self.delay_cum[k]), float(self.delay_days[k])
        return t

    def bands(self, ages: torch.Tensor):
        """(int32 band per agent on the agents' device, its ``groups.SeedPlan``): what the adjoint sums through; built
        once per world."""
        if self._bands is None or self._bands[0].numel() != ages.numel() or self._bands[0].device != ages.device:
            from .groups import SeedPlan

            table = torch.tensor(self.band_of_age, dtype=torch.int32, device=ages.device)
            band = table[ages.long().clamp(0, N_AGES - 1)].contiguous()
            self._bands = (band, SeedPlan(band, self.n_bands, device=ages.device))
        return self._bands


class TestingPolicies(PolicyCollection):
    """The ``Testing`` policies, in list order: a policy's index is its Philox stream; their windows must not overlap.
    ``step`` - called by whoever launches the step, after ``Policies.apply`` and on the stage the step starts from -
    launches ``gj_testing_step`` for every policy from its first active step to the end of the run (results keep
    arriving after ``end_date``; decisions are made only while the policy is active).  Per-agent state, allocated at a
    policy's first active step and put back by ``reset``: ``decided`` / ``result_time`` / ``positive`` per policy (12 B
    an agent) and ``isolate_until`` / ``confirmed_time`` for the run (8 B).  ``qstate``: the mask of the last launch of
    an isolating policy (fp32 per agent: 0 free, 1 at or above the plain ``Quarantine`` threshold, 3 isolating), or None.
    ``sink``: set by the Runner for its time loop - ``{"counts": device int64 [2], "on_newly": callable or None, "rows":
    list}``: the launches add their newly confirmed cases and decisions to ``counts``, hand ``on_newly`` their 0 / 1
    mask, and a differentiable launch appends its row (a scalar on the graph) to ``rows``."""

    def __init__(self, policies):
        super().__init__(policies)
        for i, a in enumerate(self.policies):
            for b in self.policies[i + 1:]:
                if a.start_date < b.end_date and b.start_date < a.end_date:
                    raise ValueError(f"testing: the windows {a.window()} and {b.window()} overlap")
        self.sink = None
        self.qstate = None
        self.isolate_until = self.confirmed_time = None
        self._state = {}            # policy index -> its per-agent arrays, from its first active step on
        self._cls = self._qstate_buffer = None

    @property
    def isolating(self) -> bool:
        return any(p.isolates for p in self.policies)

    def requires_grad(self) -> bool:
        return any(isinstance(p.probability, torch.Tensor) and p.probability.requires_grad for p in self.policies)

    def reset(self):
        """Forget a run: every policy waits for its first active step again, and the arrays go back to their initial
        values."""
        self._state = {}
        self.qstate = None
        if self.isolate_until is not None:
            self.isolate_until.zero_()
            self.confirmed_time.fill_(-1.0)

    def _agent_class(self, ag, device):
        n = ag["age"].numel()
        if self._cls is None or self._cls.numel() != n or self._cls.device != device:
            sex = ag["sex"] if "sex" in ag else torch.zeros_like(ag["age"])
            self._cls = (sex.to(device).long() * 100 + ag["age"].to(device).long()).to(torch.uint8).contiguous()
        return self._cls

    def _started(self, c, n, dev):
        if self.isolate_until is None or self.isolate_until.numel() != n or self.isolate_until.device != dev:
            self.isolate_until = torch.zeros(n, dtype=torch.float32, device=dev)
            self.confirmed_time = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
        held = self._state.get(c)
        if held is None or held["decided"].numel() != n or held["decided"].device != dev:
            held = self._state[c] = {
                # (int32 -1: the bit pattern 0xFFFFFFFF)
                "decided": torch.full((n,), -1, dtype=torch.int32, device=dev),
                "result_time": torch.full((n,), math.inf, dtype=torch.float32, device=dev),
                "positive": torch.zeros(n, dtype=torch.float32, device=dev), "y": None}
        return held

    def state(self, c=0):
        """Policy c's per-agent arrays (``decided`` as int32 bit patterns), or None before its first active step."""
        return self._state.get(c)

    def step(self, data, timer, seed, q_threshold=math.inf, agent_offset=0, all_reduce=None):
        """See the class.  ``seed``: the run's Philox key; ``q_threshold``: the active plain ``Quarantine`` minimum
        (``QuarantinePolicies.threshold``); ``agent_offset``: the global id of local agent 0 and ``all_reduce``: the sum
        over the ranks of the probability's gradient, on a rank of a partitioned world.  Returns ``qstate``.  Without a
        policy that has started: nothing launched, nothing allocated."""
        self.qstate = None
        running = [(c, p) for c, p in enumerate(self.policies) if c in self._state or p.is_active(timer.date)]
        if not running:
            return None
        from . import _native as N
        from .world import require_hip

        now = float(timer.now)
        if now < 0.0:
            raise ValueError(f"testing: timer.now = {now}, expected a time >= 0")
        ag = data["agent"]
        stage_in, inf_time = ag["symptoms"]["current_stage"], ag["infection_time"]
        dev = require_hip(inf_time.device)
        n = inf_time.numel()
        f32 = lambda t: (t if t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and not t.requires_grad
                         else t.detach().to(device=dev, dtype=torch.float32).contiguous())
        stage, inf_time = f32(stage_in), f32(inf_time)
        if stage.numel() != n:
            raise ValueError(f"testing: {stage.numel()} stages for {n} agents")
        cls = self._agent_class(ag, dev)
        sink = self.sink or {}
        want_newly = sink.get("on_newly") is not None
        for c, policy in running:
            held = self._started(c, n, dev)
            qstate = None
            if policy.isolates:
                if self._qstate_buffer is None or self._qstate_buffer.numel() != n or self._qstate_buffer.device != dev:
                    self._qstate_buffer = torch.empty(n, dtype=torch.float32, device=dev)
                qstate = self._qstate_buffer
            newly = torch.empty(n, dtype=torch.float32, device=dev) if want_newly else None
            env = {"n": n, "cls": cls, "tables": policy.tables(), "stage": stage, "inf_time": inf_time,
                   "threshold": policy.stage_threshold, "active": int(policy.is_active(timer.date)), "now": now,
                   "q_threshold": float(q_threshold),
                   "release": now + policy.isolation_days if policy.isolates else 0.0,      # (ctypes rounds to fp32: once)
                   "compliance": policy.compliance, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                   "decide_stream": TESTING_STREAM | c << 32, "comply_stream": TESTING_COMPLY_STREAM | c,
                   "agent_offset": int(agent_offset), "held": held,
                   "isolate_until": self.isolate_until if policy.isolates else None,
                   "confirmed_time": self.confirmed_time, "newly": newly, "qstate": qstate,
                   "counts": sink.get("counts"), "all_reduce": all_reduce}
            prob = policy.probability
            if torch.is_grad_enabled() and (prob.requires_grad or stage_in.requires_grad):
                from .autograd import TestingStep

                env["band"], env["plan"] = policy.bands(ag["age"].to(dev))
                y_prev = held["y"] if held["y"] is not None else held["positive"].clone()
                held["y"], row = TestingStep.apply(env, prob, stage_in, y_prev)
                if "rows" in sink:
                    sink["rows"].append(row)
            else:
                testing_launch(env, None)
            if want_newly:
                sink["on_newly"](newly)
            if qstate is not None:
                self.qstate = qstate
        return self.qstate


def testing_launch(env, flags):
    """One ``gj_testing_step`` from what ``TestingPolicies.step`` put together."""
    from . import _native as N

    held = env["held"]
    N.check(N.load().gj_testing_step(
        env["n"], N.ptr(env["cls"]), env["tables"], N.ptr(env["stage"]), N.ptr(env["inf_time"]), env["threshold"],
        env["active"], env["now"], env["q_threshold"], env["release"], env["compliance"], env["seed"],
        env["decide_stream"], env["comply_stream"], env["agent_offset"], N.ptr(held["decided"]),
        N.ptr(held["result_time"]), N.ptr(held["positive"]), N.ptr(env["isolate_until"]), N.ptr(env["confirmed_time"]),
        N.ptr(env["newly"]), N.ptr(env["qstate"]), N.ptr(flags), N.ptr(env["counts"]), N.current_stream()),
        "gj_testing_step")


def _refuse_isolation_beside_contact_quarantine(quarantine_policies, testing_policies):
    """Both write the step's mask: an isolating ``Testing`` and a ``ContactQuarantine`` must not share a date."""
    for t in getattr(testing_policies, "policies", None) or []:
        for q in getattr(quarantine_policies, "contact_policies", None) or []:
            if t.isolates and t.start_date < q.end_date and q.start_date < t.end_date:
                raise ValueError(f"testing: the window {t.window()} of a Testing with isolation overlaps the "
                                 f"ContactQuarantine's {q.window()}")


# ---- container ---------------------------------------------------------------------------------
class Policies(torch.nn.Module):
    def __init__(self, interaction_policies=None, quarantine_policies=None, close_venue_policies=None,
                 vaccination_policies=None, testing_policies=None):
        super().__init__()
        self.interaction_policies = interaction_policies
        self.quarantine_policies = quarantine_policies
        self.close_venue_policies = close_venue_policies
        self.vaccination_policies = vaccination_policies
        self.testing_policies = testing_policies
        _refuse_isolation_beside_contact_quarantine(quarantine_policies, testing_policies)

    @classmethod
    def from_policy_list(cls, policies):
        policies = list(policies or [])

        def of(kind):
            return [p for p in policies if p.spec == kind]

        return cls(
            interaction_policies=InteractionPolicies(of("interaction")),
            quarantine_policies=QuarantinePolicies(of("quarantine")),
            close_venue_policies=CloseVenuePolicies(of("close_venue")),
            vaccination_policies=VaccinationPolicies(of("vaccination")),
            testing_policies=TestingPolicies(of("testing")),
        )

    @classmethod
    def from_file(cls, fpath=None):
        if fpath is None:
            from .defaults import default_parameters

            return cls.from_parameters(default_parameters())
        with open(fpath) as f:
            return cls.from_parameters(yaml.safe_load(f))

    @classmethod
    def from_parameters(cls, params):
        device = params["system"]["device"]
        found: List[Policy] = []
        for group in (params.get("policies") or {}).values():
            for name, config in group.items():
                found += cls._parse_policy_config(config, name=name, device=device)
        return cls.from_policy_list(found)

    @staticmethod
    def _parse_policy_config(config, name, device):
        """``social_distancing`` -> class ``SocialDistancing``; either one window or numbered windows."""
        cls_name = "".join(part.capitalize() for part in name.split("_"))
        policy_class = getattr(sys.modules[__name__], cls_name)
        if "start_date" in config:
            return [policy_class(**config, device=device)]
        out = []
        for window in config.values():
            if "start_date" not in window or "end_date" not in window:
                raise ValueError("policy config file not valid.")
            out.append(policy_class(**window, device=device))
        return out

    def apply(self, data, timer):
        if self.quarantine_policies:
            self.quarantine_policies.apply(
                timer=timer, symptom_stages=data["agent"]["symptoms"]["current_stage"]
            )

    def reset(self):
        """Forget what a run applied (the vaccination ramps and dose counts, the venues a ``ContactQuarantine`` marked):
        ``Runner.forward`` calls it next to ``timer.reset()``."""
        if self.vaccination_policies is not None:
            self.vaccination_policies.reset()
        if self.quarantine_policies is not None and hasattr(self.quarantine_policies, "reset"):
            self.quarantine_policies.reset()
        if getattr(self, "testing_policies", None) is not None:
            self.testing_policies.reset()

    def test(self, data, timer, seed, agent_offset=0, all_reduce=None):
        """The ``Testing`` policies' launch (``TestingPolicies.step``) on the stage the step starts from: call it after
        ``apply``.  The mask of an isolating policy is left in ``quarantine_policies.qstate``, where the step reads a
        ``ContactQuarantine``'s.  Without a ``Testing`` policy: nothing."""
        tp = getattr(self, "testing_policies", None)
        if tp is None or len(tp.policies) == 0:
            return
        qp = self.quarantine_policies
        if tp.isolating and qp is None:
            raise ValueError("testing: isolation needs Policies.quarantine_policies (an empty QuarantinePolicies will do)")
        qstate = tp.step(data, timer, seed, q_threshold=qp.threshold if qp is not None else math.inf,
                         agent_offset=agent_offset, all_reduce=all_reduce)
        if qp is not None:
            qp.qstate = qstate

    def vaccinate(self, data, timer, seed, agent_offset=0, all_reduce=None):
        """Move ``data["agent"].susceptibility`` for every campaign whose ramp rose since it was last applied
        (``VaccinationPolicies.apply``).  ``seed``: the run's Philox key; ``agent_offset``: the global id of local agent
        0 and ``all_reduce``: the sum over the ranks of the efficacy's gradient, on a rank of a partitioned world.
        ``GradJune.forward`` calls it BEFORE the hot path, which decides whether the step is differentiable from
        ``susceptibility.requires_grad``.  Without a ``Vaccination`` policy: nothing."""
        vp = self.vaccination_policies
        if vp is None or len(vp.policies) == 0:
            return
        vp.apply(data, timer, seed, agent_offset=agent_offset, all_reduce=all_reduce)
