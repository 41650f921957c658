"""One simulated timestep (reference grad_june/model.py:18-144).

``GradJune.forward(data, timer) -> data`` keeps the reference's contract; rows a1-a9 in the middle
of it (model.py:125-138) run as the fused ``gj_step`` launch sequence on the HIP device, updating
``data["agent"].{transmission, susceptibility, is_infected, infection_time}`` in place.
"""
from __future__ import annotations

import math

import torch
import yaml

from .immunity import Immunity
from .infection import IsInfectedSampler
from .infection_networks import InfectionNetworks
from .policies import Policies
from .symptoms import SymptomsUpdater
from .transmission import TransmissionUpdater, profile_inputs, profile_requires_grad
from .world import agent_buffers, engine_for, require_hip


class GradJune(torch.nn.Module):
    def __init__(self, symptoms_updater=None, policies=None, infection_networks=None, device="cuda:0", immunity=None):
        super().__init__()
        self.symptoms_updater = symptoms_updater if symptoms_updater is not None else SymptomsUpdater.from_file()
        self.policies = policies if policies is not None else Policies.from_file()
        self.infection_networks = (infection_networks if infection_networks is not None
                                   else InfectionNetworks.from_file())
        self.immunity = immunity    # immunity.Immunity, or None: nothing wanes, nothing is launched
        self.transmission_updater = TransmissionUpdater()
        self.is_infected_sampler = IsInfectedSampler()
        self.device = device
        self.rng_seed = None        # Philox key; defaults to torch.initial_seed() at first use
        self.n_steps = 0            # Philox stream id: one stream per forward() call
        self.step_stats = None      # see forward()
        self.location_stats = None  # see forward()
        self.infector_stats = None  # see forward()
        self.tree_stats = None      # see forward()
        self.immunity_stats = None  # see forward()

    @classmethod
    def from_file(cls, fpath=None):
        if fpath is None:
            from .defaults import default_parameters

            return cls.from_parameters(default_parameters())
        with open(fpath) as f:
            return cls.from_parameters(yaml.safe_load(f))

    @classmethod
    def from_parameters(cls, params):
        return cls(
            symptoms_updater=SymptomsUpdater.from_parameters(params),
            policies=Policies.from_parameters(params),
            infection_networks=InfectionNetworks.from_parameters(params),
            device=params["system"]["device"],
            immunity=Immunity.from_parameters(params),
        )

    def infect_people(self, data, timer, new_infected):
        from .infection import infect_people

        infect_people(data, timer, new_infected)

    def hot_path(self, data, timer, exp_noise=None, want_probs=False):
        """Rows a1-a9.  Returns (new_infected, not_infected_probs or None)."""
        device = require_hip(self.device)
        active = self.infection_networks.active_networks(timer, self.policies)
        differentiable = torch.is_grad_enabled() and (
            any(isinstance(n.log_beta, torch.Tensor) and n.log_beta.requires_grad for n in active)
            or any(data["agent"][k].requires_grad for k in ("susceptibility", "is_infected", "infection_time"))
            or profile_requires_grad(data))
        self.policies.apply(timer=timer, data=data)
        engine = self._engine(data, device)
        for n in active:
            if n.name not in engine.plan.networks:
                raise KeyError(f"network '{n.name}': edge set 'attends_{n.edge_set}' is not in the world")
        has_q = bool(self.policies.quarantine_policies)
        if self.rng_seed is None:
            self.rng_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        step = self.n_steps
        self.n_steps += 1
        betas = self._betas(engine, active, timer)
        # testing: decisions, reports and - for a policy that isolates - the mask, on the stage the step starts from
        # (without a Testing policy nothing is launched); a ContactQuarantine active in the step overrides the mask
        testing = getattr(self.policies, "testing_policies", None)
        if testing is not None and len(testing.policies):
            agent_offset, all_reduce = self._vaccination_env()
            self.policies.test(data, timer, seed=self.rng_seed, agent_offset=agent_offset, all_reduce=all_reduce)
        # contact quarantine: mark, then mask, on the stage the step starts from; the step then takes the mask in the
        # place of the stage (None while no ContactQuarantine is active: nothing launched, the threshold path as it was)
        if has_q:
            isolating = self._qstate()
            self._contact_quarantine(data, timer, engine)
            if isolating is not None and self._qstate() is None:
                self.policies.quarantine_policies.qstate = isolating
        where = self._launch_env(engine, timer, active, betas, has_q, step)
        exp_noise = self._exp_noise(engine, exp_noise)
        # infection-location series: what forward() launches gj_location_stats with after the step (s0 and stage are
        # filled in by the path taken)
        # ... and gj_infector_scatter / gj_infector_gather, and gj_infection_tree: the three series share one record (and
        # one clone of s0)
        wanted = any(getattr(self, sink, None) is not None for sink in ("location_stats", "infector_stats", "tree_stats"))
        self._location_step = (None if not wanted else
                               {"engine": engine, "params": where["params"], "active": [n.name for n in active],
                                "seed": self.rng_seed, "step": step})
        if differentiable:
            return self._hot_path_differentiable(data, engine, where, active, betas, has_q, exp_noise, want_probs)
        return self._hot_path_in_place(data, engine, where, has_q, exp_noise, want_probs)

    # what a partitioned world does differently (distributed_api.DistributedGradJune), one method each ----------------
    def _engine(self, data, device):
        return engine_for(data, [n.spec() for n in self.infection_networks.networks.values()], device)

    def _betas(self, engine, active, timer):
        return {n.name: n.beta_value(self.policies, timer) for n in active}

    def _contact_quarantine(self, data, timer, engine):
        """``QuarantinePolicies.contact_step`` on this step's plan: it leaves the mask of the active ``ContactQuarantine``
        in ``quarantine_policies.qstate`` (None without one), where ``_launch_env`` and the two paths below read it."""
        qp = self.policies.quarantine_policies
        if getattr(qp, "contact_policies", None):
            plan = engine.plan
            qp.contact_step(plan, timer, self.rng_seed, edges=lambda: {
                s: data["attends_" + s].edge_index for s in plan.host.set_index if "attends_" + s in data})

    def _qstate(self):
        return getattr(self.policies.quarantine_policies, "qstate", None)

    def _launch_env(self, engine, timer, active, betas, has_q, step):
        """Where the step runs and with which launch parameters, as ``autograd.HotPathStep`` takes it in its ``env``."""
        qp = self.policies.quarantine_policies
        return {"engine": engine, "params": engine.params(
            now=timer.now, delta_time=timer.duration, day_type=0 if timer.day_type == "weekday" else 1,
            active=[n.name for n in active], betas=betas, has_quarantine=has_q,
            q_threshold=getattr(qp, "launch_threshold", qp.threshold) if has_q else math.inf, seed=self.rng_seed,
            step=step)}

    def _exp_noise(self, engine, exp_noise):
        if exp_noise is None:
            return None
        return exp_noise.to(device=engine.plan.device, dtype=torch.float32).contiguous()

    def _hot_path_in_place(self, data, engine, where, has_q, exp_noise, want_probs):
        """The step that updates ``data["agent"]``'s state tensors in place (nothing requires a gradient)."""
        bufs = agent_buffers(engine, data, need_params=True, need_stage=has_q, stage=self._qstate())
        n, device = engine.plan.host.n_agents, engine.plan.device
        new_infected = torch.empty(n, dtype=torch.float32, device=device)
        probs = torch.empty(n, dtype=torch.float32, device=device) if want_probs else None
        if self._location_step is not None:      # the step overwrites the susceptibility: keep what it started from
            self._location_step.update(s0=bufs.tensors["susceptibility"].clone(), stage=bufs.tensors["current_stage"])
        engine.step(bufs, where["params"],
                    engine.io(not_infected_probs=probs, new_infected=new_infected, exp_noise=exp_noise))
        if self._location_step is not None:
            self._location_step["transmission"] = bufs.tensors["transmission"]
        return new_infected, probs

    def _hot_path_differentiable(self, data, engine, where, active, betas, has_q, exp_noise, want_probs):
        """Row f3: the step as an autograd node (grad_june_amd.autograd.HotPathStep)."""
        from .autograd import HotPathStep

        if want_probs:
            raise NotImplementedError("want_probs is not available in differentiable mode")
        dev = engine.plan.device
        ag = data["agent"]
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        ip = ag["infection_parameters"]
        fixed = {k: f(ip[k]) for k in ("max_infectiousness", "shape", "rate", "shift")}
        # (the mask of a ContactQuarantine too is copied: the policy rewrites its buffer in the next step)
        stage = (self._qstate() if self._qstate() is not None else f(ag["symptoms"]["current_stage"])).clone() if has_q else None
        env = dict(where, fixed=fixed, stage=stage, exp_noise=exp_noise, nets=list(active), betas=betas)
        if getattr(self, "infector_stats", None) is not None or getattr(self, "tree_stats", None) is not None:
            # the node leaves its transmission array here
            env["keep_transmission"] = self._location_step
        state = [ag[k] if ag[k].dtype == torch.float32 else ag[k].to(torch.float32) for k in
                 ("susceptibility", "is_infected", "infection_time")]
        if self._location_step is not None:      # the node returns new tensors: the incoming one stays as it is
            self._location_step.update(s0=f(state[0]), stage=stage)
        susc, inf, time, new_infected = HotPathStep.apply(env, *state, *[n_.log_beta for n_ in active],
                                                          *profile_inputs(ip))
        ag.susceptibility, ag.is_infected, ag.infection_time = susc, inf, time
        return new_infected, None

    @staticmethod
    def location_edges(data, plan, held="_location_rows"):
        """What ``DevicePlan.location_rows`` builds the by-agent rows from - the world's COO edge lists, in the agent
        order in use - or None once the plan holds them (built once, kept with the plan)."""
        if getattr(plan, held, None) is not None:
            return None
        return {s: data["attends_" + s].edge_index for s in plan.host.set_index if "attends_" + s in data}

    @staticmethod
    def venue_edges(data, plan):
        """``location_edges`` for ``DevicePlan.venue_rows``: the COO edge lists, or None once the plan holds the rows."""
        return GradJune.location_edges(data, plan, held="_venue_rows")

    def _record_attribution(self, data, new_infected):
        """The step just run, attributed for the sinks the Runner set for its time loop (like ``step_stats``; without one
        nothing is cloned and nothing is launched), from detached tensors, so the series carry no gradient.
        ``location_stats``: gj_location_stats for every ``groups.LocationStats`` (the plan's ``cum`` workspaces still
        hold the step's sums); ``infector_stats``: gj_infector_scatter and gj_infector_gather for the
        ``groups.InfectorStats``, with the step's own transmissions; ``tree_stats``: gj_infection_tree for the
        ``groups.InfectionTree``, with the step's own Philox key and stream too."""
        locations, infectors, tree = self.location_stats, self.infector_stats, self.tree_stats
        if locations is None and infectors is None and tree is None:
            return
        step = self._location_step
        plan = step["engine"].plan
        nu = new_infected.detach().to(device=plan.device, dtype=torch.float32).contiguous()
        edges = self.location_edges(data, plan)
        record = (plan, step["params"], nu, step["s0"], step["stage"])
        if locations is not None:
            for stats in locations["stats"]:
                stats.add(*record, active=step["active"], background="background", row=locations["row"], edges=edges)
        if infectors is not None:
            infectors["stats"].record(*record, step["transmission"].detach(), row=infectors["row"], edges=edges)
        if tree is not None:
            tree["stats"].record(*record, step["transmission"].detach(), active=step["active"], background="background",
                                 row=tree["row"], edges=edges or self.venue_edges(data, plan), seed=step["seed"],
                                 step=step["step"])

    def _vaccination_env(self):
        """(global id of local agent 0, sum over the ranks of the efficacy's gradient or None): a rank of a partitioned
        world overrides it (distributed_api.DistributedGradJune)."""
        return 0, None

    def forward(self, data, timer, exp_noise=None):
        # vaccination first: it moves the susceptibility the step starts from, and hot_path decides whether the step is
        # differentiable from susceptibility.requires_grad before it applies the other policies.  The first call of a
        # Runner's time loop comes after next(timer): agents a campaign already covers at the initial date are
        # vaccinated in that first step, after the seeding.  Without a Vaccination policy nothing is launched
        campaigns = getattr(self.policies, "vaccination_policies", None)
        if campaigns is not None and len(campaigns.policies):
            if self.rng_seed is None:
                self.rng_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
            agent_offset, all_reduce = self._vaccination_env()
            self.policies.vaccinate(data, timer, seed=self.rng_seed, agent_offset=agent_offset, all_reduce=all_reduce)
        new_infected, _ = self.hot_path(data, timer, exp_noise=exp_noise)
        # location_stats, infector_stats, tree_stats: the step's new infections are attributed to the networks, to the
        # infectors and to one sampled infector BEFORE the symptoms update, while current_stage is still the stage the
        # quarantine mask was formed from
        self._record_attribution(data, new_infected)
        # waning immunity: after the records above (they read the step's own outcome) and before the symptoms update,
        # so the stage is still the one the step started from.  immunity_stats: set by the Runner for its time loop -
        # the launch's optional outputs.  Without an Immunity nothing is launched
        immunity = getattr(self, "immunity", None)
        if immunity is not None:
            sink = getattr(self, "immunity_stats", None) or {}
            immunity.step(data, timer.duration, new_infected, reinfected_out=sink.get("reinfected"),
                          count_out=sink.get("count"), susc_sum_out=sink.get("susc_sum"),
                          all_reduce=self._vaccination_env()[1])
        # in grad mode new_infected stays on the graph: the symptoms update is then an autograd node too
        # (autograd.SymptomsStep), which is what makes the deaths series differentiable (runner.py:198-215)
        # step_stats: set by the Runner for the duration of its time loop - the per-step result reductions
        # (runner.py:167-171) then ride on the symptoms pass instead of re-reading the arrays it just wrote
        self.symptoms_updater(data=data, timer=timer, new_infected=new_infected,
                              stats=getattr(self, "step_stats", None))
        return data
