"""Experiment driver (reference grad_june/runner.py:15-242): builds model + world + timer from the
YAML schema, seeds infections, runs the time loop and collects the result series.

Same public surface as the reference's ``Runner``.  Per-step state lives on the HIP device; the
hot path of each step is ``GradJune.hot_path`` (HIP kernels).  The per-step result reductions
(cases, cases by age, deaths) are small device reductions written into preallocated series
 instead of the reference's growing hstack/vstack chains.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import yaml

from .graph import HeteroData, ToUndirected, load_world
from .infection import infect_fraction_of_people
from .model import GradJune
from .timer import Timer
from .transmission import TransmissionSampler, profile_requires_grad
from .utils import read_path
from .world import require_hip

EDGE_SETS = ("household", "company", "school", "university", "care_home", "leisure")


def world_from_npz(path) -> HeteroData:
    """Neutral-array world (tests/golden/make_golden.py layout) -> the reference's graph format."""
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    data = HeteroData()
    ag = data["agent"]
    n = int(arrays["n_agents"])
    ag.id = torch.from_numpy(arrays.get("agent/id", np.arange(n)))
    ag.age = torch.from_numpy(arrays["age"])
    ag.sex = torch.from_numpy(arrays["sex"])
    for key in ("ethnicity", "area"):
        if "agent/" + key in arrays:
            ag[key] = arrays["agent/" + key]
    for s in EDGE_SETS:
        if f"es/{s}/agent" not in arrays:
            continue
        data[s].id = torch.from_numpy(arrays.get(f"venue_id/{s}", np.arange(len(arrays[f"es/{s}/people"]))))
        data[s].people = torch.from_numpy(arrays[f"es/{s}/people"])
        data["agent", "attends_" + s, s].edge_index = torch.from_numpy(
            np.vstack((arrays[f"es/{s}/agent"], arrays[f"es/{s}/venue"])))
    return ToUndirected()(data)


class Runner(torch.nn.Module):
    def __init__(self, model, data, timer, log_fraction_initial_cases, save_path, parameters,
                 age_bins=(0, 18, 65, 100), groups=None, seed_group=None, stages=None, locations=None, infectors=None,
                 matrices=None, tree=None):
        super().__init__()
        from .groups import (attach_groups, infection_tree_to_save, infectors_to_save, location_keys, locations_to_save,
                             stages_to_save)

        self._refuse_unpartitionable({"locations_to_save": locations, "infectors_to_save": infectors,
                                      "infection_matrices_to_save": matrices, "infection_tree_to_save": tree})
        self.model = model
        self.data = data
        self.data_backup = self.backup_infection_data(data)
        self.timer = timer
        self.log_fraction_initial_cases = log_fraction_initial_cases
        self.device = model.device
        self.age_bins = torch.tensor(age_bins, device=self.device)
        eth = data["agent"].get("ethnicity", None)
        self.ethnicities = np.sort(np.unique(eth)) if eth is not None else np.zeros(0)
        self.n_agents = data["agent"].id.shape[0]
        self.population_by_age = self.get_people_by_age()
        self.save_path = Path(save_path)
        self.input_parameters = parameters
        # result series by agent group (not in the reference): ``groups`` = attribute names of data["agent"] or a dict
        # name -> integer labels in the order of data["agent"]; the YAML key ``groups_to_save`` is encoded by get_data
        if groups is not None:
            attach_groups(data["agent"], groups)
        self.group_keys = {k: np.asarray(v) for k, v in (data["agent"].get("group_keys", None) or {}).items()}
        self._group_stats = None
        # seeding by agent group (not in the reference): ``seed_group`` names a labelling of ``group_keys``;
        # ``log_fraction_initial_cases`` is then a tensor [G] in the order of ``group_keys[seed_group]``
        if seed_group is not None and seed_group not in self.group_keys:
            raise ValueError(f"seed_group '{seed_group}': no such labelling (present: {sorted(self.group_keys)})")
        self.seed_group = seed_group
        self._seed_plan = None
        # symptom-stage series (not in the reference): ``stages`` = names of ``symptoms.stages`` or "all" (the YAML key
        # ``stages_to_save``): the occupancy of each stage and the entries into it, nationally and by every labelling
        self.stage_names = [str(s) for s in model.symptoms_updater.symptoms_sampler.stages] if stages else []
        self.stages_saved = stages_to_save(stages, self.stage_names)
        self._stage_stats = None
        # infection-location series (not in the reference): ``locations=True`` (the YAML key ``locations_to_save``):
        # each step's new infections attributed to the networks they came through, nationally and by every labelling
        self.locations_saved = locations_to_save(locations)
        self.location_keys = location_keys(model.infection_networks.networks) if self.locations_saved else []
        self._location_stats = None
        # infector series (not in the reference): ``infectors=True`` (the YAML key ``infectors_to_save``): each step's new
        # infections attributed to the agents who transmitted - infections caused per step, nationally and by every
        # labelling of the INFECTOR, per agent over the run, and the case reproduction number by cohort
        self.infectors_saved = infectors_to_save(infectors)
        self._infector_stats = None
        # who-infects-whom matrices (not in the reference): ``matrices=[name, ...]`` (the YAML key
        # ``infection_matrices_to_save``): for each of these labellings the infector series by PAIRS of groups - a step's
        # infections caused by group g in group g' - and the unattributed infections by the infected agent's group
        self.matrices_saved = self._check_matrices(matrices)
        # transmission tree (not in the reference): ``tree=True`` (the YAML key ``infection_tree_to_save``): ONE sampled
        # infector per infection - who infected whom, through which location and venue, and in which row - with the
        # exact counts by location and the mean generation interval per row
        self.tree_saved = infection_tree_to_save(tree)
        if self.tree_saved and not self.location_keys:
            self.location_keys = location_keys(model.infection_networks.networks)
        self._tree_stats = None
        self.restore_initial_data()

    _supports_locations = True

    @classmethod
    def _refuse_unpartitionable(cls, specs):
        """``specs``: {YAML key: value} (the parameters themselves will do).  The series a partitioned run cannot form."""
        from . import groups

        for key, parse, message in (
                ("locations_to_save", groups.locations_to_save,
                 "locations_to_save: the infection-location series is not available in a partitioned run"),
                ("infectors_to_save", groups.infectors_to_save,      # a halo infector's credit belongs to another rank
                 "infectors_to_save: the infector series is not available in a partitioned run"),
                ("infection_matrices_to_save", groups.infection_matrices_to_save,      # sums of the infector series' terms
                 "infection_matrices_to_save: the infection matrices are not available in a partitioned run"),
                ("infection_tree_to_save", groups.infection_tree_to_save,      # a venue's members live on other ranks
                 "infection_tree_to_save: the transmission tree is not available in a partitioned run")):
            if parse(specs.get(key)) and not cls._supports_locations:
                raise NotImplementedError(message)

    def _check_matrices(self, spec):
        """The labellings that get an infection matrix: each a labelling with result series (``groups_to_save``) of at
        most GJ_MATRIX_MAX_GROUPS groups, and only next to the infector series."""
        from . import _native as N
        from .groups import infection_matrices_to_save

        names = infection_matrices_to_save(spec)
        if names and not self.infectors_saved:
            raise ValueError("infection_matrices_to_save needs infectors_to_save: true (the matrices are the infector "
                             "series by pairs of groups)")
        skip = self.data["agent"].get("groups_without_series", None) or []
        for name in names:
            if name not in self.group_keys or name in skip:
                raise ValueError(f"infection_matrices_to_save: '{name}' is no labelling of groups_to_save (present: "
                                 f"{sorted(k for k in self.group_keys if k not in skip)})")
            if len(self.group_keys[name]) > N.GJ_MATRIX_MAX_GROUPS:
                raise ValueError(f"infection_matrices_to_save: '{name}' has {len(self.group_keys[name])} groups, a matrix "
                                 f"takes at most {N.GJ_MATRIX_MAX_GROUPS}; bin the attribute (groups_to_save: "
                                 f"[{{<name>: {{attribute: {name}, bins: [..]}}}}])")
        return names

    @classmethod
    def from_file(cls, fpath=None):
        if fpath is None:
            from .defaults import default_parameters

            return cls.from_parameters(default_parameters())
        with open(fpath) as f:
            return cls.from_parameters(yaml.safe_load(f))

    @classmethod
    def from_parameters(cls, params):
        data = cls.get_data(params)
        seed_group, log_fraction = cls.seed_parameters(params, data)
        return cls(
            model=GradJune.from_parameters(params),
            data=data,
            timer=Timer.from_parameters(params),
            log_fraction_initial_cases=log_fraction,
            save_path=params["save_path"],
            parameters=params,
            age_bins=params.get("age_bins_to_save", (0, 18, 65, 100)),
            seed_group=seed_group,
            stages=params.get("stages_to_save"),
            locations=params.get("locations_to_save"),
            infectors=params.get("infectors_to_save"),
            matrices=params.get("infection_matrices_to_save"),
            tree=params.get("infection_tree_to_save"),
        )

    @staticmethod
    def seed_parameters(params, data):
        """(labelling to seed by or None, log fraction(s)) from ``infection_seed`` (groups.seed_log_fractions): the
        reference's scalar as it is, or - with ``by`` - a float32 tensor with one value per group."""
        from .groups import seed_log_fractions

        by = params["infection_seed"].get("by")
        keys = (data["agent"].get("group_keys", None) or {}).get(by) if by is not None else None
        return seed_log_fractions(params["infection_seed"], keys)

    @staticmethod
    def get_data(params):
        device = require_hip(params["system"]["device"])
        path = read_path(params["data_path"])
        data = world_from_npz(path) if str(path).endswith(".npz") else load_world(path)
        # optional (not a reference key): ``system.locality_order: household`` renumbers the agents venue-major
        # at load time (graph.locality_order); the per-agent result of ``runner()`` is reported in the
        # file's original order
        # optional (not a reference key): ``groups_to_save: [area, ethnicity]`` asks for result series by agent group
        # (groups.py).  Encoded on the whole world in the file's order, before anything renumbers or cuts the agents
        if params.get("groups_to_save"):
            from .groups import attach_groups

            attach_groups(data["agent"], params["groups_to_save"])
        # optional (not a reference key): ``infection_seed.by: area`` seeds every group of that attribute with its own
        # fraction.  The same encoding, at the same place; a labelling that is only seeded by gets no result series
        seed_by = (params.get("infection_seed") or {}).get("by")
        if seed_by is not None and seed_by not in (data["agent"].get("group_keys", None) or {}):
            from .groups import attach_groups

            if not isinstance(seed_by, str) or seed_by not in data["agent"]:
                raise ValueError(f"infection_seed.by: the world's agents have no attribute '{seed_by}'")
            attach_groups(data["agent"], [seed_by])
            data["agent"].groups_without_series = [seed_by]
        by = params["system"].get("locality_order")
        if by:
            from .graph import locality_order

            data, original = locality_order(data, by=by)
            data["agent"].original_index = original
        data = data.to(device)
        n = len(data["agent"]["id"])
        values = TransmissionSampler.from_parameters(params)(n)
        ag = data["agent"]
        ag.infection_parameters = {"max_infectiousness": values[0].contiguous(), "shape": values[1].contiguous(),
                                   "rate": values[2].contiguous(), "shift": values[3].contiguous()}
        ag.transmission = torch.zeros(n, device=device)
        ag.susceptibility = torch.ones(n, device=device)
        ag.is_infected = torch.zeros(n, device=device)
        ag.infection_time = torch.zeros(n, device=device)
        ag.symptoms = {"current_stage": torch.ones(n, dtype=torch.long, device=device),
                       "next_stage": torch.ones(n, dtype=torch.long, device=device),
                       "time_to_next_stage": torch.zeros(n, device=device)}
        return data

    # in-memory checkpoint of the mutable state ---------------------------------------------------
    _STATE = ("susceptibility", "is_infected", "infection_time", "transmission")
    _SYMPTOMS = ("current_stage", "next_stage", "time_to_next_stage")

    def backup_infection_data(self, data):
        ag = data["agent"]
        ret = {k: ag[k].detach().clone() for k in self._STATE}
        ret["symptoms"] = {k: ag["symptoms"][k].detach().clone() for k in self._SYMPTOMS}
        return ret

    def restore_initial_data(self):
        ag = self.data["agent"]
        for k in self._STATE:
            ag[k] = self.data_backup[k].detach().clone()
        for k in self._SYMPTOMS:
            ag.symptoms[k] = self.data_backup["symptoms"][k].detach().clone()
        self.data["results"] = {"deaths_per_timestep": None}

    def _seed_requires_grad(self) -> bool:
        lf = self.log_fraction_initial_cases
        return torch.is_grad_enabled() and isinstance(lf, torch.Tensor) and lf.requires_grad

    def _seed_labels(self):
        """(int32 labels on the device, groups.SeedPlan) of the labelling the seed goes by; built once."""
        if self._seed_plan is None:
            from .groups import SeedPlan

            labels = self.data["agent"]["group_labels"][self.seed_group]
            self._seed_plan = SeedPlan(labels, len(self.group_keys[self.seed_group]), device=require_hip(self.device))
        return self._seed_plan.labels, self._seed_plan

    def _seed_all_reduce(self):
        """Hook: a partitioned run sums the seed's [G] gradient over the ranks (distributed_api.DistributedRunner)."""
        return None

    def set_initial_cases(self):
        lf = self.log_fraction_initial_cases
        if self.seed_group is None and not self._seed_requires_grad():      # the reference's path: one national value
            new_infected = infect_fraction_of_people(
                data=self.data, timer=self.timer, symptoms_updater=self.model.symptoms_updater,
                device=self.device, fraction=10.0 ** lf, agent_offset=getattr(self, "agent_offset", 0))
        else:
            from .infection import infect_fraction_by_group

            lf = lf if isinstance(lf, torch.Tensor) else torch.as_tensor(lf, dtype=torch.float64)
            labels, plan = (None, None) if self.seed_group is None else self._seed_labels()
            n_groups = 1 if self.seed_group is None else plan.n_groups
            if lf.numel() != n_groups or lf.dim() > 1:
                raise ValueError(f"log_fraction_initial_cases: shape {tuple(lf.shape)}, expected "
                                 + ("a scalar" if self.seed_group is None else f"[{n_groups}] (group_keys['{self.seed_group}'])"))
            if self._seed_requires_grad():
                fractions = (10.0 ** lf).reshape(n_groups)           # in torch: the chain rule to the log is autograd's
            else:      # as the scalar path forms it: 10.0 ** x in Python doubles, whatever the tensor's precision
                fractions = torch.tensor([10.0 ** v for v in lf.detach().reshape(-1).tolist()], dtype=torch.float64)
            new_infected = infect_fraction_by_group(
                data=self.data, timer=self.timer, symptoms_updater=self.model.symptoms_updater,
                fractions=fractions, labels=labels, device=self.device,
                agent_offset=getattr(self, "agent_offset", 0), plan=plan, all_reduce=self._seed_all_reduce())
        if self.locations_saved or self.infectors_saved or self.tree_saved:      # row 0 of these series
            self._seed_new_infected = new_infected.detach()
        self.model.symptoms_updater(data=self.data, timer=self.timer, new_infected=new_infected)

    # per-step result reductions: one fused pass (gj_step_stats) into a preallocated series ------------
    def _stats_args(self, data):
        """(agent classes, age-bin edges as a C array, dead stage) of gj_step_stats / gj_symptoms_step_stats."""
        import ctypes as C

        ag = data["agent"]
        if getattr(self, "_cls", None) is None:
            dev = require_hip(self.device)
            sex = ag["sex"] if "sex" in ag else torch.zeros_like(ag.age)
            self._cls = (sex.long() * 100 + ag.age.long()).to(device=dev, dtype=torch.uint8).contiguous()
            self._edges = (C.c_int32 * (len(self.age_bins)))(*[int(b) for b in self.age_bins.cpu()])
        return self._cls, self._edges, int(self.model.symptoms_updater.stages_ids[-1])

    def _record(self, data, row):
        from . import _native as N

        ag = data["agent"]
        n = self.n_agents
        cls, edges, dead = self._stats_args(data)
        stage = ag.symptoms["current_stage"]
        if stage.dtype != torch.float32:
            stage = stage.to(torch.float32)
        inf = ag.is_infected
        if inf.dtype != torch.float32 or not inf.is_contiguous():
            inf = inf.to(torch.float32).contiguous()
        N.check(N.load().gj_step_stats(n, N.ptr(cls), N.ptr(inf), N.ptr(stage.contiguous()),
                                       len(self.age_bins) - 1, edges, dead, N.ptr(self._series[row]),
                                       N.current_stream()), "gj_step_stats")

    # per-step result reductions by agent group: one gj_group_stats pass per labelling ----------------------------
    def _groups(self):
        """{name: groups.GroupStats} of the labellings asked for (empty: nothing is recorded, nothing is launched)."""
        if self._group_stats is None:
            from .groups import GroupStats

            labels = self.data["agent"].get("group_labels", None) or {}
            dev = require_hip(self.device) if labels else None
            skip = self.data["agent"].get("groups_without_series", None) or []
            self._group_stats = {name: GroupStats(labels[name], len(self.group_keys[name]), device=dev)
                                 for name in self.group_keys if name not in skip}
        return self._group_stats

    def _series_by_group(self, n_rows):
        """{name: float64 [n_rows, 2 G]} zeros, one per labelling: the rows of gj_group_stats (cases, then deaths).  Sums
        over this rank's agents (``_summed``)."""
        series = {name: torch.zeros(n_rows, 2 * st.n_groups, dtype=torch.float64, device=require_hip(self.device))
                  for name, st in self._groups().items()}
        self._summed += series.values()
        return series

    def _add_mask(self, series, row, mask):
        """A 0 / 1 mask per agent (a launch's newly vaccinated, newly confirmed, reinfected) counted by every labelling into
        ``row`` of a ``_series_by_group``: the cases half of gj_group_stats' output (no stage equals the ``dead`` given, so
        the other half stays zero)."""
        for name, stats in self._groups().items():
            stats.add(mask, mask, 2, series[name][row])

    def _record_groups(self, data, row, diff_rows=None):
        ag = data["agent"]
        dead = int(self.model.symptoms_updater.stages_ids[-1])
        stage, inf = ag.symptoms["current_stage"], ag.is_infected
        if diff_rows is not None:                 # differentiable run: the rows stay on the autograd graph
            from .autograd import GroupSeriesRow

            for name, stats in self._groups().items():
                diff_rows[name].append(torch.cat(GroupSeriesRow.apply({"stats": stats, "dead": dead}, inf, stage)))
            return
        stage = stage.detach().to(torch.float32).contiguous()
        inf = inf.detach().to(torch.float32).contiguous()
        for name, stats in self._groups().items():
            stats.add(inf, stage, dead, self._group_series[name][row])

    # per-step symptom-stage series: one gj_stage_stats pass for the nation and one per labelling ------------------
    def _stages(self):
        """{None or labelling name: groups.StageStats} (empty without ``stages_to_save``: nothing is allocated or launched)."""
        if self._stage_stats is None:
            self._stage_stats = {}
            if self.stages_saved:
                from .groups import StageStats

                dev, S = require_hip(self.device), len(self.stage_names)
                self._stage_stats[None] = StageStats(None, 1, S, device=dev)
                for name, st in self._groups().items():
                    self._stage_stats[name] = StageStats(st.labels, st.n_groups, S, device=dev)
        return self._stage_stats

    def _record_stages(self, data, row, diff_rows=None):
        stage = data["agent"].symptoms["current_stage"]
        if diff_rows is not None:                 # differentiable run: the rows stay on the autograd graph
            from .autograd import StageSeriesRow

            for key, stats in self._stages().items():
                diff_rows[key].append(torch.stack(StageSeriesRow.apply({"stats": stats, "prev": self._stage_prev}, stage)))
            # the next row's previous stage: a stage on the graph is a fresh tensor of its step (SymptomsStep) that
            # nothing updates in place - it is kept as it is; one that is updated in place is copied
            self._stage_prev = stage.detach() if stage.requires_grad else stage.detach().to(torch.float32, copy=True)
            return
        cur = stage.detach().to(torch.float32).contiguous()
        for key, stats in self._stages().items():
            stats.add(cur, self._stage_prev, self._stage_series[key][row])
        self._stage_prev.copy_(cur)

    # per-step infection-location series: one gj_location_stats pass for the nation and one per labelling -----------
    def _locations(self):
        """{None or labelling name: groups.LocationStats} (empty without ``locations_to_save``: nothing is allocated,
        cloned or launched)."""
        if self._location_stats is None:
            self._location_stats = {}
            if self.locations_saved:
                from .groups import LocationStats

                dev = require_hip(self.device)
                self._location_stats[None] = LocationStats(None, 1, self.location_keys, device=dev)
                for name, st in self._groups().items():
                    self._location_stats[name] = LocationStats(st.labels, st.n_groups, self.location_keys, device=dev)
        return self._location_stats

    def _record_seed_locations(self, locations, infectors=None, tree=None):
        """Row 0: the seeding step.  No network is active, so every seeded agent lands in the column ``seed``."""
        dev = require_hip(self.device)
        engine = self.model._engine(self.data, dev)
        params = engine.params(now=self.timer.now, delta_time=self.timer.duration, day_type=0, active=[], betas={})
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        nu, s0 = f(self._seed_new_infected), f(self.data_backup["susceptibility"])
        edges = self.model.location_edges(self.data, engine.plan)
        for stats in locations.values():
            stats.add(engine.plan, params, nu, s0, None, active=(), background="seed", row=0, edges=edges)
        if infectors is not None:      # nobody transmitted a seed: all unattributed; the seeds are the cohort of row 0
            infectors.clear(engine.plan)      # (U is zero between steps; a run that was interrupted may have left some)
            infectors.record(engine.plan, params, nu, s0, None, None, row=0, edges=edges)
        if tree is not None:      # nobody transmitted a seed: every seeded agent gets -2 and the column ``seed``
            tree.record(engine.plan, params, nu, s0, None, None, active=(), background="seed", row=0, edges=edges)
        self._seed_new_infected = None

    # per-step infector series: gj_infector_scatter once, gj_infector_gather for the nation and once per labelling -------
    def _infectors(self):
        """The run's ``groups.InfectorStats``, or None without ``infectors_to_save`` (nothing is allocated, cloned or
        launched)."""
        if self._infector_stats is None and self.infectors_saved:
            from .groups import InfectorStats

            self._infector_stats = InfectorStats(
                self.n_agents, {name: (st.labels, st.n_groups) for name, st in self._groups().items()},
                device=require_hip(self.device), matrices=self.matrices_saved)
        return self._infector_stats

    # transmission tree: one gj_infection_tree launch per step ---------------------------------------------------------------
    def _tree(self):
        """The run's ``groups.InfectionTree``, or None without ``infection_tree_to_save`` (nothing is allocated, cloned or
        launched)."""
        if self._tree_stats is None and self.tree_saved:
            from .groups import InfectionTree

            self._tree_stats = InfectionTree(self.n_agents, self.location_keys, device=require_hip(self.device))
        return self._tree_stats

    def _generation_interval(self, tree, dates):
        """float32 [T]: the mean, over the agents infected in row r with a sampled infector, of the days between the
        infector's row date and row r; NaN for a row without one.  Torch ops on the tree's arrays."""
        T, dev = len(dates), tree.device
        days = torch.tensor([(d - dates[0]).total_seconds() / 86400.0 for d in dates], dtype=torch.float64, device=dev)
        has = tree.infector >= 0
        row = tree.infected_row[has].long()
        parent_row = tree.infected_row[tree.infector[has].long()].long()
        sums = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, row, days[row] - days[parent_row])
        return (sums / torch.bincount(row, minlength=T).to(torch.float64)).to(torch.float32)

    # vaccination series: the launches' own counts, and one gj_group_stats pass per labelling on a launch's mask ----------
    def _campaigns(self):
        """The model's ``policies.VaccinationPolicies``, or None without a ``Vaccination`` policy (nothing is recorded)."""
        vp = getattr(self.model.policies, "vaccination_policies", None)
        return vp if vp is not None and len(vp.policies) else None

    def _immunity(self):
        """The model's ``immunity.Immunity``, or None without the ``immunity`` key (nothing is recorded)."""
        return getattr(self.model, "immunity", None)

    # contact-quarantine series: one gj_stage_stats pass on the step's mask for the nation and one per labelling ----------
    def _contact_quarantine(self):
        """The model's ``policies.QuarantinePolicies`` if it holds a ``ContactQuarantine``, else None (nothing is
        recorded, nothing is allocated)."""
        qp = getattr(self.model.policies, "quarantine_policies", None)
        return qp if getattr(qp, "contact_policies", None) else None

    def _quarantine_stats(self):
        """{None or labelling name: groups.StageStats} over the mask's values: three (0 free, 1 index case, 2 contact),
        and a fourth (3 isolating on a positive test) where a ``Testing`` policy isolates."""
        if getattr(self, "_q_stats", None) is None:
            from .groups import StageStats

            dev = require_hip(self.device)
            values = self._mask_values()
            self._q_stats = {None: StageStats(None, 1, values, device=dev)}
            for name, st in self._groups().items():
                self._q_stats[name] = StageStats(st.labels, st.n_groups, values, device=dev)
        return self._q_stats

    # testing series: the launches' own counts, one gj_group_stats pass per labelling on a launch's mask of the newly
    # confirmed, and - where a policy isolates - the fourth value of the mask in the contact quarantine's gj_stage_stats ----
    def _testing(self):
        """The model's ``policies.TestingPolicies``, or None without a ``Testing`` policy (nothing is recorded)."""
        tp = getattr(self.model.policies, "testing_policies", None)
        return tp if tp is not None and len(tp.policies) else None

    def _mask_values(self) -> int:
        tp = self._testing()
        return 4 if tp is not None and tp.isolating else 3

    def _masked(self) -> bool:
        """Whether the run has a quarantine-mask series: a ``ContactQuarantine``, or a ``Testing`` that isolates."""
        return self._contact_quarantine() is not None or self._mask_values() == 4

    def _record_quarantined(self, qstate, row):
        """The occupancy plane of gj_stage_stats on ``qstate``: exact int64 counts, so a by-group row sums to the national
        row exactly.  A step in which no ``ContactQuarantine`` is active (``qstate`` None) leaves its row zero."""
        if qstate is not None:
            for key, stats in self._quarantine_stats().items():
                stats.add(qstate, None, self._quarantine_series[key][row])

    # time loop --------------------------------------------------------------------------------------
    def forward(self):
        timer, model, data = self.timer, self.model, self.data
        timer.reset()
        if hasattr(model.policies, "reset"):      # what a run applied: the vaccination ramps and dose counts
            model.policies.reset()
        self.restore_initial_data()
        self.set_initial_cases()
        self._open_series(self._count_rows(), self._is_differentiable())
        self._record_row(data, 0)
        dates = [timer.date]
        row = 0
        while timer.date < timer.final_date:
            next(timer)
            row += 1
            sink = self._arm(row)
            try:
                data = model(data, timer)
            finally:
                step_rows = self._disarm()
            self._after_step(row, step_rows)
            self._record_row(data, row, done=bool(sink and sink.get("done")))
            dates.append(timer.date)
        T = row + 1
        self._finalize_series(T)
        results = {"dates": dates}
        self._results_national(results, T, data)
        self._results_groups(results, T)
        self._results_stages(results, T)
        self._results_locations(results, T)
        self._results_infectors(results, T, data)
        self._results_tree(results, T, data)
        self._results_vaccination(results, T)
        self._results_immunity(results, T)
        self._results_quarantine(results, T)
        self._results_testing(results, T, data)
        return results, self._in_file_order(data["agent"].is_infected)

    def _count_rows(self) -> int:
        """The rows of the run's series: the seeding's and one per step of a probe timer (4096 without the parameters)."""
        if not isinstance(self.input_parameters, dict):
            return 4096
        n_rows, probe = 1, Timer.from_parameters(self.input_parameters)
        while probe.date < probe.final_date:
            next(probe)
            n_rows += 1
        return n_rows

    def _is_differentiable(self) -> bool:
        """A differentiable run (a log_beta is an nn.Parameter, a profile tensor, the seed, a vaccination efficacy, an
        immunity or a testing parameter requires a gradient, grad mode on): the case series must stay on the autograd
        graph, so they are formed with tensor ops instead of the fused reduction kernel."""
        campaigns, immunity, testing = self._campaigns(), self._immunity(), self._testing()
        return torch.is_grad_enabled() and (any(
            isinstance(n.log_beta, torch.Tensor) and n.log_beta.requires_grad
            for n in self.model.infection_networks.networks.values()) or profile_requires_grad(self.data)
            or self._seed_requires_grad() or (campaigns is not None and campaigns.requires_grad())
            or (immunity is not None and immunity.requires_grad())
            or (testing is not None and testing.requires_grad()))

    def _in_file_order(self, t):
        """A per-agent array of the run in the order of the world's file (``system.locality_order`` renumbered the agents
        at load time)."""
        if "original_index" not in self.data["agent"]:
            return t
        out = torch.empty_like(t)
        out[self.data["agent"].original_index.to(t.device)] = t
        return out

    def _open_series(self, n_rows, differentiable):
        """Everything a run's series need before its first row: the allocations (``_summed``: those that are sums over
        this rank's agents, which a partitioned run adds over the ranks), the seeding's row of the attribution series and
        the susceptibility of row 0.  A differentiable run keeps the rows of its case, group, stage and confirmed series
        on the graph, in the ``_*_diff_rows`` lists."""
        dev = require_hip(self.device)
        self._differentiable = differentiable
        self._series = torch.zeros(n_rows, 1 + len(self.age_bins), dtype=torch.float64, device=dev)
        self._summed = [self._series]
        self._diff_rows = []
        groups = self._groups()
        self._group_series = self._series_by_group(n_rows)
        self._group_diff_rows = {name: [] for name in groups} if differentiable else None
        stages = self._stages()
        # (a differentiable run keeps its rows on the graph instead: no int64 series then)
        self._stage_series = {} if differentiable else {
            key: torch.zeros(n_rows, 2, st.n_groups, st.n_stages, dtype=torch.int64, device=st.device)
            for key, st in stages.items()}
        self._summed += self._stage_series.values()
        self._stage_diff_rows = {key: [] for key in stages} if differentiable else None
        if stages:      # row 0 counts its entries against the restored initial stage: the agents the seed moved
            self._stage_prev = self.data_backup["symptoms"]["current_stage"].detach().to(
                device=dev, dtype=torch.float32, copy=True).contiguous()

        locations, infectors, tree = self._locations(), self._infectors(), self._tree()
        for st in (*locations.values(), infectors, tree):
            if st is not None:
                st.reset(n_rows)
        if locations or infectors is not None or tree is not None:
            self._record_seed_locations(locations, infectors, tree)
        # vaccination series (not in the reference), whenever the model has a Vaccination policy: the doses given so far,
        # by campaign (the launches' own counts) and by every labelling (gj_group_stats on a launch's mask of the newly
        # vaccinated).  Integer counts, so a by-group row sums to the national row exactly; row 0 is zero; no gradient
        campaigns = self._campaigns()
        self._vaccine_series, self._vaccine_group_series = None, {}
        if campaigns is not None:
            if "campaign" in groups:
                raise ValueError("a labelling named 'campaign' would shadow the result key vaccine_doses_by_campaign")
            self._vaccine_series = torch.zeros(n_rows, len(campaigns.policies), dtype=torch.int64, device=dev)
            self._summed.append(self._vaccine_series)
            self._vaccine_group_series = self._series_by_group(n_rows)

        # testing series (not in the reference), whenever the model has a Testing policy: each step's newly confirmed
        # cases - the launches' own count, and by every labelling gj_group_stats on their 0 / 1 masks - and, where a
        # policy isolates, the agents the step's mask holds as isolating: the fourth value of the pass that counts the
        # contact quarantine's three.  Integer counts; row 0 is zero; a row lags the stage by one step (the launch of row
        # k sees the stages row k - 1 left).  In a differentiable run the national row stays on the graph
        self._confirmed_series, self._confirmed_group_series, self._confirmed_diff_rows = None, {}, []
        if self._testing() is not None:
            self._confirmed_series = torch.zeros(n_rows, 2, dtype=torch.int64, device=dev)      # confirmed, decisions
            self._summed.append(self._confirmed_series)
            self._confirmed_group_series = self._series_by_group(n_rows)
            self._confirmed_diff_rows.append(torch.zeros((), dtype=torch.float32, device=dev))
        # contact-quarantine series (not in the reference), whenever the model has a ContactQuarantine policy: the agents
        # the step's mask holds as index cases and as contacts, nationally and by every labelling.  Integer counts; row 0
        # and the rows of steps without an active ContactQuarantine are zero (a plain Quarantine is not counted); no
        # gradient.  (No sum over the ranks: a partitioned run refuses both policies that write the mask)
        self._quarantine_series = {}
        if self._masked():
            self._quarantine_series = {
                key: torch.zeros(n_rows, 2, st.n_groups, self._mask_values(), dtype=torch.int64, device=st.device)
                for key, st in self._quarantine_stats().items()}

        # waning-immunity series (not in the reference), whenever the model has an Immunity: each step's reinfections -
        # the launch's own count, and by every labelling gj_group_stats on its 0 / 1 mask - and the population's
        # susceptibility after the launch as an exact fixed-point sum.  Integer counts, so a by-group row sums to the
        # national row exactly; row 0 of the reinfections is zero, that of the susceptibility comes from one launch that
        # moves nobody; no gradient
        self._immunity_series, self._reinfection_group_series, self._reinfected = None, {}, None
        if self._immunity() is not None:
            self._immunity_series = torch.zeros(n_rows, 2, dtype=torch.int64, device=dev)      # reinfections, susc_sum
            self._summed.append(self._immunity_series)
            self._reinfection_group_series = self._series_by_group(n_rows)
            if groups:
                self._reinfected = torch.empty(self.n_agents, dtype=torch.float32, device=dev)
            self._immunity().measure(self.data, self._immunity_series[0, 1:2])

    def _record_row(self, data, row, done=False):
        """Row ``row`` of the case, group and stage series from the state as it stands (``done``: the step's symptoms
        update has filled the national row already)."""
        if not done:
            self._record(data, row)
        if self._groups():
            self._record_groups(data, row, self._group_diff_rows)
        if self._stages():
            self._record_stages(data, row, self._stage_diff_rows)
        if self._differentiable:
            ag = data["agent"]
            stage = ag.symptoms["current_stage"]
            dead = float(self.model.symptoms_updater.stages_ids[-1])
            deaths = ((stage == dead) * stage / dead).sum()          # store_differentiable_deaths' form
            self._diff_rows.append(torch.cat((ag.is_infected.sum().reshape(1), self.get_cases_by_age(data),
                                              deaths.reshape(1))))

    def _arm(self, row):
        """Before a step: where the model and the policies leave row ``row`` of the series they fill themselves.  Returns
        the sink of the national row (None in a differentiable run)."""
        model, groups = self.model, self._groups()
        locations, infectors, tree = self._locations(), self._infectors(), self._tree()
        campaigns, immunity, testing = self._campaigns(), self._immunity(), self._testing()
        sink = None
        if not self._differentiable:      # rows f1 + f2 in one pass: the model's symptoms update fills this step's row
            cls, edges, dead = self._stats_args(self.data)
            sink = {"cls": cls, "edges": edges, "n_bins": len(self.age_bins) - 1, "dead": dead, "out": self._series[row]}
        model.step_stats = sink
        if locations:
            model.location_stats = {"stats": list(locations.values()), "row": row}
        if infectors is not None:
            model.infector_stats = {"stats": infectors, "row": row}
        if tree is not None:
            model.tree_stats = {"stats": tree, "row": row}
        if campaigns is not None:      # cumulative: a row starts from the one before it
            for series in self._vaccine_group_series.values():
                series[row].copy_(series[row - 1])
            campaigns.on_newly = (lambda campaign, newly: self._add_mask(self._vaccine_group_series, row, newly)
                                  ) if groups else None
        if immunity is not None:
            model.immunity_stats = {"reinfected": self._reinfected, "count": self._immunity_series[row, 0:1],
                                    "susc_sum": self._immunity_series[row, 1:2]}
        if testing is not None:
            testing.sink = {"counts": self._confirmed_series[row], "rows": [], "on_newly": (
                lambda newly: self._add_mask(self._confirmed_group_series, row, newly)) if groups else None}
        return sink

    def _disarm(self):
        """After a step, whether it came back or raised: everything ``_arm`` set is None again.  Returns the rows the
        step's testing launches left on the graph (None without a Testing policy)."""
        model, campaigns, testing = self.model, self._campaigns(), self._testing()
        step_rows = None
        if testing is not None:
            step_rows, testing.sink = testing.sink["rows"], None
        model.immunity_stats = model.step_stats = model.location_stats = model.infector_stats = model.tree_stats = None
        if campaigns is not None:
            campaigns.on_newly = None
        return step_rows

    def _after_step(self, row, step_rows):
        """Row ``row`` of the series the runner reads off the step it just ran."""
        campaigns = self._campaigns()
        if campaigns is not None and campaigns.doses is not None:
            self._vaccine_series[row].copy_(campaigns.doses)
        if self._reinfected is not None:      # this step's mask, by group
            self._add_mask(self._reinfection_group_series, row, self._reinfected)
        if self._masked():      # the mask the step just ran with
            self._record_quarantined(getattr(self.model.policies.quarantine_policies, "qstate", None), row)
        if self._testing() is not None and self._differentiable:      # the launches' rows, on the graph
            on_graph = torch.stack(step_rows).sum() if step_rows else torch.zeros_like(self._confirmed_diff_rows[0])
            # (a launch that was no autograd node - nothing required a gradient yet - counts as a constant)
            self._confirmed_diff_rows.append(on_graph + (self._confirmed_series[row, 0].to(torch.float32) - on_graph.detach()))

    # the result keys, one family per method, in the order they enter ``results`` --------------------------------------
    def _results_national(self, results, T, data):
        n_bins = len(self.age_bins) - 1
        series = self._series[:T].to(torch.float32)
        if self._differentiable:
            series = self._reduce_differentiable(torch.stack(self._diff_rows).to(torch.float32))
        data["results"]["deaths_per_timestep"] = series[:, 1 + n_bins]
        results["cases_per_timestep"] = series[:, 0]
        results["daily_cases_per_timestep"] = torch.diff(series[:, 0], prepend=torch.tensor([0.0], device=self.device))
        results["deaths_per_timestep"] = data.results["deaths_per_timestep"]
        for i, key in enumerate(self.age_bins[1:]):
            results[f"cases_by_age_{int(key):02d}"] = series[:, 1 + i]

    def _results_groups(self, results, T):
        for name, st in self._groups().items():
            st.check(f"result series by {name}")
            by_group = self._group_series[name][:T].to(torch.float32)
            if self._differentiable:
                by_group = self._reduce_differentiable(torch.stack(self._group_diff_rows[name]).to(torch.float32))
            G = st.n_groups
            results[f"cases_by_{name}"] = by_group[:, :G]
            results[f"daily_cases_by_{name}"] = torch.diff(by_group[:, :G], dim=0,
                                                           prepend=torch.zeros(1, G, device=by_group.device))
            results[f"deaths_by_{name}"] = by_group[:, G:]

    def _results_stages(self, results, T):
        for key, st in self._stages().items():      # every stage was counted: the columns asked for are selected here
            st.check("symptom-stage series" + (f" by {key}" if key else ""))
            if self._differentiable:
                counts = self._reduce_differentiable(torch.stack(self._stage_diff_rows[key]))
            else:
                counts = self._stage_series[key][:T].to(torch.float32)      # [T, 2, G, S]
            for name in self.stages_saved:
                s = self.stage_names.index(name)
                tail = "per_timestep" if key is None else f"by_{key}"
                occupancy, entries = counts[:, 0, :, s], counts[:, 1, :, s]
                results[f"{name}_{tail}"] = occupancy[:, 0] if key is None else occupancy
                results[f"new_{name}_{tail}"] = entries[:, 0] if key is None else entries

    def _results_locations(self, results, T):
        for key, st in self._locations().items():      # out / 2^30 in fp64, then float32 like the other series; no gradient
            st.check("infection-location series" + (f" by {key}" if key else ""))
            values = st.values(T)
            if key is None:
                results["infections_by_location"] = values[:, 0, :]
            else:
                results[f"infections_by_location_by_{key}"] = values

    def _results_infectors(self, results, T, data):
        infectors = self._infectors()
        if infectors is not None:      # by the infector's group; R by the cohort's row (and group); no gradient
            infectors.check("infector series")
            results["infections_caused_per_timestep"] = infectors.values(None, T)[:, 0]
            results["infections_unattributed_per_timestep"] = infectors.unattributed[:T].to(torch.float64)      # counts: exact
            results["reproduction_number_per_timestep"] = infectors.reproduction(T)[:, 0]
            for name in self._groups():
                results[f"infections_caused_by_{name}"] = infectors.values(name, T)
                results[f"reproduction_number_by_{name}"] = infectors.reproduction(T, name)
            for name in self.matrices_saved:      # [t, infector's group, infected's group]; the counts are exact
                results[f"infection_matrix_by_{name}"] = infectors.matrix_values(name, T)
                results[f"infections_unattributed_by_{name}"] = infectors.unattributed_by[name][:T].to(torch.float64)
            data["agent"]["infections_caused"] = self._in_file_order(infectors.caused)
            data["agent"]["infected_row"] = self._in_file_order(infectors.infected_row)

    def _results_tree(self, results, T, data):
        tree = self._tree()
        if tree is not None:      # exact counts as float64; the per-agent arrays in the file's order; no gradient
            tree.check("transmission tree")
            results["infections_sampled_by_location"] = tree.counts[:T].to(torch.float64)
            results["infections_unresolved_per_timestep"] = tree.unresolved[:T].to(torch.float64)
            results["generation_interval_per_timestep"] = self._generation_interval(tree, results["dates"])
            per_agent = {"infector": tree.infector, "infection_location": tree.via, "infection_venue": tree.venue,
                         "infected_row": tree.infected_row, "offspring": tree.offspring()}
            if "original_index" in data["agent"]:      # the ids held in ``infector`` too: the file's numbering
                index = data["agent"].original_index.to(tree.device).long()
                per_agent["infector"] = torch.where(
                    tree.infector >= 0, index[tree.infector.clamp(min=0).long()].to(torch.int32), tree.infector)
            for key, values in per_agent.items():
                data["agent"][key] = self._in_file_order(values)

    def _results_vaccination(self, results, T):
        if self._campaigns() is not None:      # counts as float64: exact (float32 holds integers up to 2^24 only)
            by_campaign = self._vaccine_series[:T].to(torch.float64)
            results["vaccine_doses_per_timestep"] = by_campaign.sum(1)
            results["vaccine_doses_by_campaign"] = by_campaign
            for name, st in self._groups().items():
                results[f"vaccine_doses_by_{name}"] = self._vaccine_group_series[name][:T, : st.n_groups].clone()

    def _results_immunity(self, results, T):
        if self._immunity() is not None:      # counts as float64: exact; the susceptibility: sum / 2^30 in fp64, then float32
            counts = self._immunity_series[:T].t()
            results["reinfections_per_timestep"] = counts[0].to(torch.float64)
            results["susceptibility_per_timestep"] = (counts[1].to(torch.float64) / float(1 << 30)).to(torch.float32)
            for name, st in self._groups().items():
                results[f"reinfections_by_{name}"] = self._reinfection_group_series[name][:T, : st.n_groups].clone()

    def _results_quarantine(self, results, T):
        contact_quarantine, isolating = self._contact_quarantine(), self._mask_values() == 4
        if self._masked():      # int64 counts: [T] nationally, [T, G] by labelling
            if contact_quarantine is not None:
                contact_quarantine.check("contact quarantine")
            for key, st in self._quarantine_stats().items():
                st.check("quarantine-mask series" + (f" by {key}" if key else ""))
                counts = self._quarantine_series[key][:T, 0]      # the occupancy plane, [T, G, 3 or 4]
                tail = "per_timestep" if key is None else f"by_{key}"
                if contact_quarantine is not None:
                    results[f"quarantined_index_{tail}"] = counts[:, 0, 1] if key is None else counts[:, :, 1]
                    results[f"quarantined_contacts_{tail}"] = counts[:, 0, 2] if key is None else counts[:, :, 2]
                if isolating:
                    results[f"isolating_{tail}"] = counts[:, 0, 3] if key is None else counts[:, :, 3]

    def _results_testing(self, results, T, data):
        testing = self._testing()
        if testing is not None:      # int64 counts (a differentiable run: the national row as float32 on the graph)
            results["confirmed_cases_per_timestep"] = self._confirmed_series[:T, 0].clone()
            if self._differentiable and len(self._confirmed_diff_rows) == T:
                results["confirmed_cases_per_timestep"] = self._reduce_differentiable(torch.stack(self._confirmed_diff_rows))
            for name, st in self._groups().items():
                results[f"confirmed_cases_by_{name}"] = self._confirmed_group_series[name][:T, : st.n_groups].to(torch.int64)
            confirmed_time = testing.confirmed_time
            if confirmed_time is None:      # no policy ever started
                confirmed_time = torch.full((self.n_agents,), -1.0, dtype=torch.float32, device=require_hip(self.device))
            data["agent"]["confirmed_time"] = self._in_file_order(confirmed_time.clone())

    def _finalize_series(self, n_rows: int) -> None:
        """Hook: a partitioned run sums the ranks' per-step reductions here (distributed_api.DistributedRunner)."""

    def _reduce_differentiable(self, series: torch.Tensor) -> torch.Tensor:
        """Hook: the same for the series kept on the autograd graph in a differentiable run."""
        return series

    def _save_long(self, fname, dates, axes, cols):
        """A [T, ...] series as a long-format CSV: one line per date and per key of every axis of ``axes`` = {column:
        keys}, the last axis running fastest (the series' own row-major order), then ``cols`` = {column: flat values}."""
        import pandas as pd

        n = int(np.prod([len(keys) for keys in axes.values()]))
        frame, inner = {"date": np.repeat(np.asarray(dates, dtype=object), n)}, n
        for name, keys in axes.items():
            inner //= len(keys)
            frame[name] = np.tile(np.repeat(np.asarray(keys), inner), len(dates) * n // (len(keys) * inner))
        pd.DataFrame({**frame, **cols}).to_csv(self.save_path / fname, index=False)

    def save_results(self, results, is_infected):
        import pandas as pd

        flat = lambda key: results[key].detach().cpu().numpy().reshape(-1)
        dates = results["dates"]
        self.save_path.mkdir(exist_ok=True, parents=True)
        df = pd.DataFrame(index=results["dates"])
        df.index.name = "date"
        for key, series in results.items():
            if key != "dates" and series.dim() == 1:
                df[key] = series.detach().cpu().numpy()
        if "vaccine_doses_by_campaign" in results:      # [T, C]: one column per campaign, in the policies' order
            by_campaign = results["vaccine_doses_by_campaign"].detach().cpu().numpy()
            for c in range(by_campaign.shape[1]):
                df[f"vaccine_doses_campaign_{c}"] = by_campaign[:, c]
        df.to_csv(self.save_path / "results.csv")
        for name, keys in self.group_keys.items():      # [T, G] series: long format, one file per labelling
            if f"cases_by_{name}" not in results:       # a labelling that is only seeded by has no series
                continue
            saved = [c for st in self.stages_saved for c in (st, "new_" + st)]
            if f"vaccine_doses_by_{name}" in results:
                saved.append("vaccine_doses")
            if f"reinfections_by_{name}" in results:
                saved.append("reinfections")
            if f"quarantined_index_by_{name}" in results:
                saved += ["quarantined_index", "quarantined_contacts"]
            if f"confirmed_cases_by_{name}" in results:
                saved.append("confirmed_cases")
            if f"isolating_by_{name}" in results:
                saved.append("isolating")
            self._save_long(f"results_by_{name}.csv", dates, {name: keys},
                            {c: flat(f"{c}_by_{name}") for c in ("cases", "daily_cases", "deaths", *saved)})
        if "infections_by_location" in results:      # date, location, infections
            self._save_long("results_by_location.csv", dates, {"location": self.location_keys},
                            {"infections": flat("infections_by_location")})
            for name, keys in self.group_keys.items():
                if f"infections_by_location_by_{name}" in results:
                    self._save_long(f"results_by_location_by_{name}.csv", dates, {name: keys, "location": self.location_keys},
                                    {"infections": flat(f"infections_by_location_by_{name}")})
        if "infections_caused_per_timestep" in results:      # date, series, value
            series = ("infections_caused", "infections_unattributed", "reproduction_number")
            self._save_long("results_infectors.csv", dates, {"series": series}, {"value": np.stack(
                [results[f"{k}_per_timestep"].detach().cpu().numpy() for k in series], 1).reshape(-1)})
            for name, keys in self.group_keys.items():
                if f"infections_caused_by_{name}" not in results:
                    continue
                cols = {"infections_caused": flat(f"infections_caused_by_{name}"),
                        "reproduction_number": flat(f"reproduction_number_by_{name}")}
                if f"infections_unattributed_by_{name}" in results:      # (a labelling with an infection matrix)
                    cols["infections_unattributed"] = flat(f"infections_unattributed_by_{name}")
                self._save_long(f"results_infectors_by_{name}.csv", dates, {name: keys}, cols)
                if f"infection_matrix_by_{name}" in results:      # date, infector, infected, infections
                    self._save_long(f"results_infection_matrix_by_{name}.csv", dates, {"infector": keys, "infected": keys},
                                    {"infections": flat(f"infection_matrix_by_{name}")})
        if "infections_sampled_by_location" in results:      # one line per infected agent
            ag = self.data["agent"]
            row_of = ag["infected_row"].detach().cpu().numpy()
            infected = np.nonzero(row_of >= 0)[0]
            dates = np.asarray(results["dates"], dtype=object)
            pd.DataFrame({"infected": infected, "infector": ag["infector"].detach().cpu().numpy()[infected],
                          "date": dates[row_of[infected]],
                          "location": np.asarray(self.location_keys, dtype=object)[
                              ag["infection_location"].detach().cpu().numpy()[infected]],
                          "venue": ag["infection_venue"].detach().cpu().numpy()[infected]}
                         ).to_csv(self.save_path / "results_infection_tree.csv", index=False)
        if "confirmed_cases_per_timestep" in results:      # one line per confirmed agent
            import datetime

            when = self.data["agent"]["confirmed_time"].detach().cpu().numpy()
            agents = np.nonzero(when >= 0)[0]
            pd.DataFrame({"agent": agents,
                          "date": [results["dates"][0] + datetime.timedelta(days=float(t)) for t in when[agents]]}
                         ).to_csv(self.save_path / "results_confirmed.csv", index=False)
        pd.DataFrame({"is_infected": is_infected.detach().cpu().numpy()}).to_csv(
            self.save_path / "results_is_infected.csv")

    def store_differentiable_deaths(self, data):
        stage = data["agent"].symptoms["current_stage"]
        dead = int(self.model.symptoms_updater.stages_ids[-1])
        deaths = ((stage == dead) * stage / dead).sum()
        prev = data["results"]["deaths_per_timestep"]
        data["results"]["deaths_per_timestep"] = deaths if prev is None else torch.hstack((prev, deaths))

    def _age_masks(self, ages):
        lo, hi = self.age_bins[:-1], self.age_bins[1:]
        return (ages[None, :] > lo[:, None]) & (ages[None, :] < hi[:, None])     # [bins, A], open intervals

    def get_cases_by_age(self, data):
        return (self._age_masks(data["agent"].age) * data["agent"].is_infected[None, :]).sum(1)

    def get_people_by_age(self):
        counts = self._age_masks(self.data["agent"].age).sum(1)
        return {int(self.age_bins[i + 1].item()): counts[i] for i in range(len(counts))}

    def get_cases_by_ethnicity(self, data):
        ret = torch.zeros(len(self.ethnicities), device=self.device)
        for i, ethnicity in enumerate(self.ethnicities):
            mask = torch.tensor(self.data["agent"].ethnicity == ethnicity, device=self.device)
            ret[i] = (mask * data["agent"].is_infected).sum()
        return ret
