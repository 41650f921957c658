"""Result series by agent group (area, super area, ethnicity, sex, any integer label).

Also the host side of seeding by group: :class:`SeedPlan`, the tables ``gj_adjoint_seed`` reduces through, and
:func:`seed_log_fractions`, the ``infection_seed`` keys ``by`` / ``log_fraction_by_group`` of the YAML schema.

Host side: the label encoding (:func:`encode_groups`) and :class:`GroupStats`, the binding of ``gj_group_stats`` /
``gj_adjoint_group_stats`` (include/gradjune_hip.h, "row f2 by agent group") for one labelling of the agents.  The
reference has one such reduction, ``get_cases_by_ethnicity`` (grad_june/runner.py:235-242), which its time loop never
calls; here the Runner records ``cases_by_<name>`` / ``deaths_by_<name>`` at every step when asked to.
"""
from __future__ import annotations

import re
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _native as N

#: result keys of Runner.forward() that a group name must not shadow
_RESERVED = re.compile(r"age(_\d+)?")
#: stage names whose series <st>_per_timestep / <st>_by_<name> would shadow a result key of Runner.forward()
_STAGE_SHADOWS = ("cases", "daily_cases", "deaths")


class GroupLabelError(RuntimeError):
    """gj_group_stats met a label outside [0, n_groups) or a value it cannot sum (see the header)."""


def check_group_name(name) -> str:
    if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", name):
        raise ValueError(f"group name {name!r}: expected an identifier-like string")
    if _RESERVED.fullmatch(name):
        raise ValueError(f"group name '{name}' collides with the result keys cases_by_age_XX; "
                         "pass the age bins as a label dict under another name")
    return name


def _as_numpy(v) -> np.ndarray:
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def encode_groups(agent, spec) -> Tuple[Dict[str, torch.Tensor], Dict[str, list]]:
    """``spec``: a list of attribute names of ``agent`` (``data["agent"]``), or a dict ``name -> integer labels``
    (one per agent, in the order of ``agent``), or a list mixing names and such dicts.

    An attribute - strings or numbers - is encoded with ``np.unique(..., return_inverse=True)``: the columns are the
    sorted distinct values of the WHOLE world it is called on.  Integer labels of a dict are used as they are: they must
    lie in ``[0, G)`` with ``G = max + 1``, and a group without agents keeps its (zero) column.
    A dict entry whose value is a mapping bins a numeric attribute instead - ``{age_band: {attribute: age, bins: [0, 18,
    65, 100]}}``: the label is the band with ``lo <= value < hi``, the column keys are ``"0-18"``, ``"18-65"``, ... (the
    naming of ``Vaccination``'s efficacy bands), and a band without agents keeps its column (:func:`bin_attribute`).
    Returns ``({name: int32 labels [n_agents]}, {name: list of column keys})``."""
    n = len(agent["id"])
    items: List[Tuple[str, object]] = []
    if isinstance(spec, dict):
        items = [(k, v) for k, v in spec.items()]
    elif isinstance(spec, (list, tuple)):
        for s in spec:
            if isinstance(s, dict):
                items.extend(s.items())
            else:
                items.append((s, None))
    elif isinstance(spec, str):
        items = [(spec, None)]
    else:
        raise TypeError(f"groups: expected a list of attribute names or a dict name -> labels, not {type(spec).__name__}")
    labels, keys = {}, {}
    for name, given in items:
        check_group_name(name)
        if name in labels:
            raise ValueError(f"group '{name}' is given twice")
        if isinstance(given, dict):
            lab, key = bin_attribute(agent, name, given)
        elif given is None:
            if name not in agent:
                raise KeyError(f"groups: the world's agents have no attribute '{name}' "
                               f"(present: {sorted(k for k in agent.keys())})")
            values = _as_numpy(agent[name])
            if values.ndim != 1 or values.shape[0] != n:
                raise ValueError(f"group '{name}': attribute of shape {values.shape}, expected ({n},)")
            uniq, inverse = np.unique(values, return_inverse=True)
            lab, key = inverse.reshape(-1), uniq.tolist()
        else:
            lab = _as_numpy(given)
            if lab.ndim != 1 or lab.shape[0] != n:
                raise ValueError(f"group '{name}': {lab.shape} labels for {n} agents")
            if lab.dtype.kind not in "iu":
                raise TypeError(f"group '{name}': integer labels expected, not {lab.dtype}")
            if n and (int(lab.min()) < 0 or int(lab.max()) >= N.GJ_MAX_GROUPS):
                raise ValueError(f"group '{name}': labels must lie in [0, {N.GJ_MAX_GROUPS})")
            key = list(range(int(lab.max()) + 1 if n else 1))
        labels[name] = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32))
        keys[name] = key
    return labels, keys


def bin_attribute(agent, name, spec) -> Tuple[np.ndarray, List[str]]:
    """The labelling ``name: {attribute: <agent attribute>, bins: [e0, e1, ...]}``: (labels, column keys).  Band i is
    ``bins[i] <= value < bins[i + 1]`` and is called ``"<bins[i]>-<bins[i + 1]>"``.  The bins must increase strictly, and
    every agent's value must lie in one of them: both are ``ValueError`` otherwise."""
    unknown = set(spec) - {"attribute", "bins"}
    if unknown or "attribute" not in spec or "bins" not in spec:
        raise ValueError(f"group '{name}': a binned labelling is {{attribute: <name>, bins: [..]}}, not {dict(spec)!r}")
    attribute, bins = spec["attribute"], spec["bins"]
    if not isinstance(attribute, str) or attribute not in agent:
        raise KeyError(f"group '{name}': the world's agents have no attribute '{attribute}' "
                       f"(present: {sorted(k for k in agent.keys())})")
    values = _as_numpy(agent[attribute])
    n = len(agent["id"])
    if values.ndim != 1 or values.shape[0] != n or values.dtype.kind not in "iuf":
        raise ValueError(f"group '{name}': attribute '{attribute}' of shape {values.shape} and type {values.dtype}, "
                         f"expected {n} numbers")
    if isinstance(bins, (str, bytes)) or not hasattr(bins, "__len__") or len(bins) < 2:
        raise ValueError(f"group '{name}': bins = {bins!r}, expected at least two edges")
    edges = np.asarray(bins, dtype=np.float64)
    if edges.ndim != 1 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
        raise ValueError(f"group '{name}': bins {list(bins)} are not strictly increasing")
    lab = np.digitize(values, edges) - 1                      # edges[i] <= value < edges[i + 1]
    outside = (lab < 0) | (lab >= len(edges) - 1) | ~np.isfinite(values.astype(np.float64))
    if outside.any():
        raise ValueError(f"group '{name}': {int(outside.sum())} agents have a value of '{attribute}' outside every bin of "
                         f"{list(bins)} (lo <= value < hi), e.g. {values[outside][:3].tolist()}")
    return lab, [f"{lo}-{hi}" for lo, hi in zip(bins[:-1], bins[1:])]


def attach_groups(agent, spec) -> None:
    """Encode ``spec`` on ``agent`` and keep the result on it: ``group_labels`` (a dict of per-agent tensors, so that
    whatever renumbers or cuts the agents - graph.locality_order, the multi-GPU partition - carries the labels along)
    and ``group_keys`` (lists: not per-agent data)."""
    labels, keys = encode_groups(agent, spec)
    old_l, old_k = dict(agent.get("group_labels", None) or {}), dict(agent.get("group_keys", None) or {})
    old_l.update(labels)
    old_k.update(keys)
    agent.group_labels, agent.group_keys = old_l, old_k


class GroupStats:
    """One labelling on the device: labels, group count and the workspace of ``gj_group_stats``."""

    def __init__(self, labels: torch.Tensor, n_groups: int, device=None):
        if n_groups < 1 or n_groups > N.GJ_MAX_GROUPS:
            raise ValueError(f"n_groups = {n_groups}: expected 1 .. {N.GJ_MAX_GROUPS}")
        dev = torch.device(device) if device is not None else labels.device
        self.labels = labels.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.n_groups = int(n_groups)
        self.n = self.labels.numel()
        # GJ_GROUP_WORKSPACE_BYTES: 2 G sums of 8 bytes, then the error word
        self.workspace = torch.zeros(2 * self.n_groups + 1, dtype=torch.int64, device=dev)

    def add(self, is_infected: torch.Tensor, current_stage: torch.Tensor, dead: int, out: torch.Tensor) -> None:
        """out[0:G] += cases by group, out[G:2G] += deaths by group (fp64, device)."""
        if is_infected.numel() != self.n or current_stage.numel() != self.n:
            raise ValueError(f"{is_infected.numel()} / {current_stage.numel()} values for {self.n} labels")
        if out.dtype != torch.float64 or out.numel() != 2 * self.n_groups or not out.is_contiguous():
            raise ValueError("out: a contiguous float64 tensor of 2 * n_groups elements")
        N.check(N.load().gj_group_stats(self.n, N.ptr(self.labels), self.n_groups, N.ptr(is_infected),
                                        N.ptr(current_stage), int(dead), N.ptr(out), N.ptr(self.workspace),
                                        N.current_stream()), "gj_group_stats")

    def gather(self, current_stage, dead: int, g_cases, g_deaths, want_inf: bool = True, want_stage: bool = True):
        """The adjoint: (grad_is_infected or None, grad_stage or None)."""
        dev = self.labels.device
        grad_inf = torch.empty(self.n, dtype=torch.float32, device=dev) if want_inf else None
        grad_stage = torch.empty(self.n, dtype=torch.float32, device=dev) if want_stage else None
        N.check(N.load().gj_adjoint_group_stats(self.n, N.ptr(self.labels), self.n_groups, N.ptr(current_stage),
                                                int(dead), N.ptr(g_cases), N.ptr(g_deaths), N.ptr(grad_inf),
                                                N.ptr(grad_stage), N.current_stream()), "gj_adjoint_group_stats")
        return grad_inf, grad_stage

    def check(self, what: str = "gj_group_stats") -> None:
        """Raise if a launch since the last check met a bad label or value (one device read)."""
        word = self.workspace[2 * self.n_groups:]
        err = int(word.item()) & 0xFFFFFFFF
        if err:
            word.zero_()
            why = []
            if err & N.GJ_GROUP_ERR_LABEL:
                why.append(f"a label outside [0, {self.n_groups}) (its agent was skipped)")
            if err & N.GJ_GROUP_ERR_VALUE:
                why.append("an is_infected that is not finite or beyond 2^18 (it was counted as 0)")
            raise GroupLabelError(f"{what}: " + " and ".join(why))


class StageLabelError(RuntimeError):
    """gj_stage_stats met a label outside [0, n_groups) or a stage that is no integer in [0, n_stages)."""


def stages_to_save(spec, stages) -> List[str]:
    """The YAML key ``stages_to_save`` / the Runner's ``stages=``: a list of names of ``symptoms.stages``, or ``all``.
    Returns the names in the order given (``all``: the model's order).  An unknown name, and a name whose result keys
    ``<st>_per_timestep`` / ``new_<st>_per_timestep`` / ``<st>_by_<name>`` would shadow a key the Runner already
    reports, raise ``ValueError``."""
    stages = [str(s) for s in stages]
    if spec is None or (isinstance(spec, (list, tuple)) and not spec):
        return []
    if isinstance(spec, str):
        spec = stages if spec == "all" else [spec]
    names = [str(s) for s in spec]
    for st in names:
        if st not in stages:
            raise ValueError(f"stages_to_save: '{st}' is no symptom stage (known: {stages})")
        if st in _STAGE_SHADOWS or "new_" + st in names:
            raise ValueError(f"stages_to_save: the series of stage '{st}' would shadow the result key '{st}_per_timestep'")
    if len(set(names)) != len(names):
        raise ValueError(f"stages_to_save: a stage is given twice ({names})")
    return names


class StageStats:
    """``gj_stage_stats`` / ``gj_adjoint_stage_stats`` for one labelling of the agents, or for none (``labels`` None:
    the national call, one group): the labels, the shape of the histogram and the sticky error word."""

    def __init__(self, labels, n_groups: int, n_stages: int, device=None):
        if n_groups < 1 or n_groups > N.GJ_MAX_GROUPS:
            raise ValueError(f"n_groups = {n_groups}: expected 1 .. {N.GJ_MAX_GROUPS}")
        if n_stages < 1 or n_stages > N.GJ_MAX_STAGES or n_groups * n_stages > 2 ** 31 - 1:
            raise ValueError(f"n_stages = {n_stages}: expected 1 .. {N.GJ_MAX_STAGES}, n_groups * n_stages < 2^31")
        if labels is None and n_groups != 1:
            raise ValueError("no labels: one group")
        dev = torch.device(device) if device is not None else labels.device
        self.labels = None if labels is None else labels.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.n_groups, self.n_stages, self.device = int(n_groups), int(n_stages), dev
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def _agents(self, *per_agent) -> int:
        n = per_agent[0].numel()
        for t in per_agent:
            if t is not None and (t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError("per-agent arguments: contiguous float32 tensors of one length")
        if self.labels is not None and self.labels.numel() != n:
            raise ValueError(f"{n} stages for {self.labels.numel()} labels")
        return n

    def add(self, current_stage: torch.Tensor, prev_stage, out: torch.Tensor) -> None:
        """out[0] += occupancy [G, S]; out[1] += entries [G, S] where ``prev_stage`` (or None) differs (int64, device)."""
        n = self._agents(current_stage, prev_stage)
        if out.dtype != torch.int64 or out.numel() != 2 * self.n_groups * self.n_stages or not out.is_contiguous():
            raise ValueError("out: a contiguous int64 tensor of 2 * n_groups * n_stages elements")
        N.check(N.load().gj_stage_stats(n, N.ptr(self.labels), self.n_groups, self.n_stages, N.ptr(current_stage),
                                        N.ptr(prev_stage), N.ptr(out), N.ptr(self.err), N.current_stream()),
                "gj_stage_stats")

    def gather(self, current_stage, prev_stage, g_occupancy, g_entries) -> torch.Tensor:
        """The adjoint: grad_stage [n] for the cotangents [G, S] (fp32, or None = zeros) of the two planes."""
        n = self._agents(current_stage, prev_stage)
        for g in (g_occupancy, g_entries):
            if g is not None and (g.dtype != torch.float32 or g.numel() != self.n_groups * self.n_stages
                                  or not g.is_contiguous()):
                raise ValueError("cotangents: contiguous float32 tensors of n_groups * n_stages elements")
        grad = torch.empty(n, dtype=torch.float32, device=self.device)
        N.check(N.load().gj_adjoint_stage_stats(n, N.ptr(self.labels), self.n_groups, self.n_stages,
                                                N.ptr(current_stage), N.ptr(prev_stage), N.ptr(g_occupancy),
                                                N.ptr(g_entries), N.ptr(grad), N.current_stream()),
                "gj_adjoint_stage_stats")
        return grad

    def check(self, what: str = "gj_stage_stats") -> None:
        """Raise if a launch since the last check met a bad label or stage (one device read)."""
        err = int(self.err.item()) & 0xFFFFFFFF
        if err:
            self.err.zero_()
            why = []
            if err & N.GJ_STAGE_ERR_LABEL:
                why.append(f"a label outside [0, {self.n_groups}) (its agent was skipped)")
            if err & N.GJ_STAGE_ERR_STAGE:
                why.append(f"a stage that is no integer in [0, {self.n_stages}) (its agent was skipped)")
            raise StageLabelError(f"{what}: " + " and ".join(why))


class LocationError(RuntimeError):
    """gj_location_stats met a label outside [0, n_groups), a new_infected that is neither 0 nor 1, a NaN or negative
    term, or a row outside its edge set."""


def locations_to_save(spec) -> bool:
    """The YAML key ``locations_to_save`` / the Runner's ``locations=``: true or false (absent: false)."""
    if spec is None:
        return False
    if isinstance(spec, (bool, np.bool_)):
        return bool(spec)
    raise ValueError(f"locations_to_save: expected true or false, not {spec!r}")


def location_keys(networks) -> List[str]:
    """Columns of the infection-location series: the network names in the order given (``infection_networks.networks``),
    then ``background`` (an infection nobody transmitted: the reference's probability floor), then ``seed``."""
    names = [str(n) for n in networks]
    for reserved in ("background", "seed"):
        if reserved in names:
            raise ValueError(f"a network named '{reserved}' would shadow that column of the infection-location series")
    return names + ["background", "seed"]


class LocationStats:
    """``gj_location_stats`` for one labelling of the agents, or for none (``labels`` None: the national call, one
    group).  Owns the integer series ``out`` [rows, n_groups, len(columns)] - units of 1 / GJ_LOC_UNIT of an infection -
    and the sticky error word."""

    def __init__(self, labels, n_groups: int, columns, device=None, n_rows: int = 1):
        if n_groups < 1 or n_groups > N.GJ_MAX_GROUPS:
            raise ValueError(f"n_groups = {n_groups}: expected 1 .. {N.GJ_MAX_GROUPS}")
        if labels is None and n_groups != 1:
            raise ValueError("no labels: one group")
        self.columns = [str(c) for c in columns]
        if not 1 <= len(self.columns) <= N.GJ_LOC_MAX_COLS or len(set(self.columns)) != len(self.columns):
            raise ValueError(f"columns: 1 .. {N.GJ_LOC_MAX_COLS} distinct names, not {self.columns}")
        dev = torch.device(device) if device is not None else labels.device
        self.labels = None if labels is None else labels.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.n_groups, self.n_cols, self.device = int(n_groups), len(self.columns), dev
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.reset(n_rows)

    def reset(self, n_rows: int = 1) -> None:
        self.out = torch.zeros(int(n_rows), self.n_groups, self.n_cols, dtype=torch.int64, device=self.device)

    def add(self, plan, params, new_infected, susceptibility0, current_stage, active=(), background="background",
            row: int = 0, edges=None) -> None:
        """out[row] += the shares of the step ``params`` describes (a ``gj_step_params``, after its ``gj_step`` on
        ``plan``: the plan's ``cum`` workspaces hold that step's sums).  ``active``: the column name of each of the
        step's networks, in the order of ``params.nets``; ``edges``: see ``DevicePlan.location_rows``."""
        n = plan.host.n_agents
        for t in (new_infected, susceptibility0, current_stage):
            if t is not None and (t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.device != self.device):
                raise ValueError(f"per-agent arguments: contiguous float32[{n}] on {self.device}")
        if self.labels is not None and self.labels.numel() != n:
            raise ValueError(f"{n} agents for {self.labels.numel()} labels")
        if len(active) != params.n_nets:
            raise ValueError(f"{len(active)} columns for {params.n_nets} active networks")
        import ctypes as C

        cols = (C.c_int32 * max(1, len(active)))(*[self.columns.index(str(c)) for c in active])
        N.check(N.load().gj_location_stats(
            C.byref(plan.c), C.byref(params), plan.location_rows(edges), N.ptr(new_infected), N.ptr(susceptibility0),
            N.ptr(current_stage), N.ptr(self.labels), self.n_groups, cols, self.n_cols,
            self.columns.index(background), N.ptr(self.out[row]), N.ptr(self.err), N.current_stream()),
            "gj_location_stats")

    def values(self, n_rows=None) -> torch.Tensor:
        """The series in infections: out / GJ_LOC_UNIT formed in fp64, then float32 [rows, n_groups, columns]."""
        out = self.out if n_rows is None else self.out[:n_rows]
        return (out.to(torch.float64) / float(N.GJ_LOC_UNIT)).to(torch.float32)

    def check(self, what: str = "gj_location_stats") -> None:
        """Raise if a launch since the last check met bad input (one device read)."""
        err = int(self.err.item()) & 0xFFFFFFFF
        if err:
            self.err.zero_()
            why = []
            if err & N.GJ_LOC_ERR_LABEL:
                why.append(f"a label outside [0, {self.n_groups}) (its agent was skipped)")
            if err & N.GJ_LOC_ERR_VALUE:
                why.append("a new_infected that is neither 0 nor 1 (skipped) or a NaN / negative term (counted as 0)")
            if err & N.GJ_LOC_ERR_ROWS:
                why.append("a row pointer or venue id outside its edge set (skipped)")
            raise LocationError(f"{what}: " + " and ".join(why))


def infection_matrices_to_save(spec) -> List[str]:
    """The YAML key ``infection_matrices_to_save`` / the Runner's ``matrices=``: a list of labelling names (absent: none)."""
    if spec is None:
        return []
    if isinstance(spec, str):
        spec = [spec]
    if not isinstance(spec, (list, tuple)) or not all(isinstance(s, str) for s in spec):
        raise ValueError(f"infection_matrices_to_save: expected a list of labelling names, not {spec!r}")
    if len(set(spec)) != len(spec):
        raise ValueError(f"infection_matrices_to_save: a labelling is given twice ({list(spec)})")
    return list(spec)


class InfectorError(RuntimeError):
    """gj_infector_scatter / gj_infector_gather met a label outside [0, n_groups), a new_infected that is neither 0 nor
    1, a NaN or negative term, a credit that is not finite, or a row outside its edge set."""


def infectors_to_save(spec) -> bool:
    """The YAML key ``infectors_to_save`` / the Runner's ``infectors=``: true or false (absent: false)."""
    if spec is None:
        return False
    if isinstance(spec, (bool, np.bool_)):
        return bool(spec)
    raise ValueError(f"infectors_to_save: expected true or false, not {spec!r}")


class InfectorStats:
    """``gj_infector_scatter`` / ``gj_infector_gather`` for a world of ``n_agents`` and any number of labellings
    (``labellings``: {name: (labels, n_groups)}; the national sums are kept under the key None).  Owns what the two passes
    accumulate over a run: ``caused`` (fp64 [n]: the infections every agent caused), ``infected_row`` (int32 [n]: the row
    an agent was infected in, -1: never), the integer series ``out[key]`` [rows, n_groups] - units of 1 / GJ_LOC_UNIT of
    an infection, by the INFECTOR's group - and ``unattributed`` [rows] (exact counts), and the sticky error word.  ``U``,
    the per-venue units of one step, lives with the plan (``DevicePlan.infector_units``) and is zero between steps:
    ``clear`` = "memset" zeroes all of it, "walk" only the venues the step's new infections touched.

    ``matrices``: the names of the labellings (a list, or a dict by name) that also get a who-infects-whom matrix
    (``gj_infection_matrix_scatter`` / ``gj_infection_matrix_gather``): ``matrix[name]`` [rows, G, G] - the same units,
    [infector's group, infected's group] - and ``unattributed_by[name]`` [rows, G] (exact counts, by the infected agent's
    group).  A labelling of more than GJ_MATRIX_MAX_GROUPS groups cannot have one.  ``UG``, the units of one step by the
    infected's group, lives with the plan too (``DevicePlan.infection_matrix_units``), G times the size of ``U``;
    ``matrix_clear`` = "memset" or "walk" as for ``U``."""

    def __init__(self, n_agents: int, labellings=None, device=None, n_rows: int = 1, clear: str = "memset",
                 matrices=None, matrix_clear: str = "walk"):
        for how in (clear, matrix_clear):
            if how not in ("memset", "walk"):
                raise ValueError(f"clear = {how!r}: 'memset' or 'walk'")
        self.n, self.device, self.clear_by = int(n_agents), torch.device(device), clear
        self.matrix_clear_by = matrix_clear
        self.labels, self.n_groups = {None: None}, {None: 1}
        for name, (labels, n_groups) in (labellings or {}).items():
            if n_groups < 1 or n_groups > N.GJ_MAX_GROUPS:
                raise ValueError(f"n_groups = {n_groups}: expected 1 .. {N.GJ_MAX_GROUPS}")
            if labels.numel() != self.n:
                raise ValueError(f"{self.n} agents for {labels.numel()} labels of '{name}'")
            self.labels[name] = labels.detach().to(device=self.device, dtype=torch.int32).contiguous()
            self.n_groups[name] = int(n_groups)
        self.matrix_names = list(matrices or ())
        for name in self.matrix_names:
            if name is None or name not in self.labels:
                raise ValueError(f"infection matrix by '{name}': no such labelling (present: "
                                 f"{sorted(k for k in self.labels if k is not None)})")
            if self.n_groups[name] > N.GJ_MATRIX_MAX_GROUPS:
                raise ValueError(f"infection matrix by '{name}': {self.n_groups[name]} groups, a matrix takes at most "
                                 f"{N.GJ_MATRIX_MAX_GROUPS} (GJ_MATRIX_MAX_GROUPS)")
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.reset(n_rows)

    def reset(self, n_rows: int = 1) -> None:
        dev = self.device
        self.caused = torch.zeros(self.n, dtype=torch.float64, device=dev)
        self.infected_row = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.unattributed = torch.zeros(int(n_rows), dtype=torch.int64, device=dev)
        self.out = {key: torch.zeros(int(n_rows), G, dtype=torch.int64, device=dev) for key, G in self.n_groups.items()}
        groups = {name: self.n_groups[name] for name in self.matrix_names}
        self.matrix = {name: torch.zeros(int(n_rows), G, G, dtype=torch.int64, device=dev) for name, G in groups.items()}
        self.unattributed_by = {name: torch.zeros(int(n_rows), G, dtype=torch.int64, device=dev)
                                for name, G in groups.items()}

    def _agents(self, *per_agent) -> None:
        for t in per_agent:
            if t is not None and (t.numel() != self.n or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.device != self.device):
                raise ValueError(f"per-agent arguments: contiguous float32[{self.n}] on {self.device}")

    def scatter(self, plan, params, new_infected, susceptibility0, current_stage, row: int = 0, edges=None,
                cohort: bool = True) -> None:
        """Pass 1 of the step ``params`` describes, into the plan's ``U`` (zero before); unattributed[row] += the
        infections nobody transmitted; infected_row = row for the step's new infections (``cohort``)."""
        import ctypes as C

        if plan.host.n_agents != self.n:
            raise ValueError(f"a plan of {plan.host.n_agents} agents for {self.n}")
        self._agents(new_infected, susceptibility0, current_stage)
        if not 0 <= row < self.unattributed.numel():
            raise IndexError(f"row {row} of {self.unattributed.numel()}")
        N.check(N.load().gj_infector_scatter(
            C.byref(plan.c), C.byref(params), plan.location_rows(edges), N.ptr(new_infected), N.ptr(susceptibility0),
            N.ptr(current_stage), plan.infector_units()[1], N.ptr(self.unattributed[row:]),
            N.ptr(self.infected_row) if cohort else None, int(row), N.ptr(self.err), N.current_stream()),
            "gj_infector_scatter")

    def gather(self, plan, params, transmission, current_stage, row: int = 0, edges=None) -> None:
        """Pass 2: caused += the step's credits (once), out[key][row] += their sums by group for every labelling."""
        import ctypes as C

        n_ext = plan.host.n_ext_agents      # (the step's transmission array: the owned agents come first)
        if (transmission.numel() != n_ext or transmission.dtype != torch.float32 or not transmission.is_contiguous()
                or transmission.device != self.device):
            raise ValueError(f"transmission: contiguous float32[{n_ext}] on {self.device}")
        self._agents(current_stage)
        if not 0 <= row < self.unattributed.numel():
            raise IndexError(f"row {row} of {self.unattributed.numel()}")
        for key, G in self.n_groups.items():
            N.check(N.load().gj_infector_gather(
                C.byref(plan.c), C.byref(params), plan.location_rows(edges), N.ptr(transmission), N.ptr(current_stage),
                plan.infector_units()[1], N.ptr(self.labels[key]), G, N.ptr(self.caused) if key is None else None,
                N.ptr(self.out[key][row]), N.ptr(self.err), N.current_stream()), "gj_infector_gather")

    def clear(self, plan, new_infected=None, edges=None) -> None:
        """The plan's ``U`` back to zero: all of it, or (``clear`` = "walk") what the step of ``new_infected`` touched."""
        import ctypes as C

        U, pointers = plan.infector_units()
        if self.clear_by == "walk" and new_infected is not None:
            N.check(N.load().gj_infector_clear(C.byref(plan.c), plan.location_rows(edges), N.ptr(new_infected), pointers,
                                               N.current_stream()), "gj_infector_clear")
        else:
            for u in U:
                u.zero_()

    def matrix_scatter(self, plan, params, new_infected, susceptibility0, current_stage, row: int = 0, edges=None) -> None:
        """Pass 1 once more for every labelling with a matrix, into the plan's ``UG`` of that labelling (zero before);
        unattributed_by[name][row] += the infections nobody transmitted, by the infected agent's group."""
        import ctypes as C

        if plan.host.n_agents != self.n:
            raise ValueError(f"a plan of {plan.host.n_agents} agents for {self.n}")
        self._agents(new_infected, susceptibility0, current_stage)
        if not 0 <= row < self.unattributed.numel():
            raise IndexError(f"row {row} of {self.unattributed.numel()}")
        for name in self.matrix_names:
            G = self.n_groups[name]
            N.check(N.load().gj_infection_matrix_scatter(
                C.byref(plan.c), C.byref(params), plan.location_rows(edges), N.ptr(new_infected), N.ptr(susceptibility0),
                N.ptr(current_stage), N.ptr(self.labels[name]), G, plan.infection_matrix_units(name, G)[1],
                N.ptr(self.unattributed_by[name][row]), N.ptr(self.err), N.current_stream()),
                "gj_infection_matrix_scatter")

    def matrix_gather(self, plan, params, transmission, current_stage, row: int = 0, edges=None) -> None:
        """Pass 2 by pairs of groups: matrix[name][row] += the step's terms, for every labelling with a matrix.  Needs
        the step's ``U`` (``scatter``) beside its ``UG``."""
        import ctypes as C

        n_ext = plan.host.n_ext_agents
        if (transmission.numel() != n_ext or transmission.dtype != torch.float32 or not transmission.is_contiguous()
                or transmission.device != self.device):
            raise ValueError(f"transmission: contiguous float32[{n_ext}] on {self.device}")
        self._agents(current_stage)
        if not 0 <= row < self.unattributed.numel():
            raise IndexError(f"row {row} of {self.unattributed.numel()}")
        for name in self.matrix_names:
            G = self.n_groups[name]
            N.check(N.load().gj_infection_matrix_gather(
                C.byref(plan.c), C.byref(params), plan.location_rows(edges), N.ptr(transmission), N.ptr(current_stage),
                plan.infector_units()[1], plan.infection_matrix_units(name, G)[1], N.ptr(self.labels[name]), G,
                N.ptr(self.matrix[name][row]), N.ptr(self.err), N.current_stream()), "gj_infection_matrix_gather")

    def matrix_clear(self, plan, new_infected=None, edges=None) -> None:
        """The plan's ``UG`` of every labelling with a matrix back to zero: all of it, or (``matrix_clear`` = "walk")
        what the step of ``new_infected`` touched."""
        import ctypes as C

        for name in self.matrix_names:
            G = self.n_groups[name]
            UG, pointers = plan.infection_matrix_units(name, G)
            if self.matrix_clear_by == "walk" and new_infected is not None:
                N.check(N.load().gj_infection_matrix_clear(C.byref(plan.c), plan.location_rows(edges), N.ptr(new_infected),
                                                           pointers, G, N.current_stream()), "gj_infection_matrix_clear")
            else:
                for u in UG:
                    u.zero_()

    def record(self, plan, params, new_infected, susceptibility0, current_stage, transmission, row: int = 0,
               edges=None) -> None:
        """One step: scatter, the matrix scatters, then (a step with networks) the gathers, the matrix gathers and the
        clears."""
        self.scatter(plan, params, new_infected, susceptibility0, current_stage, row=row, edges=edges)
        if self.matrix_names:
            self.matrix_scatter(plan, params, new_infected, susceptibility0, current_stage, row=row, edges=edges)
        if params.n_nets > 0:
            self.gather(plan, params, transmission, current_stage, row=row, edges=edges)
            if self.matrix_names:
                self.matrix_gather(plan, params, transmission, current_stage, row=row, edges=edges)
            self.clear(plan, new_infected, edges=edges)
            if self.matrix_names:
                self.matrix_clear(plan, new_infected, edges=edges)

    def values(self, key=None, n_rows=None) -> torch.Tensor:
        """A series in infections: out / GJ_LOC_UNIT formed in fp64, then float32 [rows, n_groups]."""
        out = self.out[key] if n_rows is None else self.out[key][:n_rows]
        return (out.to(torch.float64) / float(N.GJ_LOC_UNIT)).to(torch.float32)

    def matrix_values(self, name, n_rows=None) -> torch.Tensor:
        """A matrix series in infections, formed as ``values`` forms its: float32 [rows, G (infector), G (infected)]."""
        out = self.matrix[name] if n_rows is None else self.matrix[name][:n_rows]
        return (out.to(torch.float64) / float(N.GJ_LOC_UNIT)).to(torch.float32)

    def reproduction(self, n_rows: int, key=None) -> torch.Tensor:
        """The case reproduction number by cohort, float32 [n_rows, n_groups]: the mean of ``caused`` over the agents
        infected in row r (of group g); NaN for an empty cohort.  One ``gj_group_stats`` pass on the label
        ``infected_row * G + g`` with ``caused`` as float32 values; the counts are an integer bincount."""
        G, T = self.n_groups[key], int(n_rows)
        row = self.infected_row.long()
        label = row * G + (0 if key is None else self.labels[key].long())
        if key is not None:
            label = torch.where((self.labels[key] >= 0) & (self.labels[key] < G), label, torch.full_like(label, T * G))
        label = torch.where((row >= 0) & (row < T), label, torch.full_like(label, T * G))      # bin T * G: not a cohort
        stats = GroupStats(label, T * G + 1, device=self.device)
        sums = torch.zeros(2 * (T * G + 1), dtype=torch.float64, device=self.device)
        stats.add(self.caused.to(torch.float32), torch.zeros(self.n, dtype=torch.float32, device=self.device), 1, sums)
        stats.check("reproduction number")
        counts = torch.bincount(label, minlength=T * G + 1)[: T * G]
        return (sums[: T * G] / counts.to(torch.float64)).to(torch.float32).view(T, G)

    def check(self, what: str = "gj_infector_scatter / gj_infector_gather") -> None:
        """Raise if a launch since the last check met bad input (one device read)."""
        err = int(self.err.item()) & 0xFFFFFFFF
        if err:
            self.err.zero_()
            why = []
            if err & N.GJ_LOC_ERR_LABEL:
                why.append("a label outside its labelling's groups (its agent was skipped)")
            if err & N.GJ_LOC_ERR_VALUE:
                why.append("a new_infected that is neither 0 nor 1 (skipped), a NaN / negative term (counted as 0) "
                           "or a credit that is not finite (skipped)")
            if err & N.GJ_LOC_ERR_ROWS:
                why.append("a row pointer or venue id outside its edge set (skipped)")
            raise InfectorError(f"{what}: " + " and ".join(why))


class InfectionTreeError(RuntimeError):
    """gj_infection_tree met a new_infected that is neither 0 nor 1, a NaN or negative term, a saturated weight, or a
    row outside its edge set."""


def infection_tree_to_save(spec) -> bool:
    """The YAML key ``infection_tree_to_save`` / the Runner's ``tree=``: true or false (absent: false)."""
    if spec is None:
        return False
    if isinstance(spec, (bool, np.bool_)):
        return bool(spec)
    raise ValueError(f"infection_tree_to_save: expected true or false, not {spec!r}")


class InfectionTree:
    """``gj_infection_tree`` for a world of ``n_agents``: one sampled infector per infection.  Owns what the launches
    write over a run - per agent, int32: ``infector`` (global id; -1 never infected, -2 nobody transmitted, -3
    unresolved), ``via`` (the index into ``columns`` of the location it came through), ``venue`` (in its edge set's
    numbering, -1 with -2) and ``infected_row`` (-1: never) - and per row ``counts`` [rows, L] (exact, by location
    column) and ``unresolved`` [rows], and the sticky error word."""

    def __init__(self, n_agents: int, columns, device=None, n_rows: int = 1):
        self.columns = [str(c) for c in columns]
        if not 1 <= len(self.columns) <= N.GJ_LOC_MAX_COLS or len(set(self.columns)) != len(self.columns):
            raise ValueError(f"columns: 1 .. {N.GJ_LOC_MAX_COLS} distinct names, not {self.columns}")
        self.n, self.device = int(n_agents), torch.device(device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.reset(n_rows)

    def reset(self, n_rows: int = 1) -> None:
        dev = self.device
        self.infector = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.via = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.venue = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.infected_row = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(int(n_rows), len(self.columns), dtype=torch.int64, device=dev)
        self.unresolved = torch.zeros(int(n_rows), dtype=torch.int64, device=dev)

    def record(self, plan, params, new_infected, susceptibility0, current_stage, transmission, active=(),
               background="background", row: int = 0, edges=None, seed: int = 0, step: int = 0,
               agent_offset: int = 0) -> None:
        """One step: the tree's entries of the agents with new_infected == 1, counts[row] and unresolved[row].
        ``active``: the column name of each of the step's networks, in the order of ``params.nets``; ``seed``, ``step``:
        the Philox key and stream of the draw; ``edges``: see ``DevicePlan.location_rows`` / ``venue_rows``."""
        import ctypes as C

        if plan.host.n_agents != self.n:
            raise ValueError(f"a plan of {plan.host.n_agents} agents for {self.n}")
        for t in (new_infected, susceptibility0, current_stage):
            if t is not None and (t.numel() != self.n or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.device != self.device):
                raise ValueError(f"per-agent arguments: contiguous float32[{self.n}] on {self.device}")
        n_ext = plan.host.n_ext_agents
        if transmission is not None and (transmission.numel() != n_ext or transmission.dtype != torch.float32
                                         or not transmission.is_contiguous() or transmission.device != self.device):
            raise ValueError(f"transmission: contiguous float32[{n_ext}] on {self.device}")
        if len(active) != params.n_nets:
            raise ValueError(f"{len(active)} columns for {params.n_nets} active networks")
        if not 0 <= row < self.unresolved.numel():
            raise IndexError(f"row {row} of {self.unresolved.numel()}")
        cols = (C.c_int32 * max(1, len(active)))(*[self.columns.index(str(c)) for c in active])
        venue_rows = plan.venue_rows(edges) if params.n_nets > 0 else None      # (the seeding step reads no venue)
        N.check(N.load().gj_infection_tree(
            C.byref(plan.c), C.byref(params), plan.location_rows(edges), venue_rows, N.ptr(new_infected),
            N.ptr(susceptibility0), N.ptr(current_stage), N.ptr(transmission), cols, len(self.columns),
            self.columns.index(background), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(agent_offset),
            N.ptr(self.infector), N.ptr(self.via), N.ptr(self.venue), N.ptr(self.infected_row), int(row),
            N.ptr(self.counts[row]), N.ptr(self.unresolved[row:]), N.ptr(self.err), N.current_stream()),
            "gj_infection_tree")

    def offspring(self) -> torch.Tensor:
        """int64 [n]: the infections every agent was drawn as the infector of (agent_offset 0)."""
        drawn = self.infector[self.infector >= 0].long()
        return torch.bincount(drawn, minlength=self.n)[: self.n]

    def check(self, what: str = "gj_infection_tree") -> None:
        """Raise if a launch since the last check met bad input (one device read)."""
        err = int(self.err.item()) & 0xFFFFFFFF
        if err:
            self.err.zero_()
            why = []
            if err & N.GJ_LOC_ERR_VALUE:
                why.append("a new_infected that is neither 0 nor 1 (skipped), a NaN / negative term (counted as 0) or a "
                           "transmitter's weight above 2^10 (saturated)")
            if err & N.GJ_LOC_ERR_ROWS:
                why.append("a row pointer, venue id or member outside its edge set (skipped)")
            raise InfectionTreeError(f"{what}: " + " and ".join(why))


class SeedPlan:
    """One labelling as ``gj_adjoint_seed`` wants it (include/gradjune_hip.h, gj_seed_plan): the agents with a label in
    [0, n_groups) sorted by label (stable), every group's segment cut into chunks of GJ_SEED_CHUNK agents.  Built once per
    labelling with torch ops on the labels' device (one host read: the number of chunks)."""

    def __init__(self, labels: torch.Tensor, n_groups: int, device=None):
        if n_groups < 1 or n_groups > N.GJ_MAX_GROUPS:
            raise ValueError(f"n_groups = {n_groups}: expected 1 .. {N.GJ_MAX_GROUPS}")
        dev = torch.device(device) if device is not None else labels.device
        self.labels = labels.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.n_groups, self.n = int(n_groups), self.labels.numel()
        G = self.n_groups
        lab = self.labels.long()
        key = torch.where((lab >= 0) & (lab < G), lab, torch.full_like(lab, G))     # no group: sorted behind the last
        counts = torch.bincount(key, minlength=G + 1)[:G]
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        chunks = (counts + (N.GJ_SEED_CHUNK - 1)) // N.GJ_SEED_CHUNK
        self.seg_offsets = torch.cat((zero, torch.cumsum(counts, 0))).contiguous()
        self.chunk_first = torch.cat((zero, torch.cumsum(chunks, 0))).contiguous()
        self.n_sorted, self.n_chunks = (int(v) for v in torch.stack((counts.sum(), chunks.sum())).tolist())
        self.order = torch.argsort(key, stable=True)[: self.n_sorted].contiguous()
        self.chunk_group = torch.repeat_interleave(torch.arange(G, device=dev), chunks).to(torch.int32).contiguous()
        self.c = N.SeedPlan(self.n_sorted, self.n_chunks, N.ptr(self.order), N.ptr(self.seg_offsets),
                            N.ptr(self.chunk_first), N.ptr(self.chunk_group))

    @property
    def all_valid(self) -> bool:
        return self.n_sorted == self.n


def seed_log_fractions(seed_params: dict, keys=None):
    """The ``infection_seed`` section of the YAML schema -> (attribute to seed by or None, log fractions).

    ``log_fraction_initial_cases`` alone (the reference's schema): (None, that scalar, as it is).  With ``by: <agent
    attribute>`` every group of that labelling gets its own log fraction: ``log_fraction_by_group: {key: value}`` for
    the groups listed, the scalar for the others.  ``keys``: the labelling's column keys (``group_keys[by]``), needed
    then; the result is a float64 tensor in their order (the YAML's doubles as they are, so that a group's fraction is
    formed from the same number as the scalar seed's).  A key that is no group of the labelling is an error."""
    scalar = seed_params["log_fraction_initial_cases"]
    by, listed = seed_params.get("by"), seed_params.get("log_fraction_by_group")
    if by is None:
        if listed:
            raise ValueError("infection_seed.log_fraction_by_group needs infection_seed.by (the agent attribute to group by)")
        return None, scalar
    check_group_name(by)
    if keys is None:
        raise ValueError(f"infection_seed.by = '{by}': no such labelling")
    index = {str(k): i for i, k in enumerate(keys)}
    out = torch.full((len(index),), float(scalar), dtype=torch.float64)
    for k, v in (listed or {}).items():
        if str(k) not in index:
            raise ValueError(f"infection_seed.log_fraction_by_group: '{k}' is no value of the agents' '{by}' "
                             f"({len(index)} groups, e.g. {list(index)[:5]})")
        out[index[str(k)]] = float(v)
    return by, out
