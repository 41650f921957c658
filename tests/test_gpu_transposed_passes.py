"""GPU: the backward's transposed sparse passes (gj_step_params.transpose = 1) element by element, per tile layout.

The backward of a step runs the SAME tiled phases as the forward with the per-network weights of the two passes
exchanged, on a signed cotangent.  Here those phases are driven directly (as autograd._transposed_passes drives them:
quarantine_transmission, step_phase 8, step_phase 4) and through autograd._transposed_passes itself, and every venue's
cum' and every agent's tbar is held to the float64 restatement of gj_testlib.sparse_passes_fp64 - which
tests/test_transposed_reference.py pins to torch.autograd through the oracle - within the PER-ELEMENT bound that
gj_testlib.sparse_pass_bounds derives from the number formats (no global tolerance, no "largest gradient" scale).

Independently of any restatement: <y, L t> == <L^T y, t> from the device outputs (a table exchanged at only one of the
three `transpose` sites of csrc/gj_tiled.h breaks it), bit-identity of the transposed results across tile geometries,
gj_adjoint_beta_partial / _finish against their formula on synthetic inputs of up to 300 000 venues, the CSR plan's
refusal, values beyond the fixed-point windows with either sign, and the public API under a changed geometry.

Layout forms that run with transpose = 1 here (asserted on the plans' own fields in
test_every_layout_form_runs_transposed and in the medium-world tests): workspace form of phases C + D (ell_k == 0),
direct form (ell_k > 0) with one and with several venue groups, pass 1 in the direct form (presum), narrow, wide and
explicit-slot descriptors, multi_slots rows, the run form, the split epilogue, several venue blocks per set; and, in
test_chunks_without_slot_rows_walk_the_tile_tables, narrow and wide descriptors without the rows (the table walk)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gj_testlib as L
from grad_june_amd import tiling as TL
from test_gpu_golden_parity import LAYOUT_IDS, LAYOUTS, engine_for
from test_gpu_random_worlds import random_layout, random_world
from test_transposed_reference import june769_case, qmask_of, signed_vector

pytestmark = pytest.mark.gpu

TILED = [(l, i) for l, i in zip(LAYOUTS, LAYOUT_IDS) if l[0] == "tiled"]
RUN_FORM = ("tiled", dict(runs=("household",), slices="small"))      # the household set forced into the run form
LAYOUTS_T = [l for l, _ in TILED] + [RUN_FORM]
IDS_T = [i for _, i in TILED] + ["tiled-run-form-households"]
CASES_769 = [(d, q) for d in (0, 1) for q in (False, True)]


# ---- worlds ------------------------------------------------------------------------------------------------------------
def household_major_case(case):
    """The case with the agents renumbered household-major (what the run form needs): per-agent arrays permuted."""
    from test_gpu_run_form import household_major

    w = case["world"]
    hh = w["edge_sets"]["household"]
    order, new_of = household_major(hh["agent"].numpy(), hh["venue"].numpy(), w["n_agents"])
    world = {"n_agents": w["n_agents"], "age": w["age"][torch.from_numpy(order)], "sex": w["sex"][torch.from_numpy(order)],
             "edge_sets": {k: {"agent": torch.from_numpy(new_of[v["agent"].numpy()]), "venue": v["venue"],
                               "people": v["people"]} for k, v in w["edge_sets"].items()}}
    return dict(case, world=world, stage=None if case["stage"] is None else case["stage"][order])


_CASES = {}


def case_769(day_type, quarantine, run_form=False):
    key = (day_type, quarantine, run_form)
    if key not in _CASES:
        c = june769_case(day_type, quarantine)
        _CASES[key] = household_major_case(c) if run_form else c
    return _CASES[key]


def build(case, layout, device):
    return engine_for(case["world"], case["tables"], device, layout)


def reference(case, key, vec, transpose, scale=1.0):
    """The restatement with its bounds, computed once per (case, vector, direction, scale) and shared by the layouts
    (kept in the case itself)."""
    k = (key, transpose, scale)
    refs = case.setdefault("_refs", {})
    if k not in refs:
        refs[k] = L.sparse_passes_with_bounds(case["world"], case["active"], case["betas"], case["tables"],
                                          case["day_type"], qmask_of(case), vec, transpose=transpose, scale=scale)
    return refs[k]


# ---- driving the engine ------------------------------------------------------------------------------------------------
def params_of(engine, case):
    has_q = case["stage"] is not None
    return engine.params(now=1.0, delta_time=1.0, day_type=case["day_type"], active=case["active"], betas=case["betas"],
                         has_quarantine=has_q, q_threshold=case["q_thr"] if has_q else math.inf)


def buffers_of(engine, case, vec, device, susceptibility=None):
    from grad_june_amd.engine import AgentBuffers

    n = engine.plan.host.n_agents
    x = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).to(device)
    stage = None if case["stage"] is None else torch.from_numpy(case["stage"]).to(device)
    susc = torch.ones(n, device=device) if susceptibility is None else susceptibility
    return AgentBuffers(engine.plan, susceptibility=susc, transmission=x, current_stage=stage), x


def cum_per_network(engine, case):
    out, per_set = {}, {}
    for name in case["active"]:
        es = engine.plan.networks[name].edge_set
        k = per_set.get(es, 0)
        per_set[es] = k + 1
        out[name] = engine.plan.cum_of(es)[:, k].clone()
    return out


def run_passes(engine, case, vec, device, transpose=1, susceptibility=None):
    """The three calls of autograd._transposed_passes on `vec`: ({network: cum}, per-agent result)."""
    p = params_of(engine, case)
    p.transpose = transpose
    bufs, _ = buffers_of(engine, case, vec, device, susceptibility)
    out = torch.full((engine.plan.host.n_agents,), float("nan"), device=device)
    io = engine.io(trans_susc=out)
    engine.quarantine_transmission(bufs, p)
    engine.step_phase(bufs, p, io, 8)
    cum = cum_per_network(engine, case)
    engine.step_phase(bufs, p, io, 4)
    torch.cuda.synchronize()
    return cum, out


def within(got, want, bound, what):
    """Every single element within ITS bound (a NaN fails)."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond their bound; worst at {i}: got "
                             f"{got[i]!r}, want {want[i]!r}, error {err[i]:.3e}, bound {bound[i]:.3e}")
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def check_parity(engine, case, key, vec, device, what):
    ref = reference(case, key, vec, True)
    cum, tbar = run_passes(engine, case, vec, device)
    worst = 0.0
    for n in case["active"]:
        worst = max(worst, within(cum[n], ref["cum"][n], ref["cum_bound"][n], f"{what} cum'/{n}"))
    worst = max(worst, within(tbar, ref["out"], ref["out_bound"], f"{what} tbar"))
    assert np.abs(ref["out"]).max() > 0
    return worst


def beta_gradient_reference(case, fwd, bwd):
    """ln(10) * sum_v [p_contact > 0] cum_n[v] cum'_n[v] / (beta_n p_contact[v]) from the two restatements, and its
    bound: the product rule on the per-venue bounds, 1e-12 of sum |terms| for the fp64 sum and one float32 rounding."""
    want, bound = {}, {}
    for n in case["active"]:
        bp = fwd["bp"][n]
        ok = bp > 0
        cf, cb, ef, eb = fwd["cum"][n][ok], bwd["cum"][n][ok], fwd["cum_bound"][n][ok], bwd["cum_bound"][n][ok]
        terms = cf * cb / bp[ok]
        want[n] = math.log(10.0) * float(np.sum(terms))
        bound[n] = (math.log(10.0) * float(np.sum((np.abs(cf) * eb + np.abs(cb) * ef + ef * eb) / bp[ok])
                                         + 1e-12 * np.sum(np.abs(terms))) + L.U32 * abs(want[n])) * L.SLACK
    return want, bound


def check_through_autograd(engine, case, key, vec, t, device, what):
    """autograd._forward_sums on t, then autograd._transposed_passes on `vec` (any magnitude): tbar, cum' and the beta
    gradients against the restatement of the vector the kernels saw (vec / its power-of-two scale)."""
    from grad_june_amd import autograd as AG

    n = engine.plan.host.n_agents
    nets = [SimpleNamespace(name=nm) for nm in case["active"]]
    p = params_of(engine, case)
    bufs, scratch = buffers_of(engine, case, t, device)
    acc = torch.empty(n, device=device)
    cum_fwd = AG._forward_sums(engine, p, bufs, acc, nets, compute_transmission=False)
    x = torch.from_numpy(vec).to(device)
    scale = float(AG._power_of_two_scale(x.abs().max()))
    assert 0.5 <= float(np.abs(vec).max()) / scale <= 1.0 and math.log2(scale) == round(math.log2(scale))
    tbar, grads = AG._transposed_passes(engine, p, bufs, scratch, x, nets, case["betas"], cum_fwd)
    assert p.transpose == 0
    cum = cum_per_network(engine, case)                  # cum' of vec / scale is left in the plan
    torch.cuda.synchronize()
    fwd = reference(case, "t", t, False)
    bwd = reference(case, key, vec, True, scale)
    within(acc, fwd["out"], fwd["out_bound"], f"{what} forward sums")
    within(tbar, bwd["out"], bwd["out_bound"], f"{what} tbar")
    for nm in case["active"]:
        within(cum[nm] * scale, bwd["cum"][nm], bwd["cum_bound"][nm], f"{what} cum'/{nm}")
    want, bound = beta_gradient_reference(case, fwd, bwd)
    for nm, g in zip(case["active"], grads):
        assert g.dtype == torch.float32
        assert abs(float(g) - want[nm]) <= bound[nm], (what, nm, float(g), want[nm], bound[nm])
    assert max(abs(w) for w in want.values()) > 0


def vectors(n, seed=3):
    x = signed_vector(n, seed)
    t = np.abs(signed_vector(n, seed + 1))
    return x, t


# ---- 2. element-wise parity in every tiled layout ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS_T, ids=IDS_T)
def test_transposed_passes_on_the_reference_world(device, layout):
    """The 769-agent world, eleven networks (care_visit: the one network whose two weights differ), both day types,
    quarantine off and on: cum' of every venue and network and tbar of every agent within their bounds - by the direct
    engine calls on max |x| = 1, and through autograd._transposed_passes on x * 1e5 and x * 1e-10 with the beta
    gradients."""
    run_form = layout is RUN_FORM
    engines = {}
    for day_type, quarantine in CASES_769:
        case = case_769(day_type, quarantine, run_form)
        if "e" not in engines:
            engines["e"] = build(case, layout, device)
        engine = engines["e"]
        x, t = vectors(case["world"]["n_agents"])
        what = f"day {day_type} quarantine {quarantine}"
        check_parity(engine, case, "x", x, device, what)
        for mag in (1e5, 1e-10):
            check_through_autograd(engine, case, ("x", mag), (x * np.float32(mag)).astype(np.float32), t, device,
                                   f"{what} x{mag:g}")
    if run_form:
        t_ = {s.name: s.tiled for s in engine.plan.host.sets}["household"]
        assert t_.runs is not None and t_.runs.n_primary > 700


def forms_of(host, split_epilogue=False):
    f = set()
    for s in host.sets:
        t = s.tiled
        f.add("direct" if t.ell_k else "workspace")
        f.add("explicit" if t.slot_idx is not None and t.n_edges > 0 else ("wide" if t.desc_wide else "narrow"))
        if t.multi_slots is not None and len(t.multi_slots):
            f.add("multi_slots")
        if TL.walk_share(t) > 0:
            f.add("walk")
        if t.runs is not None:
            f.add("runs")
        if t.presum:
            f.add("presum")
        if t.n_blocks > 1:
            f.add("blocks>1")
    if split_epilogue:
        f.add("split_epilogue")
    return f


def test_every_layout_form_runs_transposed(device):
    """The parametrisation above really reaches every form (on the plans' own fields): a silent fall-back to one form
    would hollow the coverage out."""
    seen = set()
    for layout in LAYOUTS_T:
        case = case_769(0, False, layout is RUN_FORM)
        e = build(case, layout, device)
        seen |= forms_of(e.plan.host, e.plan.agent_scratch is not None)
        if layout[1].get("direct_table_floats"):
            assert e.plan.tiled_c.direct_table_floats == layout[1]["direct_table_floats"]
    assert seen >= {"direct", "workspace", "narrow", "wide", "explicit", "multi_slots", "runs", "presum", "blocks>1",
                    "split_epilogue"}, seen


# Geometries of the reference world in which most household and company chunks span more tiles than their descriptor
# expresses (tiling.walk_share: narrow 75 % / 91 %, wide 67 % / 73 %).  desc_explicit=False keeps the wide one on
# descriptors (by itself it would switch to explicit slots).
WALK_GEOMETRIES = [dict(sv_max=64, eb_target=512, slices="small", desc_wide=False, direct=False),
                   dict(sv_max=16, eb_target=64, slices="small", desc_wide=True, desc_explicit=False, direct=False)]


def test_chunks_without_slot_rows_walk_the_tile_tables(device, monkeypatch):
    """A plan whose descriptors mark "multi" chunks and whose gj_tiled_set.multi_slots is NULL (valid input by
    include/gradjune_hip.h; what build_tiled(multi_rows=False) gives): the lanes of such a chunk walk the tile tables in
    phases A and D - narrow descriptors (chunk_slot_slow) and wide ones (chunk_slot_walk).  Next to it the same geometry
    with the rows of explicit slots - for the wide descriptors the only layout that has rows at all.  Both resolve the
    same slots and the sums are integer: per-element parity for each, forward and transposed, quarantine off and on, and
    cum and the per-agent result bit for bit the same."""
    import functools

    real = TL.build_tiled
    for geometry in WALK_GEOMETRIES:
        engines = {}
        for rows in (True, False):
            with monkeypatch.context() as m:
                if not rows:
                    m.setattr(TL, "build_tiled", functools.partial(real, multi_rows=False))
                engines[rows] = build(case_769(0, False), ("tiled", geometry), device)
        tiled = {rows: {s.name: s.tiled for s in e.plan.host.sets} for rows, e in engines.items()}
        for name in ("household", "company"):
            walk, with_rows = tiled[False][name], tiled[True][name]
            assert walk.multi_slots is None and TL.walk_share(walk) > 0.5, (geometry, name, TL.walk_share(walk))
            assert with_rows.multi_slots is not None and len(with_rows.multi_slots) > 0, (geometry, name)
            for t in (walk, with_rows):
                assert t.slot_idx is None and bool(t.desc_wide) == geometry["desc_wide"], (geometry, name)
        assert "walk" in forms_of(engines[False].plan.host) and "walk" not in forms_of(engines[True].plan.host)
        for quarantine in (False, True):
            case = case_769(0, quarantine)
            x = signed_vector(case["world"]["n_agents"], 3)
            for transpose in (0, 1):
                what = f"{geometry} quarantine {quarantine} transpose {transpose}"
                ref, got = reference(case, "x", x, bool(transpose)), {}
                for rows, engine in engines.items():
                    if transpose:
                        check_parity(engine, case, "x", x, device, f"{what} rows {rows}")
                    got[rows] = cum, out = run_passes(engine, case, x, device, transpose=transpose)
                    for n in case["active"]:          # (check_parity's checks, for either direction)
                        within(cum[n], ref["cum"][n], ref["cum_bound"][n], f"{what} rows {rows} cum/{n}")
                    within(out, ref["out"], ref["out_bound"], f"{what} rows {rows} per agent")
                for n in case["active"]:
                    assert torch.equal(got[True][0][n], got[False][0][n]), (what, n)
                assert torch.equal(got[True][1], got[False][1]), what


# ---- 3. the adjoint identity ----------------------------------------------------------------------------------------------
def check_adjoint_identity(engine, case, key, y, t, device, what):
    """<y, L t> == <L^T y, t> in float64 from the device outputs, within sum |y| E2_forward + sum |t| E2_transposed."""
    _, lt = run_passes(engine, case, t, device, transpose=0)
    _, lty = run_passes(engine, case, y, device, transpose=1)
    a = float(np.dot(y.astype(np.float64), lt.cpu().numpy().astype(np.float64)))
    b = float(np.dot(lty.cpu().numpy().astype(np.float64), t.astype(np.float64)))
    fwd, bwd = reference(case, (key, "t"), t, False), reference(case, (key, "y"), y, True)
    bound = float(np.dot(np.abs(y), fwd["out_bound"]) + np.dot(np.abs(t), bwd["out_bound"]))
    assert abs(a - b) <= bound, (what, a, b, abs(a - b), bound)
    return abs(a)


@pytest.mark.parametrize("layout", LAYOUTS_T, ids=IDS_T)
def test_adjoint_identity_on_the_reference_world(device, layout):
    run_form = layout is RUN_FORM
    engine, size = None, 0.0
    for day_type, quarantine in CASES_769:
        case = case_769(day_type, quarantine, run_form)
        engine = engine or build(case, layout, device)
        n = case["world"]["n_agents"]
        y, t = signed_vector(n, 11), np.abs(signed_vector(n, 12, zeros=0.5))
        size = max(size, check_adjoint_identity(engine, case, "adj", y, t, device, f"day {day_type} q {quarantine}"))
    assert size > 0


# ---- random worlds ------------------------------------------------------------------------------------------------------
SEED_BASE = 3000          # (no draw of these 40 is without a network: checked by test_random_draws_have_networks)


def random_case(seed):
    rng = np.random.default_rng(SEED_BASE + seed)
    world = random_world(rng)
    A = world["n_agents"]
    tables = {n: torch.from_numpy(rng.random((2, 2, 100)).astype(np.float32)) for n in L.LEISURE + ("care_visit",)
              if rng.random() < 0.8}
    specs = L.network_specs(world, tables)
    if not specs:
        return None
    active = [s.name for s in specs if rng.random() < 0.8] or [specs[0].name]
    betas = {n: float(np.float32(rng.uniform(0.1, 40.0))) for n in active}
    quarantine = rng.random() < 0.5
    stage = rng.integers(1, 7, A).astype(np.float32) if quarantine else None
    layout = random_layout(rng, A)
    while layout[0] == "csr":
        layout = random_layout(rng, A)
    case = dict(world=world, tables=tables, active=active, betas=betas, day_type=int(rng.integers(0, 2)), stage=stage,
                q_thr=float(rng.choice([2.0, 3.0, 4.0])) if quarantine else None)
    return case, layout


def test_random_draws_have_networks():
    """At most 4 of the 40 draws may be skipped for having no network (the generators run without a GPU)."""
    assert sum(random_case(seed) is None for seed in range(40)) <= 4


@pytest.mark.parametrize("seed", range(40))
def test_transposed_passes_on_random_worlds(device, seed):
    """Random small worlds (empty sets, unattended venues, `people` != degree, duplicated edges, one giant venue) in
    random tile geometries, a random subset of the networks: parity per element and the adjoint identity."""
    draw = random_case(seed)
    if draw is None:
        pytest.skip("the draw has no network on any of its sets")
    case, (name, kw) = draw
    engine = L.make_engine(case["world"], case["tables"], device, layout=name, **kw)
    n = case["world"]["n_agents"]
    x, t = signed_vector(n, seed), np.abs(signed_vector(n, 100 + seed, zeros=0.5))
    what = f"seed {seed}: {n} agents, active {case['active']}, q {case['q_thr']}, {kw}"
    ref = reference(case, "x", x, True)
    cum, tbar = run_passes(engine, case, x, device)
    for nm in case["active"]:
        within(cum[nm], ref["cum"][nm], ref["cum_bound"][nm], f"{what} cum'/{nm}")
    within(tbar, ref["out"], ref["out_bound"], f"{what} tbar")
    check_adjoint_identity(engine, case, "adj", x, t, device, what)


# ---- the medium world -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium():
    """make_world("june", 100 000 agents, clustered): eleven networks incl. care_visit, 300 000 leisure edges.  Built once
    per module, agents household-major (so that the run form is possible); a quarantine policy on random stages."""
    import bench as B
    from grad_june_amd.synthetic import make_world, reorder_agents

    w = reorder_agents(make_world("june", n_agents=100_000, geography="clustered"), by="household")
    specs = B.network_specs(w)
    rng = np.random.default_rng(5)
    world = {"n_agents": w["n_agents"], "age": torch.from_numpy(w["age"]), "sex": torch.from_numpy(w["sex"]),
             "edge_sets": {k: {kk: torch.from_numpy(np.ascontiguousarray(vv)) for kk, vv in v.items()}
                           for k, v in w["edge_sets"].items()}}
    tables = {s.name: torch.from_numpy(np.asarray(s.table, dtype=np.float32).reshape(2, 2, 100)) for s in specs
              if s.table is not None}
    active = [n for n in L.HIERARCHY if n in w["networks"]]
    assert "care_visit" in active and len(active) == 11
    betas = {n: float(np.float32(4.0 * v)) for n, v in B.betas_of(w).items()}
    case = dict(world=world, tables=tables, active=active, betas=betas, day_type=0,
                stage=rng.integers(1, 7, w["n_agents"]).astype(np.float32), q_thr=4.0)
    x, t = vectors(w["n_agents"], seed=21)
    return case, x, t


MEDIUM_GEOMETRIES = [{}, dict(sv_max=256, eb_target=2048, slices=(-(-100_000 // 1024), 1024))]


@pytest.mark.parametrize("geometry", MEDIUM_GEOMETRIES, ids=["default", "small-tiles-1024-agent-slices"])
def test_transposed_passes_on_the_medium_world(device, medium, geometry):
    """One transposed step on 100 000 agents in the default geometry and in small tiles with 1024-agent slices (wide and
    explicit descriptors, a multi_slots row, up to 163 venue blocks per set): parity per element, the beta gradients
    through autograd._transposed_passes, and the adjoint identity."""
    case, x, t = medium
    engine = L.make_engine(case["world"], case["tables"], device, layout="tiled", runs=False, **geometry)
    forms = forms_of(engine.plan.host)
    assert {"direct", "workspace", "blocks>1"} <= forms
    if geometry:
        assert {"wide", "explicit", "multi_slots"} <= forms, forms
    check_parity(engine, case, "x", x, device, "medium")
    check_through_autograd(engine, case, ("x", 1e5), (x * np.float32(1e5)).astype(np.float32), t, device, "medium x1e5")
    check_adjoint_identity(engine, case, "adj", x, t, device, "medium")


# ---- 4. bit-identity across geometries -----------------------------------------------------------------------------------
def test_tile_geometry_cannot_change_a_bit_of_the_transposed_pass(device, medium):
    """The analogue of test_gpu_api.py::test_tile_geometry_cannot_change_a_bit for transpose = 1 on the medium world:
    every tuner candidate (world.TUNE_CANDIDATES, GEOMETRY_CANDIDATES without direct=False), tiny tiles, presum and
    explicit slots give bitwise the same tbar, cum' and beta gradients as the defaults - half of them compiled on the
    device.  The candidates that change the FORM of pass 2 for a set - direct=False (the forward test leaves it out: the
    workspace form adds an agent's terms in fixed point, the direct form in float32) and the run form of the households
    - keep cum' and the beta gradients bit for bit (pass 1 is fixed point in every form) and hold tbar to the
    per-element bound."""
    from grad_june_amd import autograd as AG
    from grad_june_amd import world as W
    from grad_june_amd.benchrun import GEOMETRY_CANDIDATES

    case, x, t = medium
    A = case["world"]["n_agents"]
    cands = [dict(c) for c in W.TUNE_CANDIDATES] + [dict(c) for c in GEOMETRY_CANDIDATES if "direct" not in c]
    cands += [{"eb_target": 4096, "sv_max": 64, "slice_agents": 1024}, {"presum": True}, {"desc_explicit": True}]
    other_form = [{"eb_target": 131072, "sv_max": 16384, "direct": False}, {"runs": ("household",)}]
    nets = [SimpleNamespace(name=nm) for nm in case["active"]]
    xd = torch.from_numpy(x).to(device)
    ref, seen, forms = None, set(), set()
    bound = reference(case, "x", x, True, float(2.0 ** math.ceil(math.log2(float(np.abs(x).max())))))
    for i, cand in enumerate(cands + other_form):
        cand = dict(cand)
        same_form = i < len(cands)
        sa = cand.pop("slice_agents", None)
        if sa is not None:
            cand["slices"] = (-(-A // sa), sa)
        cand.setdefault("runs", False)
        if i % 2:
            cand["device_compile"] = True
        engine = L.make_engine(case["world"], case["tables"], device, layout="tiled", **cand)
        p = params_of(engine, case)
        bufs, scratch = buffers_of(engine, case, t, device)
        cum_fwd = AG._forward_sums(engine, p, bufs, torch.empty(A, device=device), nets, compute_transmission=False)
        tbar, grads = AG._transposed_passes(engine, p, bufs, scratch, xd, nets, case["betas"], cum_fwd)
        got = {"tbar": tbar.clone(), "grads": torch.stack(grads).clone()}
        for hs in engine.plan.host.sets:
            got["cum'/" + hs.name] = engine.plan.cum_of(hs.name).clone()
        torch.cuda.synchronize()
        seen.add(tuple(hs.tiled.n_blocks for hs in engine.plan.host.sets) + (engine.plan.host.n_slices,))
        forms |= forms_of(engine.plan.host)
        if ref is None:
            ref = got
            assert float(tbar.abs().max()) > 0 and float(got["grads"].abs().min()) > 0
            continue
        for k in ref:
            if k == "tbar" and not same_form:
                within(got[k], bound["out"], bound["out_bound"], f"{cand} tbar")
            else:
                assert torch.equal(got[k], ref[k]), (cand, k)
    assert len(seen) >= 4          # the candidates really are different geometries
    assert {"presum", "explicit", "runs", "workspace", "direct"} <= forms, forms


# ---- 5. gj_adjoint_beta_partial / _finish against their formula ----------------------------------------------------------
def _beta_sets(rng, V, nk, stride, n_sets):
    sets = []
    for _ in range(n_sets):
        pc = (1.0 / rng.integers(1, 50, V)).astype(np.float32)
        pc[rng.random(V) < 0.2] = 0.0                                  # venues nobody can meet in
        sets.append(dict(fwd=rng.random((V, stride)).astype(np.float32) * 8.0,
                         bwd=rng.standard_normal((V, stride)).astype(np.float32),        # signed
                         pc=pc, w=rng.random(V), beta=rng.uniform(0.1, 40.0, nk).astype(np.float32)))
    return sets


@pytest.mark.parametrize("nk", [1, 6, 8])
@pytest.mark.parametrize("V", [1, 1023, 1024, 1025, 256 * 1024 + 1, 300_000])
def test_adjoint_beta_kernels_against_their_formula(device, V, nk):
    """ln(10) * scale * sum_v [p_contact > 0] cum_fwd * cum_bwd / (beta * p_contact) * weight (autograd._beta_gradients)
    in float64 numpy on the same float32 inputs.  The kernel adds fp64 terms of exactly represented inputs - only the
    order of the additions (1024 lanes x GJ_ADJ_BETA_BLOCKS workgroups) differs from numpy's: 1e-12 * sum |terms| per
    network.  Venue counts around the workgroup width and the grid, nk up to GJ_MAX_NETS_PER_SET, a stride larger than nk
    (the ABI bounds the stride by GJ_MAX_NETS_PER_SET, so nk = 8 runs at stride 8), two sets into shared and into
    disjoint columns, with and without the fp64 weights; a second call gives the same bits."""
    import ctypes as C

    from grad_june_amd import _native as N

    assert (N.GJ_ADJ_BETA_BLOCKS, N.GJ_MAX_NETS_PER_SET) == (256, 8)
    lib = N.load()
    stride = min(N.GJ_MAX_NETS_PER_SET, nk + 2)
    rng = np.random.default_rng(V * 10 + nk)
    sets = _beta_sets(rng, V, nk, stride, 2)
    scale = np.float32(2.0 ** -3)
    dev = [{k: torch.from_numpy(v).to(device).contiguous() for k, v in s.items() if k != "beta"} for s in sets]
    for weights in (False, True):
        for shared in (True, False):
            if not shared and 2 * nk > N.GJ_MAX_NETS:
                cols = [list(range(nk)), list(range(N.GJ_MAX_NETS - nk, N.GJ_MAX_NETS))]
            else:
                cols = [list(range(nk)), list(range(nk)) if shared else list(range(nk, 2 * nk))]
            n_cols = max(max(c) for c in cols) + 1
            want, mass = np.zeros(n_cols), np.zeros(n_cols)
            for s, cs in zip(sets, cols):
                ok = s["pc"] > 0
                for k, c in enumerate(cs):
                    terms = (s["fwd"][ok, k].astype(np.float64) * s["bwd"][ok, k].astype(np.float64)
                             / (np.float64(s["beta"][k]) * s["pc"][ok].astype(np.float64))
                             * (s["w"][ok] if weights else 1.0))
                    want[c] += math.fsum(terms)
                    mass[c] += float(np.abs(terms).sum())
            want, mass = want * float(scale) * math.log(10.0), mass * float(scale) * math.log(10.0)
            outs = []
            for _ in range(2):
                partial = torch.zeros(N.GJ_ADJ_BETA_BLOCKS * N.GJ_MAX_NETS, dtype=torch.float64, device=device)
                out = torch.full((N.GJ_MAX_NETS,), -7.0, dtype=torch.float64, device=device)
                for s, d, cs in zip(sets, dev, cols):
                    N.check(lib.gj_adjoint_beta_partial(V, stride, nk, N.ptr(d["fwd"]), N.ptr(d["bwd"]), N.ptr(d["pc"]),
                                                        N.ptr(d["w"]) if weights else None, (C.c_float * nk)(*[float(b) for b in s["beta"]]),
                                                        (C.c_int32 * nk)(*cs), N.ptr(partial), N.current_stream()),
                            "gj_adjoint_beta_partial")
                sc = torch.tensor([scale], device=device)
                N.check(lib.gj_adjoint_beta_finish(n_cols, N.ptr(partial), N.ptr(sc), N.ptr(out), N.current_stream()),
                        "gj_adjoint_beta_finish")
                torch.cuda.synchronize()
                outs.append(out.cpu().numpy())
            assert np.array_equal(outs[0], outs[1])
            assert (outs[0][n_cols:] == -7.0).all()                   # columns nobody asked for are not written
            err = np.abs(outs[0][:n_cols] - want)
            assert (err <= 1e-12 * mass).all(), (V, nk, weights, shared, err, 1e-12 * mass)
            assert V < 64 or (mass > 0).all()


# ---- 6. small items -----------------------------------------------------------------------------------------------------
def test_transpose_on_a_csr_plan_is_refused_and_writes_nothing(device):
    """transpose = 1 on a plan without the tiled layout: every entry that runs a sparse pass returns GJ_E_PLAN and
    launches nothing (the outputs, the per-venue sums and the per-agent inputs keep their sentinel / their values)."""
    import ctypes as C

    from grad_june_amd import _native as N

    case = case_769(0, True)
    engine = build(case, ("csr", {}), device)
    lib = N.load()
    p = params_of(engine, case)
    p.transpose = 1
    x = signed_vector(case["world"]["n_agents"], 3)
    bufs, xbuf = buffers_of(engine, case, x, device)
    engine._prep(bufs, p)
    n = engine.plan.host.n_agents
    outs = [torch.full((n,), -7.0, device=device) for _ in range(3)]
    io = engine.io(not_infected_probs=outs[0], trans_susc=outs[1], new_infected=outs[2])
    cum_before = [c.clone().fill_(-7.0) for c in engine.plan.cum]
    for c in engine.plan.cum:
        c.fill_(-7.0)
    q_before = bufs.tensors["q_transmission"].fill_(-7.0).clone()
    args = (C.byref(engine.plan.c), C.byref(bufs.c), C.byref(p))
    assert lib.gj_venue_reduce(*args, N.current_stream()) == -3                       # GJ_E_PLAN
    assert lib.gj_agent_gather(*args, C.byref(io), 0, N.current_stream()) == -3
    assert lib.gj_step(*args, C.byref(io), N.current_stream()) == -3
    for phase in (8, 4):
        assert lib.gj_step_phase(*args, C.byref(io), phase, N.current_stream()) == -3
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)
    assert all(torch.equal(a, b) for a, b in zip(engine.plan.cum, cum_before))
    assert torch.equal(bufs.tensors["q_transmission"], q_before)
    assert torch.equal(xbuf.cpu(), torch.from_numpy(x))
    p.transpose = 0                                                                   # the same call is fine forward
    assert lib.gj_step_phase(*args, C.byref(io), 4, N.current_stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["workspace-form", "direct-form", "run-form"])
def test_signed_terms_beyond_the_windows(device, form):
    """The contract of csrc/gj_tiled.h:65-71 for NEGATIVE values, which only a cotangent brings: a term below the window
    of pass 1 (|term| <= 16 384) makes its venue read -1e30 (times beta * p_contact), a negative and a positive one on one
    venue NaN, and a zero factor downstream (p_contact of an empty venue, a susceptibility of 0) still gives 0.  Pass 2's
    window (|value| <= 262 144) exists in the workspace form, whose per-agent sums are fixed point: a venue value below
    it reads -1e30 for its agents, two of opposite sign NaN; the direct form adds an agent's values in float32 and returns
    the sum itself.  So does the run form for an agent's primary edge (its first edge to its smallest venue); what is left
    of the set - here agent 12's edge to venue 7 - goes through the workspace and saturates.  Households of two
    (p_contact = 1), beta = 40; the values are finite and just beyond the windows.  The agents are numbered
    household-major, so a plan without the direct form takes the run form unless it is told not to (runs=False)."""
    n, V = 256, 128
    agent = np.arange(n)
    venue = agent // 2
    agent = np.concatenate([agent, [12]])               # agent 12 also attends venue 7 (agents 14, 15)
    venue = np.concatenate([venue, [7]])
    people = np.full(V, 2)
    people[2] = 0                                       # p_contact = clamp(1 / -1, 0, 1) = 0
    people[7] = 2
    world = {"n_agents": n, "age": torch.zeros(n, dtype=torch.int64), "sex": torch.zeros(n, dtype=torch.int64),
             "edge_sets": {"household": {"agent": torch.from_numpy(agent), "venue": torch.from_numpy(venue),
                                         "people": torch.from_numpy(people)}}}
    case = dict(world=world, tables=None, active=["household"], betas={"household": 40.0}, day_type=0, stage=None,
                q_thr=None)
    kw = {"workspace-form": dict(direct=False, runs=False), "direct-form": {}, "run-form": dict(runs=("household",))}[form]
    engine = L.make_engine(world, None, device, layout="tiled", **kw)
    tiled = engine.plan.host.sets[0].tiled
    assert (tiled.ell_k > 0, tiled.runs is not None) == {"workspace-form": (False, False), "direct-form": (True, False),
                                                         "run-form": (False, True)}[form]
    x = np.zeros(n, dtype=np.float32)
    x[0] = -20000.0                                     # venue 0: one term below pass 1's window
    x[2], x[3] = -20000.0, 20000.0                      # venue 1: one below, one above
    x[4] = -20000.0                                     # venue 2: below the window, p_contact = 0
    x[8] = x[9] = -16000.0                              # venue 4: inside pass 1's window, 40 * -32000 is below pass 2's
    x[13], x[14] = -16000.0, 16000.0                    # venues 6 and 7: -640 000 and +640 000, both meet in agent 12
    x[20], x[21] = 3.0, -5.0                            # venue 10: ordinary
    susc = torch.ones(n, device=device)
    susc[9] = 0.0
    susc[1] = 0.0
    cum, tbar = run_passes(engine, case, x, device, susceptibility=susc)
    cum, tbar = cum["household"].cpu().numpy(), tbar.cpu().numpy()
    assert cum[0] == np.float32(40.0) * np.float32(-1e30)
    assert np.isnan(cum[1])
    assert cum[2] == 0.0
    assert (cum[4], cum[6], cum[7], cum[10]) == (-1280000.0, -640000.0, 640000.0, -80.0)
    assert tbar[0] <= -1e30 and tbar[1] == 0.0                          # saturated; times a susceptibility of 0
    assert np.isnan(tbar[2]) and np.isnan(tbar[3])
    assert tbar[4] == 0.0 and tbar[5] == 0.0
    assert tbar[9] == 0.0
    assert tbar[20] == -80.0 and tbar[21] == -80.0
    if form == "direct-form":
        assert tbar[8] == -1280000.0 and tbar[13] == -640000.0 and tbar[14] == 640000.0 and tbar[12] == 0.0
    elif form == "run-form":
        assert tbar[0] == np.float32(40.0) * np.float32(-1e30)
        assert tbar[8] == -1280000.0 and tbar[13] == -640000.0 and tbar[14] == 640000.0
        assert tbar[12] == np.float32(1e30)             # venue 7 through the workspace: saturated; plus -640 000 of venue 6
    else:
        assert tbar[0] == np.float32(-1e30) and tbar[8] == np.float32(-1e30) and tbar[13] == np.float32(-1e30)
        assert tbar[14] == np.float32(1e30) and np.isnan(tbar[12])
    rest = np.ones(n, dtype=bool)
    rest[[0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 15, 20, 21]] = False
    assert (tbar[rest] == 0.0).all()


@pytest.mark.parametrize("seed", [1])
def test_api_gradients_do_not_depend_on_the_tile_geometry(device, seed, monkeypatch):
    """Three chained GradJune.hot_path steps on a random world with injected noise, the profile leaves requiring
    gradients: the per-agent profile gradients and the log_beta gradients are bit for bit the same under the default
    geometry (world.TUNE = "0") and under tiny tiles with 64-agent slices, chosen through the tuner's own knob
    (world.TUNE = "auto" with that geometry as its only candidate)."""
    import gj_oracle as O
    import grad_june_amd as G
    from grad_june_amd import world as W
    from test_gpu_parameter_gradients import PROFILE, _run_random_world

    A = random_world(np.random.default_rng(9500 + seed))["n_agents"]
    tiny = {"sv_max": 16, "eb_target": 64, "slices": (-(-A // 64), 64)}
    results, shapes = [], []
    for tune in ("0", "auto"):
        monkeypatch.setattr(W, "TUNE", tune)
        monkeypatch.setattr(W, "TUNE_CANDIDATES", (tiny,))
        monkeypatch.setattr(W, "TUNE_MIN_EDGES", 0)
        made = []
        real = W.DevicePlan

        def spy(host, *a, **k):
            made.append((host.n_slices,) + tuple(s.tiled.n_blocks for s in host.sets))
            return real(host, *a, **k)

        monkeypatch.setattr(W, "DevicePlan", spy)
        run = _run_random_world(G, O, device, seed, profile_leaves=True, oracle=False)
        monkeypatch.setattr(W, "DevicePlan", real)
        assert run is not None
        hip_series, _, ps, _, dev, _, names = run
        loss = torch.stack(hip_series).sum()
        assert loss.requires_grad
        loss.backward()
        results.append([p.grad.clone() for p in ps] + [dev[k].grad.clone() for k in PROFILE])
        shapes.append(made[-1])
        assert any(n in L.LEISURE or n == "care_visit" for n in names), names
    assert shapes[0] != shapes[1], shapes              # the knob really changed the geometry
    assert any(float(g.abs().max()) > 0 for g in results[0][len(results[0]) - 4:])
    for a, b in zip(*results):
        assert torch.equal(a, b)
