"""CPU: the launch layer's validation, pinned code by code.

The library loads without a GPU and the host never dereferences the device pointers of a plan, so a hand-built
``Plan`` / ``Tiled`` / ``StepParams`` whose pointers hold a fake non-null value exercises every check that comes before
a launch.  EVERY case here is rejected with a negative code before the first launch of its call (on a machine with a
GPU a case that passed validation would launch on the fake pointers): each assertion is ``< 0`` first, then the code.
The codes are those of the library before the launch layer's network classification, grid and alignment helpers were
shared; they are part of the ABI's behaviour and must not move.

Not pinned, because no input reaches it: ``tiled_agents``' "more than GJ_MAX_DIRECT direct sets" check.  GJ_MAX_DIRECT
equals GJ_MAX_SETS and a set forms at most one group of networks (a second group of the same set is "not adjacent"),
so the counter it guards never exceeds GJ_MAX_SETS - 1 when it is tested.
"""
import ctypes as C

import pytest

from grad_june_amd import _native as N

OK, E_NULL, E_RANGE, E_PLAN = 0, -1, -2, -3         # include/gradjune_hip.h
FAKE = 0x10000                                        # 16-byte aligned, never dereferenced by the host
RAW, Q, QL, QL75 = N.MASK_RAW, N.MASK_Q, N.MASK_QL, N.MASK_QL_AGE75


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    import os

    if not os.path.exists(N.LIB_PATH):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(root, "__graft_entry__.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        m.build()
    return N.load()


def rejected(code, want):
    assert code < 0, f"passed validation (or launched): {code}"
    assert code == want


class Case:
    """One edge set of 4 venues / 8 edges with room for two networks (cum_stride 2), 64 agents, two leisure tables;
    a second, empty set.  ``tiled``: one slice, one work item, no e_cls, neither direct nor run form."""

    def __init__(self, tiled=True, n_agents=64):
        self.plan = N.Plan()
        p = self.plan
        p.n_agents, p.n_ext_agents, p.n_sets = n_agents, 64, 2
        s = p.sets[0]
        s.n_venues, s.n_edges, s.v_pcontact, s.cum, s.cum_stride = 4, 8, FAKE, FAKE, 2
        p.sets[1].cum_stride = 1
        p.agent_class, p.tables, p.n_tables = FAKE, FAKE, 2
        if tiled:
            self.tiled = N.Tiled()
            t = self.tiled
            t.n_slices, t.slice_agents, t.n_work, t.work = 1, 64, 1, FAKE
            ts = t.sets[0]
            ts.n_blocks, ts.max_block_venues = 1, 4
            for f in ("blk_v0", "blk_e0", "e_lv", "a_la", "tile_sptr", "tile_jpos", "chunk_ptr", "chunk_desc", "val"):
                setattr(ts, f, FAKE)
            p.tiled = C.pointer(t)
        else:
            s.v_rowptr = s.v_agent = s.a_rowptr = s.a_venue = FAKE
            p.sets[1].v_rowptr = p.sets[1].a_rowptr = FAKE
            p.n_blocks, p.blocks = 1, FAKE
        self.state = N.AgentState()
        for f in ("max_infectiousness", "shape", "rate", "shift", "infection_time", "is_infected", "susceptibility",
                  "transmission", "q_transmission", "current_stage"):
            setattr(self.state, f, FAKE)
        self.params = N.StepParams()
        self.params.delta_time = 1.0
        self.io = N.StepIO()

    @property
    def tset(self):
        return self.tiled.sets[0]

    def direct(self):                       # the set in the direct form of pass 2
        self.tset.ell_k, self.tset.ell = 2, FAKE
        return self

    def run_form(self):                     # the set in the run form
        ts = self.tset
        ts.run_pv_blk = ts.run_pv_win = ts.run_blk_r0 = ts.run_win_lo = ts.run_win_n = FAKE
        ts.run_max_window, ts.run_tiled_edges = 4, 4
        return self

    def nets(self, *nets):
        """(set, mask_kind[, table]) per network"""
        self.params.n_nets = len(nets)
        for i, n in enumerate(nets):
            x = self.params.nets[i]
            x.beta, x.set, x.mask_kind, x.table = 1.0, n[0], n[1], (n[2] if len(n) > 2 else 0)
        return self

    def phase(self, lib, phase):
        return lib.gj_step_phase(C.byref(self.plan), C.byref(self.state), C.byref(self.params), C.byref(self.io), phase,
                                 None)


# ---- the rule "a leisure set has a table for every network, any other set exactly one network" ---------------------
@pytest.mark.parametrize("phase", [6, 2])
def test_two_plain_networks_on_one_tiled_set(lib, phase):
    rejected(Case().nets((0, Q), (0, Q)).phase(lib, phase), E_PLAN)


@pytest.mark.parametrize("phase", [6, 2, 5])
def test_leisure_pair_without_edge_classes(lib, phase):
    rejected(Case().nets((0, QL, 0), (0, QL75, 1)).phase(lib, phase), E_PLAN)


@pytest.mark.parametrize("phase", [6, 2])
def test_masked_network_beside_a_leisure_one_tiled(lib, phase):
    c = Case().nets((0, Q), (0, QL, 1))
    c.tset.e_cls = FAKE
    rejected(c.phase(lib, phase), E_PLAN)


def test_masked_network_beside_a_leisure_one_csr(lib):
    c = Case(tiled=False).nets((0, QL, 1), (0, Q))
    rejected(c.phase(lib, 1), E_PLAN)
    rejected(lib.gj_venue_reduce(C.byref(c.plan), C.byref(c.state), C.byref(c.params), None), E_PLAN)


def test_two_plain_networks_on_a_direct_set(lib):
    rejected(Case().direct().nets((0, Q), (0, Q)).phase(lib, 3), E_PLAN)
    rejected(Case().direct().nets((0, QL, 0), (0, Q)).phase(lib, 4), E_PLAN)


# ---- group_networks: before anything else of a step ----------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 3, 6])
def test_raw_network_beside_a_masked_one(lib, phase):
    rejected(Case().nets((0, RAW), (0, Q)).phase(lib, phase), E_PLAN)
    rejected(Case().nets((0, Q), (0, RAW)).phase(lib, phase), E_PLAN)


def test_table_index_past_n_tables(lib):
    rejected(Case().nets((0, QL, 2)).phase(lib, 6), E_PLAN)
    rejected(Case().nets((0, QL, -1)).phase(lib, 6), E_PLAN)


def test_leisure_network_without_tables_or_classes(lib):
    for field in ("tables", "agent_class"):
        c = Case().direct().nets((0, QL, 0))
        setattr(c.plan, field, None)
        rejected(c.phase(lib, 3), E_PLAN)


def test_networks_of_one_set_that_are_not_adjacent(lib):
    rejected(Case().nets((0, Q), (1, Q), (0, Q)).phase(lib, 6), E_PLAN)
    rejected(Case(tiled=False).nets((0, Q), (1, Q), (0, Q)).phase(lib, 1), E_PLAN)


def test_more_networks_than_the_sets_cum_stride(lib):
    c = Case().nets((0, QL, 0), (0, QL, 1), (0, QL, 0))
    c.tset.e_cls = FAKE
    rejected(c.phase(lib, 6), E_PLAN)
    rejected(Case().nets((1, Q), (1, Q)).phase(lib, 6), E_PLAN)          # stride 1


def test_ranges_of_the_network_list(lib):
    rejected(Case().nets((2, Q)).phase(lib, 6), E_RANGE)                 # set past n_sets
    rejected(Case().nets((0, 4)).phase(lib, 6), E_RANGE)                 # mask kind
    c = Case().nets((0, Q))
    c.params.day_type = 2
    rejected(c.phase(lib, 6), E_RANGE)
    c = Case().nets((0, Q))
    c.params.n_nets = N.GJ_MAX_NETS + 1
    rejected(c.phase(lib, 6), E_RANGE)
    c = Case(tiled=False).nets((0, Q))
    c.params.transpose = 1                                               # the backward passes are the tiled layout's
    rejected(c.phase(lib, 1), E_PLAN)


def test_unknown_phase(lib):
    rejected(Case().nets((0, Q)).phase(lib, 99), E_RANGE)
    rejected(Case().nets((0, Q)).phase(lib, -1), E_RANGE)


# ---- phase 3: the direct and the run form of pass 2 ----------------------------------------------------------------
def test_direct_leisure_set_needs_dword_aligned_classes(lib):
    c = Case().direct().nets((0, QL, 0), (0, QL, 1))
    c.plan.agent_class = FAKE + 1
    rejected(c.phase(lib, 3), E_PLAN)
    rejected(c.phase(lib, 4), E_PLAN)


def test_run_form_window_pointer_alignment(lib):
    c = Case().run_form().nets((0, Q))
    c.tset.run_pv_win = FAKE + 4
    rejected(c.phase(lib, 3), E_PLAN)


# ---- phase 5: the run form of pass 1 -------------------------------------------------------------------------------
def test_run_form_without_the_per_agent_values(lib):
    c = Case(n_agents=0).run_form().nets((0, Q))        # (no owned agents: the state's pointers are not looked at before)
    c.state.transmission = None
    rejected(c.phase(lib, 5), E_NULL)
    c.params.has_quarantine = 1
    c.state.transmission, c.state.q_transmission = FAKE, None
    rejected(c.phase(lib, 5), E_NULL)


def test_run_form_alignment_of_values_and_block_index(lib):
    c = Case().run_form().nets((0, Q))
    c.tset.run_pv_blk = FAKE + 8
    rejected(c.phase(lib, 5), E_PLAN)
    c = Case().run_form().nets((0, Q))
    c.state.transmission = FAKE + 4
    rejected(c.phase(lib, 5), E_PLAN)


def test_run_form_of_a_leisure_set(lib):
    c = Case().run_form().nets((0, QL, 0))
    c.tset.e_cls = FAKE
    rejected(c.phase(lib, 5), E_PLAN)


# ---- plan and state ------------------------------------------------------------------------------------------------
def test_csr_gather_cannot_write_agent_sums(lib):
    c = Case(tiled=False).nets((0, Q))
    c.io.agent_sums = FAKE
    rejected(c.phase(lib, 4), E_PLAN)


def test_state_pointers(lib):
    c = Case().nets((0, Q))
    c.state.susceptibility = None
    rejected(c.phase(lib, 6), E_NULL)
    c = Case().nets((0, Q))
    c.state.is_infected = None                           # only a1 / a9 touch the infection state
    rejected(c.phase(lib, 3), E_NULL)
    rejected(c.phase(lib, 0), E_NULL)
    c = Case().nets((0, Q))
    c.params.has_quarantine = 1
    c.state.current_stage = None
    rejected(c.phase(lib, 6), E_NULL)
    c = Case().nets((0, Q))
    c.state.shape = None
    rejected(c.phase(lib, 0), E_NULL)
    rejected(lib.gj_step_phase(C.byref(c.plan), None, C.byref(c.params), None, 6, None), E_NULL)
    rejected(lib.gj_step_phase(C.byref(c.plan), C.byref(c.state), None, None, 6, None), E_NULL)


def test_plan_checks_come_first(lib):
    c = Case().nets((0, RAW), (0, Q))                    # (the network list is wrong too: the plan's code wins)
    c.plan.sets[0].cum_stride = N.GJ_MAX_NETS_PER_SET + 1
    rejected(c.phase(lib, 6), E_PLAN)
    c = Case().nets((0, Q))
    c.tiled.slice_agents = 65
    rejected(c.phase(lib, 6), E_PLAN)
    c = Case().nets((0, Q))
    c.tset.val = None
    rejected(c.phase(lib, 6), E_NULL)
    c = Case().run_form().nets((0, Q))
    c.tset.run_win_n = None                              # run form: all five arrays or none
    rejected(c.phase(lib, 6), E_NULL)
    c = Case().direct().nets((0, Q))
    c.tset.ell_k = 3
    rejected(c.phase(lib, 3), E_PLAN)
    c = Case().nets((0, Q))
    c.plan.n_ext_agents = 32                             # fewer than the owned agents
    rejected(c.phase(lib, 6), E_RANGE)


# ---- symptoms: the three entry points share their argument rules ---------------------------------------------------
def symptoms_params(n_stages=8, progress=FAKE):
    p = N.SymptomsParams()
    p.n_stages, p.progress = n_stages, progress
    return p


def symptoms_calls(lib):
    """name -> f(n, cls, new, cur, nxt, ttn, params, progresses, dwell) with every other argument valid"""
    edges = (C.c_int32 * 4)(0, 20, 60, 100)

    def update(n, cls, new, cur, nxt, ttn, p, pr, dw):
        return lib.gj_symptoms_update(n, cls, new, cur, nxt, ttn, p, pr, dw, None)

    def adjoint(n, cls, new, cur, nxt, ttn, p, pr, dw):
        return lib.gj_adjoint_symptoms(n, cls, new, cur, nxt, ttn, p, pr, dw, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                       None)

    def fused(n, cls, new, cur, nxt, ttn, p, pr, dw):
        return lib.gj_symptoms_step_stats(n, cls, new, cur, nxt, ttn, p, pr, dw, FAKE, 3, edges, 7, FAKE, None)

    return {"update": update, "adjoint": adjoint, "fused": fused}


@pytest.mark.parametrize("entry", ["update", "adjoint", "fused"])
def test_symptoms_argument_errors(lib, entry):
    f = symptoms_calls(lib)[entry]
    p = C.byref(symptoms_params())
    good = [FAKE] * 5
    rejected(f(-1, *good, p, None, None), E_RANGE)
    assert f(0, None, None, None, None, None, None, None, None) == OK          # nothing to do
    for i in range(5):                                                           # each required array
        args = list(good)
        args[i] = None
        rejected(f(4, *args, p, None, None), E_NULL)
    rejected(f(4, *good, None, None, None), E_NULL)                              # params
    for n_stages in (2, N.GJ_MAX_STAGES + 1):
        rejected(f(4, *good, C.byref(symptoms_params(n_stages)), None, None), E_RANGE)
    rejected(f(4, *good, p, FAKE, None), E_NULL)                                 # inject both or neither
    rejected(f(4, *good, p, None, FAKE), E_NULL)
    rejected(f(4, *good, C.byref(symptoms_params(progress=None)), None, None), E_NULL)   # own draws need the table
    # precedence: a NULL array before the stage count, the stage count before the injected pair
    rejected(f(4, None, *good[1:], C.byref(symptoms_params(2)), FAKE, None), E_NULL)
    rejected(f(4, *good, C.byref(symptoms_params(2)), FAKE, None), E_RANGE)


def test_symptoms_adjoint_outputs(lib):
    p = C.byref(symptoms_params())
    # outs: g_current, g_next, g_time (optional), g_current_in, g_next_in, g_time_in (optional), g_new_infected
    for missing in (3, 4, 6):
        outs = [FAKE] * 7
        outs[missing] = None
        rejected(lib.gj_adjoint_symptoms(4, FAKE, FAKE, FAKE, FAKE, FAKE, p, None, None, *outs, None), E_NULL)
    # a missing output before the stage count
    outs = [FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE]
    rejected(lib.gj_adjoint_symptoms(4, FAKE, FAKE, FAKE, FAKE, FAKE, C.byref(symptoms_params(2)), None, None, *outs,
                                     None), E_NULL)


def test_fused_symptoms_statistics_arguments(lib):
    p = C.byref(symptoms_params())
    edges = (C.c_int32 * 4)(0, 20, 60, 100)
    f = lib.gj_symptoms_step_stats
    g = [FAKE] * 5
    rejected(f(4, *g, p, None, None, FAKE, 9, edges, 7, FAKE, None), E_RANGE)   # n_bins past GJ_MAX_AGE_BINS
    rejected(f(4, *g, p, None, None, FAKE, -1, edges, 7, FAKE, None), E_RANGE)
    rejected(f(4, *g, p, None, None, FAKE, 3, edges, 7, None, None), E_NULL)    # out
    rejected(f(4, *g, p, None, None, FAKE, 3, None, 7, FAKE, None), E_NULL)     # edges
    rejected(f(4, *g, p, None, None, None, 3, edges, 7, FAKE, None), E_NULL)    # is_infected
    rejected(f(0, *g, p, None, None, FAKE, 3, edges, 7, None, None), E_NULL)    # out is checked before n == 0
    rejected(f(4, *g, None, None, None, FAKE, 9, edges, 7, FAKE, None), E_RANGE)  # the bins before the NULL params
    s = lib.gj_step_stats
    rejected(s(4, FAKE, FAKE, FAKE, 9, edges, 7, FAKE, None), E_RANGE)
    rejected(s(4, FAKE, FAKE, FAKE, 3, edges, 7, None, None), E_NULL)
    rejected(s(4, FAKE, FAKE, FAKE, 3, None, 7, FAKE, None), E_NULL)
    for i in range(3):
        a = [FAKE] * 3
        a[i] = None
        rejected(s(4, *a, 3, edges, 7, FAKE, None), E_NULL)
    assert s(0, None, None, None, 0, None, 7, FAKE, None) == OK


# ---- the transmission adjoint's two entry points share theirs -------------------------------------------------------
PROFILE_STATE = ("max_infectiousness", "shape", "rate", "shift", "infection_time", "is_infected")


def profile_state(missing=None):
    st = N.AgentState()
    for k in PROFILE_STATE:
        setattr(st, k, None if k == missing else FAKE)
    return st


@pytest.mark.parametrize("params", [False, True])
def test_transmission_adjoint_argument_errors(lib, params):
    extra = [FAKE] * 4 if params else []
    fn = lib.gj_adjoint_transmission_params if params else lib.gj_adjoint_transmission

    def f(n, st, trans_bar, grad_inf, grad_time):
        return fn(n, C.byref(st) if st is not None else None, 0.0, trans_bar, None, grad_inf, grad_time, *extra, None)

    st = profile_state()
    rejected(f(-1, st, FAKE, FAKE, FAKE), E_RANGE)
    assert f(0, None, None, None, None) == OK
    rejected(f(4, None, FAKE, FAKE, FAKE), E_NULL)
    rejected(f(4, st, None, FAKE, FAKE), E_NULL)
    rejected(f(4, st, FAKE, None, FAKE), E_NULL)
    rejected(f(4, st, FAKE, FAKE, None), E_NULL)
    for k in PROFILE_STATE:
        rejected(f(4, profile_state(missing=k), FAKE, FAKE, FAKE), E_NULL)
    rejected(f(-1, None, None, None, None), E_RANGE)                    # the count before the pointers
