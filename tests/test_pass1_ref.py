"""The restatement of pass 1 (tests/gj_pass1_ref.py) - what tests/test_gpu_pass1_kernels.py holds the device to bit for
bit - checked on the CPU so that a wrong restatement cannot hide: against float64 sums from the edge lists within the
project's own derived bound (gj_testlib.sparse_pass_bounds, E1), against the per-venue sums recorded from the reference
(tests/golden), under permutations of the edge lists, and each of its rules on hand-made venues.

The last part shows that the inputs of the GPU file can tell a wrong kernel from a right one: every misstatement of one
rule differs from the restatement on a world and an input of that file.  No broken kernel is built or run."""
import math

import numpy as np
import pytest
import torch

import gj_pass1_ref as R1
import gj_testlib as L
import test_gpu_pass1_kernels as G
from grad_june_amd import _native as N
from grad_june_amd.plan import _host, p_contact

F32 = np.float32
WORLDS = ["small", "quads", "run", "uniform", "halo-small", "halo-run", "primary", "presum", "batch2", "tables", "wrap"]
# a case of the GPU file on each of its worlds (the plan gives p_contact and max_venue_edges; the restatement does not
# know the geometry)
CASE_OF = {"small": "ws-narrow", "quads": "quads-ws-4160", "run": "run", "uniform": "uniform-ws", "halo-small": "halo-ws",
           "halo-run": "halo-run", "primary": "primary-run", "presum": "presum-3", "batch2": "presum-batch2",
           "tables": "presum-34", "wrap": "presum-wrap"}


def test_every_world_of_the_gpu_file_is_covered():
    assert {G.CASES[c][0] for c in G.EVERY} == set(WORLDS) == set(CASE_OF)
    assert all(G.CASES[c][0] == k for k, c in CASE_OF.items())


# ---- against float64 within E1 -----------------------------------------------------------------------------------------
def as_testlib_world(w):
    """The world as gj_testlib takes it: torch tensors, halo agents counted as agents."""
    sets = {k: {kk: torch.from_numpy(np.asarray(vv)) for kk, vv in v.items()} for k, v in w["edge_sets"].items()}
    return {"n_agents": w["n_ext"], "age": torch.from_numpy(np.asarray(w["age"])), "sex": torch.from_numpy(np.asarray(w["sex"])),
            "edge_sets": sets}


@pytest.mark.parametrize("wkey", WORLDS)
def test_restatement_within_the_derived_bound_of_float64(wkey):
    case = CASE_OF[wkey]
    w = G.world_of(wkey)
    world = as_testlib_world(w)
    tables = {n: torch.from_numpy(t) for n, t in w["tables"].items()}
    for transpose in (0, 1):
        x = G.transmissions(w, 300 + transpose, signed=bool(transpose))
        for has_q in (False, True):
            day_type = transpose ^ int(has_q)
            want = G.restated(case, x, day_type=day_type, transpose=transpose, has_q=has_q)
            qmask = (w["stage_ext"] < G.Q_THR).astype(np.float64) if has_q else None
            ref = L.sparse_passes_with_bounds(world, w["active"], w["betas"], tables, day_type, qmask, x,
                                              transpose=bool(transpose))
            column = {}
            for n in w["active"]:
                es = L.edge_set_name(n)
                k = column.get(es, 0)
                column[es] = k + 1
                got = R1.f32_of(want[es][0])[:, k].astype(np.float64)
                bad = ~(np.abs(got - ref["cum"][n]) <= ref["cum_bound"][n])
                assert not bad.any(), (wkey, n, transpose, has_q, int(np.argmax(bad)), got[bad][:3], ref["cum"][n][bad][:3],
                                       ref["cum_bound"][n][bad][:3])
                if len(w["edge_sets"][es]["agent"]):
                    assert np.abs(ref["cum"][n]).max() > 0
                assert not want[es][1].any()


# ---- against the per-venue sums recorded from the reference --------------------------------------------------------------
GOLDEN_RTOL = 2e-5          # tests/test_gpu_golden_parity.py, cum_n[v]


def golden_records():
    out = []
    for name in ("c100.npz", "synth10k.npz", "june769.npz"):
        npz = L.load_npz(name)
        prefixes = sorted({k.split("/")[0] + "/" for k in npz if "/cum/" in k})
        out += [(name, p) for p in prefixes]
    return out


@pytest.mark.parametrize("name,prefix", golden_records())
def test_restatement_against_the_recorded_sums(name, prefix):
    npz = L.load_npz(name)
    world, tables = L.world_from(npz), L.tables_from(npz)
    rec = L.step_record(npz, prefix)
    sc = L.step_scalars(rec)
    specs = L.network_specs(world, tables or None)
    sets = {k: {kk: vv.numpy() for kk, vv in v.items()} for k, v in world["edge_sets"].items()}
    thr = sc["quarantine_thresholds"]
    want = R1.restate(sets, {k: p_contact(v["people"]) for k, v in sets.items()}, specs, sc["active"], sc["betas"],
                      rec["transmission"].astype(np.float32), age=world["age"].numpy(), sex=world["sex"].numpy(),
                      stage=rec["pre/current_stage"].astype(np.float32), q_thr=L.q_threshold(thr), has_quarantine=thr is not None,
                      day_type=sc["day_type"], transpose=0)
    column = {}
    by_name = {s.name: s for s in specs}
    for n in sc["active"]:
        es = by_name[n].edge_set
        k = column.get(es, 0)
        column[es] = k + 1
        ref = rec["cum/" + n]
        got = R1.f32_of(want[es][0])[:, k]
        atol = 1e-12 + 1e-6 * float(np.abs(ref).max() if ref.size else 0)      # (as test_gpu_golden_parity.run_case)
        assert np.allclose(got, ref, rtol=GOLDEN_RTOL, atol=atol), (name, prefix, n, np.abs(got - ref).max())


# ---- permutations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkey", ["small", "uniform", "halo-run", "presum"])
def test_permuting_the_edge_list_changes_no_bit(wkey):
    case = CASE_OF[wkey]
    w = G.world_of(wkey)
    host = G.case_host(case)
    rng = np.random.default_rng(5)
    x = G.transmissions(w, 301, signed=True)
    kw = dict(rules=G.rules_of(case), age=w["age"], sex=w["sex"], stage=w["stage_ext"], q_thr=G.Q_THR, has_quarantine=True,
              day_type=1, transpose=1)
    pcs = {s.name: s.v_pcontact for s in host.sets}
    want = R1.restate(w["edge_sets"], pcs, w["specs"], w["active"], w["betas"], x, **kw)
    shuffled = {}
    for name, es in w["edge_sets"].items():
        perm = rng.permutation(len(es["agent"]))
        shuffled[name] = dict(es, agent=es["agent"][perm], venue=es["venue"][perm])
    again = R1.restate(shuffled, pcs, w["specs"], w["active"], w["betas"], x, **kw)
    for name in want:
        assert np.array_equal(want[name][0], again[name][0]) and np.array_equal(want[name][1], again[name][1])


# ---- hand-made venues --------------------------------------------------------------------------------------------------------
def one_venue(terms, rule="default", edges=None, pc=1.0, beta=1.0, **kw):
    """(s of the only venue as float32, flagged) with beta = p_contact = 1: cum is s itself."""
    terms = np.asarray(terms, dtype=np.float32)
    n = len(terms)
    cum, flagged = R1.restate_set(np.arange(n), np.zeros(n, dtype=np.int64), np.array([pc], dtype=np.float32),
                                  [(beta, None, False, True)], terms, rule=rule, max_venue_edges=edges, **kw)
    return R1.f32_of(cum)[0, 0], bool(flagged[0, 0])


def test_rint_half_to_even():
    for numerator, fx in ((1, 0), (3, 2), (5, 2), (2, 1)):
        term = F32(numerator * 2.0 ** -37)
        assert R1.to_fx(np.array([term]))[0] == fx
        assert one_venue([term])[0] == F32(fx * 2.0 ** -36)
    assert R1.to_fx(np.array([F32(-3 * 2.0 ** -37)]))[0] == -2 and R1.to_fx(np.array([F32(-2.0 ** -37)]))[0] == 0


def test_the_double_rounding_venue():
    terms = [16384.0] * 32 + [2.0 ** -5, 2.0 ** -36]
    assert one_venue(terms) == (F32(524288.0), False)
    assert one_venue(terms, variant=("single_rounding",)) == (F32(524288.0625), False)
    exact = 32 * 16384 * 2 ** 36 + 2 ** 31 + 1
    assert int(R1.to_fx(np.array(terms, dtype=np.float32)).sum()) == exact
    assert R1.from_fx(np.array([exact]))[0] == F32(524288.0) and R1.from_fx_once(np.array([exact]))[0] == F32(524288.0625)
    # rounding once is what float64 arithmetic of arbitrary width would give: checked against the integer itself
    for v in (exact, -exact, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 60 + 2 ** 36, 12345, 0):
        assert float(R1.from_fx_once(np.array([v]))[0]) == float(np.float32(np.longdouble(v) / np.longdouble(2.0 ** 36)))


def test_the_window():
    window = F32(16384.0)
    above = np.nextafter(window, F32(np.inf))
    assert R1.term_limit_bits(0) == R1.term_limit_bits(4096) == int(window.view(np.uint32)) == 0x46800000
    assert one_venue([window, 1.0]) == (F32(16385.0), False)                    # exactly at the window: inside
    assert one_venue([-window, 1.0]) == (F32(-16383.0), False)
    assert one_venue([above, 1.0]) == (F32(1.0e30), True)                       # the next float32: outside
    assert one_venue([-above, 1.0]) == (F32(-1.0e30), True)
    # 2^13 for a largest venue of 4 097 to 8 192 edges, 2^12 to 16 384, 2^11 to 32 768
    half = int(F32(8192.0).view(np.uint32))
    assert [R1.term_limit_bits(e) for e in (4097, 8192)] == [half, half]
    assert R1.term_limit_bits(8193) == R1.term_limit_bits(16384) == int(F32(4096.0).view(np.uint32))
    assert R1.term_limit_bits(20000) == int(F32(2048.0).view(np.uint32))
    assert one_venue([8192.0, 1.0], edges=4097) == (F32(8193.0), False)
    assert one_venue([np.nextafter(F32(8192.0), F32(np.inf)), 1.0], edges=4097) == (F32(1.0e30), True)
    assert one_venue([np.nextafter(F32(8192.0), F32(np.inf)), 1.0], edges=4096)[1] is False


@pytest.mark.parametrize("value,default,sign", [(np.nan, np.nan, 0), (np.inf, 1e30, 1), (-np.inf, -1e30, -1), (3e4, 1e30, 1),
                                                (-3e4, -1e30, -1)])
def test_both_flag_rules(value, default, sign):
    for rule, expect in (("default", F32(default)), ("presum", F32(np.nan))):
        s, flagged = one_venue([1.0, value, 2.0], rule=rule)
        assert flagged and (np.isnan(s) if np.isnan(expect) else s == expect), (rule, s)
        # p_contact of 0: the saturated value gives 0, a NaN stays
        z, _ = one_venue([1.0, value, 2.0], rule=rule, pc=0.0)
        assert np.isnan(z) if np.isnan(expect) else (z == 0.0 and math.copysign(1.0, z) == sign)
    # both signs in one venue: NaN under either rule; a finite term is summed under neither
    assert np.isnan(one_venue([3e4, -3e4])[0]) and np.isnan(one_venue([3e4, -3e4], rule="presum")[0])
    assert one_venue([1.0, 2.0], rule="presum") == (F32(3.0), False)


def test_sources_and_weights():
    """q * x for the masked kinds (a quarantined agent's NaN stays a NaN, its finite value becomes a zero), x for the
    household; the care-visit mask on the transmitting side only when transposed."""
    x = np.array([1.0, 2.0, np.nan, 4.0], dtype=np.float32)
    stage = np.array([1.0, 5.0, 5.0, 4.0], dtype=np.float32)
    masked = R1.source(x, stage, 4.0, True, raw=False)
    assert masked[0] == 1.0 and masked[1] == 0.0 and np.isnan(masked[2]) and masked[3] == 0.0
    assert np.array_equal(R1.bits(R1.source(x, stage, 4.0, True, raw=True)), R1.bits(x))          # every element, the NaN too
    assert np.array_equal(R1.bits(R1.source(x, stage, 4.0, False, raw=False)), R1.bits(x))         # no quarantine: x itself
    table = np.full((2, 2, 100), 0.5, dtype=np.float32)
    age, sex = np.array([80, 30]), np.array([0, 1])
    nets = [(1.0, table, True, False)]
    args = (np.array([0, 1]), np.array([0, 0]), np.array([1.0], dtype=np.float32), nets, np.array([2.0, 4.0], dtype=np.float32))
    forward = R1.f32_of(R1.restate_set(*args, age=age, sex=sex, transpose=0)[0])[0, 0]
    transposed = R1.f32_of(R1.restate_set(*args, age=age, sex=sex, transpose=1)[0])[0, 0]
    assert forward == 3.0 and transposed == 1.0


# ---- every misstatement shows on an input of the GPU file --------------------------------------------------------------------
def restate_case(case, x, *, transpose=0, has_q=False, variant=(), drop=None):
    w = G.world_of(G.CASES[case][0])
    host = G.case_host(case)
    return R1.restate(w["edge_sets"], {s.name: s.v_pcontact for s in host.sets}, w["specs"], w["active"], w["betas"], x,
                      rules=G.rules_of(case), drop=drop, age=w["age"], sex=w["sex"], stage=w["stage_ext"], q_thr=G.Q_THR,
                      has_quarantine=has_q, day_type=0, transpose=transpose, variant=variant)


def differs(a, b, name):
    return not np.array_equal(a[name][0], b[name][0])


def window_of(case, name):
    host = G.case_host(case)
    return R1.f32_of(np.array([R1.term_limit_bits(host.sets[host.set_index[name]].max_venue_edges)], dtype=np.uint32))[0]


def test_misstated_roundings_show():
    for case, name in G.ROUNDINGS:                 # the double-rounding venues of the GPU file
        x, venue = G.double_rounding_input(case, name)
        true, wrong = restate_case(case, x), restate_case(case, x, variant=("single_rounding",))
        assert true[name][0][venue, 0] != wrong[name][0][venue, 0], (case, name)
    for case in ("ws-narrow", "uniform-ws", "run", "presum-3", "presum-batch2"):       # floor: the small terms, in every set
        w = G.world_of(G.CASES[case][0])
        x = G.small_terms(w, 320, signed=False)
        true, wrong = restate_case(case, x), restate_case(case, x, variant=("floor",))
        assert all(differs(true, wrong, name) for name in true if len(w["edge_sets"][name]["agent"])), case
    # (the values of `transmissions`, 2^-10 and more, are whole numbers of 2^-36, and a venue's sum of them is too large
    # for an error of a few 2^-36 to survive its rounding to float32: they cannot tell floor from rint in any set)
    w = G.world_of("small")
    x = G.transmissions(w, 300, signed=False)
    assert restate_case("ws-narrow", x)["school"][0].tolist() == restate_case("ws-narrow", x, variant=("floor",))["school"][0].tolist()


def test_misstated_windows_show():
    # the window not shrunk for the big venue: the next float32 above 2^13 at the agents of the wave-uniform venue, and
    # the terms of 10 000 of the wrap world
    case, name, how = "uniform-ws", "school", "uniform"
    w = G.world_of("uniform")
    chosen = G.special_agents(case, name, how)
    above = np.nextafter(window_of(case, name), F32(np.inf))
    assert window_of(case, name) == 8192.0
    x = G.special_input(w, chosen, above, 0)
    true, wrong = restate_case(case, x), restate_case(case, x, variant=("window_not_shrunk",))
    assert differs(true, wrong, name) and true[name][1].any() and not wrong[name][1].any()
    x = np.full(20_000, 10000.0, dtype=np.float32)
    true, wrong = restate_case("presum-wrap", x), restate_case("presum-wrap", x, variant=("window_not_shrunk",))
    assert np.isnan(R1.f32_of(true["school"][0])[0, 0]) and np.isfinite(R1.f32_of(wrong["school"][0])[0, 0])
    # < instead of <= at the window: the window itself at the chosen agents of every special case of a plain set
    for case, name, how in G.SPECIALS:
        if G.tiled_of(case, name).e_cls is not None:
            continue
        w = G.world_of(G.CASES[case][0])
        x = G.special_input(w, G.special_agents(case, name, how), window_of(case, name), 0)
        true, wrong = restate_case(case, x), restate_case(case, x, variant=("strict_window",))
        assert differs(true, wrong, name) and not true[name][1].any() and wrong[name][1].any(), (case, name)


def test_dropped_edges_show():
    for case in ("halo-ws", "halo-run"):           # halo edges dropped
        w = G.world_of(G.CASES[case][0])
        x = G.transmissions(w, 300, signed=False)
        drop = {name: es["agent"] >= w["n_agents"] for name, es in w["edge_sets"].items()}
        true, wrong = restate_case(case, x), restate_case(case, x, drop=drop)
        for name in ("household", "company", "school", "leisure"):
            assert drop[name].any() and differs(true, wrong, name), (case, name)
    for case in ("primary-run", "run", "uniform-run"):       # the first or the last agent of a run-form block dropped
        w = G.world_of(G.CASES[case][0])
        es = w["edge_sets"]["household"]
        r0 = _host(G.tiled_of(case, "household").runs.blk_r0).astype(np.int64)
        primary = ~G.tiled_of(case, "household").runs.keep
        x = G.transmissions(w, 300, signed=False)
        true = restate_case(case, x)
        shown = {"first": 0, "last": 0}
        for which, agents in (("first", r0[:-1]), ("last", r0[1:] - 1)):
            for a in agents[np.diff(r0) > 0]:
                wrong = restate_case(case, x, drop={"household": primary & (es["agent"] == a)})
                assert (primary & (es["agent"] == a)).sum() == 1
                shown[which] += differs(true, wrong, "household")
                assert x[a] != 0 or not differs(true, wrong, "household")
        assert shown["first"] >= 1 and shown["last"] >= 1, (case, shown)


def test_care_visit_mask_in_the_forward_direction_shows():
    for case in ("ws-narrow", "presum-3", "quads-ws-4160"):
        w = G.world_of(G.CASES[case][0])
        x = G.transmissions(w, 300, signed=False)
        true, wrong = restate_case(case, x), restate_case(case, x, variant=("mask_forward",))
        k = [s.mask_kind for s in w["specs"] if s.edge_set == "leisure"].index(N.MASK_QL_AGE75)
        assert not np.array_equal(true["leisure"][0][:, k], wrong["leisure"][0][:, k]), case
        # transposed, the mask belongs there: the misstatement is none
        xt = G.transmissions(w, 301, signed=True)
        assert not differs(restate_case(case, xt, transpose=1), restate_case(case, xt, transpose=1, variant=("mask_forward",)),
                           "leisure")
