"""CPU: the restatement of the who-infects-whom matrix (tests/gj_matrix_ref.py) against the infector series' restatement,
the binned labellings of ``groups.encode_groups`` and the host logic of the ``infection_matrices_to_save`` key.  The GPU
tests hold the kernels to this restatement."""
import functools

import numpy as np
import pytest
import torch

import gj_infector_ref as I
import gj_matrix_ref as M
from test_infector_ref import _runner
from test_location_ref import _Model

BINS = {"age_band": {"attribute": "age", "bins": [0, 18, 65, 100]}}


@functools.lru_cache(maxsize=None)
def world_case(G=5):
    """make_world(1000) of the GPU tests with generic sums, a step's new infections, labels, and both restatements."""
    from test_gpu_infector_stats import BETAS
    from test_gpu_location_stats import ACTIVE, THRESHOLD, draw_cum, edges_of, generic_values, make_world

    A = 1000
    world, tables = make_world(A)
    rng = np.random.default_rng(77)
    cum = draw_cum(world, rng, generic_values)
    s0, stage = rng.random(A).astype(np.float32), rng.integers(1, 8, A).astype(np.float32)
    s0[rng.random(A) < 0.1] = 0.0
    nu = (rng.random(A) < 0.4).astype(np.float32)
    group = rng.integers(0, G, A)
    q = (stage < np.float32(THRESHOLD)).astype(np.float64)
    nets = I.step_nets(world, tables, ACTIVE, BETAS, 1, q)
    edges = {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(world).items()}
    return dict(A=A, G=G, nets=nets, edges=edges, cum=cum, s0=s0, nu=nu, group=group,
                national=I.scatter(nets, edges, cum, s0, nu, A),
                by_group=M.scatter_by_group(nets, edges, cum, s0, nu, A, group, G))


def test_the_units_by_group_sum_to_the_infector_series_units_in_every_cell():
    c = world_case()
    units, lost, err, _ = c["national"]
    UG, lost_by, err_by = c["by_group"]
    assert err == err_by == 0 and sum(int(u.sum()) for u in units.values()) > 100 * I.U
    for s, u in units.items():
        assert UG[s].shape == u.shape + (c["G"],) and (UG[s] >= 0).all()
        assert np.array_equal(UG[s].sum(-1), u), s
    assert int(lost_by.sum()) == lost > 0


def test_every_infection_of_a_group_is_in_its_plane_or_in_its_unattributed_count():
    c = world_case()
    UG, lost_by, _ = c["by_group"]
    new = np.bincount(c["group"][c["nu"] == 1], minlength=c["G"])
    for g in range(c["G"]):
        scattered = sum(int(u[:, :, g].sum()) for u in UG.values())
        assert scattered + I.U * int(lost_by[g]) == I.U * int(new[g]), g
    assert new.min() > 0 and (lost_by > 0).any()


def test_bad_labels_and_values_in_the_restatement():
    c = world_case()
    group, nu = c["group"].copy(), c["nu"].copy()
    at = np.nonzero(nu == 1)[0][:3]
    group[at[0]], group[at[1]], nu[at[2]] = c["G"], -1, 2.0
    UG, lost, err = M.scatter_by_group(c["nets"], c["edges"], c["cum"], c["s0"], nu, c["A"], group, c["G"])
    assert err == M.ERR_LABEL | M.ERR_VALUE
    keep = c["nu"].copy()
    keep[at] = 0.0
    want, want_lost, _ = M.scatter_by_group(c["nets"], c["edges"], c["cum"], c["s0"], keep, c["A"], c["group"], c["G"])
    assert all(np.array_equal(UG[s], want[s]) for s in want) and np.array_equal(lost, want_lost)


def test_the_matrix_sums_the_infector_series_terms_by_pairs_of_groups():
    """A venue with one new infection in group 1 and transmitters in groups 0 and 2: their shares land in column 1."""
    A, G = 3, 3
    edges = {"x": (np.array([0, 1, 2]), np.array([0, 0, 0]))}
    one = np.ones(A)
    nets = [I.Net("x", 0, 2.0, one, one)]
    cum = {"x": np.array([[0.5]], np.float32)}
    pc = {"x": np.array([0.25], np.float32)}
    group = np.array([0, 1, 2])
    UG, lost, err = M.scatter_by_group(nets, edges, cum, one, np.array([0, 1, 0], np.float32), A, group, G)
    assert err == 0 and not lost.any() and UG["x"].tolist() == [[[0, I.U, 0]]]
    tr = np.array([0.75, 0.0, 0.25], np.float32)          # cum = beta * pc * (0.75 + 0.25) = 0.5
    got = M.matrix(nets, edges, cum, pc, UG, tr, A, group, G)
    assert got == [[0, 3 * I.U // 4, 0], [0, 0, 0], [0, I.U // 4, 0]]
    assert M.matrix(nets, edges, cum, pc, {"x": UG["x"].sum(-1, keepdims=True)}, tr, A, None, 1) == [[I.U]]


# ---- binned labellings ------------------------------------------------------------------------------------------------------
def _agents(n=200, seed=4):
    rng = np.random.default_rng(seed)
    return {"id": np.arange(n), "age": torch.from_numpy(rng.integers(0, 100, n)), "area": rng.integers(0, 3, n)}


def test_a_binned_labelling_is_the_digitized_attribute():
    from grad_june_amd.groups import encode_groups

    agent = _agents()
    age = agent["age"].numpy()
    age[:4] = [0, 17, 18, 99]                                                       # the edges: lo <= value < hi
    for spec in (BINS, [BINS], ["area", BINS]):
        labels, keys = encode_groups(agent, spec)
        assert keys["age_band"] == ["0-18", "18-65", "65-100"]
        assert labels["age_band"].dtype == torch.int32
        assert np.array_equal(labels["age_band"].numpy(), np.digitize(age, [0, 18, 65, 100]) - 1)
        assert labels["age_band"][:4].tolist() == [0, 0, 1, 2]
    assert set(encode_groups(agent, ["area", BINS])[0]) == {"area", "age_band"}
    # a band without agents keeps its column; float edges name themselves
    labels, keys = encode_groups(agent, {"half": {"attribute": "age", "bins": [0, 99.5, 200]}})
    assert keys["half"] == ["0-99.5", "99.5-200"] and not labels["half"].any()


def test_a_binned_labelling_refuses_bad_bins_and_values_outside_them():
    from grad_june_amd.groups import encode_groups

    agent = _agents()
    for bins in ([0, 18, 18, 100], [0, 65, 18, 100], [100, 0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            encode_groups(agent, {"age_band": {"attribute": "age", "bins": bins}})
    agent["age"][7] = 99
    with pytest.raises(ValueError, match="outside every bin"):
        encode_groups(agent, {"age_band": {"attribute": "age", "bins": [0, 18, 65, 99]}})      # hi is exclusive
    agent["age"][8] = 0
    with pytest.raises(ValueError, match="outside every bin"):
        encode_groups(agent, {"age_band": {"attribute": "age", "bins": [1, 18, 65, 100]}})
    with pytest.raises(KeyError, match="no attribute"):
        encode_groups(agent, {"age_band": {"attribute": "height", "bins": [0, 1]}})
    with pytest.raises(ValueError, match="attribute: <name>, bins"):
        encode_groups(agent, {"age_band": {"attribute": "age", "edges": [0, 100]}})
    with pytest.raises(ValueError, match="at least two"):
        encode_groups(agent, {"age_band": {"attribute": "age", "bins": [0]}})


def test_the_runner_takes_a_binned_labelling_like_any_other():
    r = _runner(groups=[BINS, "area"])                                              # ages 5, 20, 30, 70, 80, 40
    assert r.group_keys["age_band"].tolist() == ["0-18", "18-65", "65-100"]
    assert r.data["agent"].group_labels["age_band"].tolist() == [0, 1, 1, 2, 2, 1]
    assert set(r.group_keys) == {"age_band", "area"}


# ---- the key ---------------------------------------------------------------------------------------------------------------
def test_yaml_key():
    from grad_june_amd.groups import infection_matrices_to_save

    assert infection_matrices_to_save(None) == [] and infection_matrices_to_save([]) == []
    assert infection_matrices_to_save(["age_band", "area"]) == ["age_band", "area"]
    assert infection_matrices_to_save("area") == ["area"]
    for bad in (True, 3, [1], {"area": 1}):
        with pytest.raises(ValueError, match="list of labelling names"):
            infection_matrices_to_save(bad)
    with pytest.raises(ValueError, match="twice"):
        infection_matrices_to_save(["area", "area"])


def test_the_runner_validates_the_key(monkeypatch):
    from grad_june_amd import _native as N
    from grad_june_amd import runner as RN

    plain = _runner(infectors=True, groups=["area"])
    assert plain.matrices_saved == []
    on = _runner(infectors=True, groups=["area", BINS], matrices=["age_band"])
    assert on.matrices_saved == ["age_band"]
    with pytest.raises(ValueError, match="no labelling of groups_to_save"):
        _runner(infectors=True, groups=["area"], matrices=["age_band"])
    with pytest.raises(ValueError, match="no labelling of groups_to_save"):
        _runner(infectors=True, matrices=["area"])
    with pytest.raises(ValueError, match="needs infectors_to_save"):
        _runner(groups=["area"], matrices=["area"])
    with pytest.raises(ValueError, match="needs infectors_to_save"):
        _runner(infectors=False, groups=["area"], matrices=["area"])
    assert N.GJ_MATRIX_MAX_GROUPS == 64 and N.GJ_MATRIX_MAX_GROUPS ** 2 <= N.GJ_LOC_LDS_BINS
    many = {"many": np.array([0, 1, 2, 3, 4, N.GJ_MATRIX_MAX_GROUPS])}                # 65 groups
    with pytest.raises(ValueError, match="at most 64"):
        _runner(infectors=True, groups=many, matrices=["many"])
    assert _runner(infectors=True, groups={"many": np.array([0, 1, 2, 3, 4, 63])}, matrices=["many"]).matrices_saved == ["many"]
    # from the YAML
    data = on.data
    monkeypatch.setattr(RN.Runner, "get_data", staticmethod(lambda params: data))
    monkeypatch.setattr(RN.GradJune, "from_parameters", classmethod(lambda cls, params: _Model()))
    monkeypatch.setattr(RN.Timer, "from_parameters", classmethod(lambda cls, params: None))
    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused", "infectors_to_save": True}
    assert RN.Runner.from_parameters(dict(params)).matrices_saved == []
    assert RN.Runner.from_parameters(dict(params, infection_matrices_to_save=["age_band"])).matrices_saved == ["age_band"]
    with pytest.raises(ValueError, match="needs infectors_to_save"):
        RN.Runner.from_parameters(dict(params, infectors_to_save=False, infection_matrices_to_save=["age_band"]))


def test_the_statistics_object_validates_its_matrices():
    from grad_june_amd import _native as N
    from grad_june_amd.groups import InfectorStats

    labels = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="no such labelling"):
        InfectorStats(6, {"area": (labels, 3)}, device="cpu", matrices=["age_band"])
    with pytest.raises(ValueError, match="at most 64"):
        InfectorStats(6, {"area": (labels, N.GJ_MATRIX_MAX_GROUPS + 1)}, device="cpu", matrices=["area"])
    with pytest.raises(ValueError, match="'memset' or 'walk'"):
        InfectorStats(6, {"area": (labels, 3)}, device="cpu", matrices=["area"], matrix_clear="never")
    st = InfectorStats(6, {"area": (labels, 3), "sex": (labels, 2)}, device="cpu", n_rows=4, matrices={"area": True})
    assert st.matrix["area"].shape == (4, 3, 3) and st.matrix["area"].dtype == torch.int64
    assert st.unattributed_by["area"].shape == (4, 3) and set(st.matrix) == {"area"}
    assert st.matrix_values("area", 2).shape == (2, 3, 3) and st.matrix_values("area").dtype == torch.float32
    assert InfectorStats(6, {"area": (labels, 3)}, device="cpu").matrix == {}      # no key: nothing allocated


def test_a_partitioned_run_refuses_the_key():
    from grad_june_amd.distributed_api import DistributedRunner

    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused",
              "infection_matrices_to_save": ["age_band"]}
    with pytest.raises(NotImplementedError, match="partitioned"):
        DistributedRunner.from_parameters(params)                    # before a world is loaded or a device is touched
    with pytest.raises(NotImplementedError, match="partitioned"):
        _runner(DistributedRunner, groups=["area"], matrices=["area"])
    assert _runner(DistributedRunner, groups=["area"]).matrices_saved == []


def test_argument_errors_do_not_need_a_gpu():
    """A NULL plan is refused before anything touches the device, by all three entry points."""
    from grad_june_amd import _native as N

    lib = N.load()
    assert lib.gj_infection_matrix_scatter(None, None, None, None, None, None, None, 1, None, None, None, None) == -1
    assert lib.gj_infection_matrix_gather(None, None, None, None, None, None, None, None, 1, None, None, None) == -1
    assert lib.gj_infection_matrix_clear(None, None, None, None, 1, None) == -1
    assert M.U == N.GJ_LOC_UNIT
