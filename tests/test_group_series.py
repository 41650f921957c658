"""CPU: result series by agent group - the label encoding, how the labels follow a renumbering of the agents, the
Runner's construction with and without groups, and the C declarations of gj_group_stats / gj_adjoint_group_stats
against their ctypes bindings.  No device is touched (the kernels are covered by tests/test_gpu_group_series.py)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from grad_june_amd import _native as N
from grad_june_amd.groups import attach_groups, encode_groups
from grad_june_amd.runner import Runner, world_from_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gradjune_hip.h")
WORLD = os.path.join(ROOT, "gradabm-june_amd", "grad_june_amd", "worlds", "world769.npz")


def world():
    return world_from_npz(WORLD)


def test_string_attributes_are_encoded_in_sorted_order():
    data = world()
    ag = data["agent"]
    labels, keys = encode_groups(ag, ["area", "ethnicity", "sex"])
    assert list(labels) == ["area", "ethnicity", "sex"]
    for name in ("area", "ethnicity"):
        raw = np.asarray(ag[name])
        assert keys[name] == sorted(set(raw.tolist()))                       # the column order of Runner.ethnicities
        assert labels[name].dtype == torch.int32 and labels[name].shape == (769,)
        assert np.array_equal(np.asarray(keys[name])[labels[name].numpy()], raw)
    assert len(keys["area"]) == 3 and len(keys["ethnicity"]) == 17
    assert keys["sex"] == [0, 1] and np.array_equal(labels["sex"].numpy(), ag.sex.numpy())


def test_integer_labels_are_taken_as_they_are_and_count_empty_groups():
    data = world()
    lab = np.zeros(769, dtype=np.int64)
    lab[5], lab[9] = 6, 2                                                    # groups 1, 3, 4, 5 have nobody
    labels, keys = encode_groups(data["agent"], {"ward": lab})
    assert keys["ward"] == list(range(7))
    assert np.array_equal(labels["ward"].numpy(), lab)
    labels, keys = encode_groups(data["agent"], ["area", {"ward": torch.from_numpy(lab)}])
    assert list(labels) == ["area", "ward"] and len(keys["ward"]) == 7


def test_sparse_integer_attributes_get_dense_columns():
    data = world()
    data["agent"].district = torch.from_numpy(np.where(np.arange(769) % 2 == 0, 40, 7))
    labels, keys = encode_groups(data["agent"], ["district"])
    assert keys["district"] == [7, 40]
    assert np.array_equal(labels["district"].numpy(), (np.arange(769) % 2 == 0).astype(np.int32))


def test_bad_specifications_are_refused():
    data = world()
    ag = data["agent"]
    with pytest.raises(KeyError, match="super_area"):
        encode_groups(ag, ["area", "super_area"])
    with pytest.raises(ValueError, match="age"):                             # cases_by_age_XX exists already
        encode_groups(ag, ["age"])
    with pytest.raises(ValueError, match="age_18"):
        encode_groups(ag, {"age_18": np.zeros(769, dtype=np.int64)})
    with pytest.raises(ValueError):
        encode_groups(ag, {"ward": np.zeros(768, dtype=np.int64)})           # one label short
    with pytest.raises(ValueError):
        encode_groups(ag, {"ward": np.full(769, -1)})
    with pytest.raises(TypeError):
        encode_groups(ag, {"ward": np.zeros(769, dtype=np.float32)})
    with pytest.raises(ValueError):
        encode_groups(ag, ["area", "area"])
    with pytest.raises(ValueError):
        encode_groups(ag, ["not a name"])


def test_g_is_that_of_the_whole_world_and_a_cut_keeps_it():
    """The multi-GPU partition cuts the agents AFTER the encoding: a slice that holds one area still has three columns."""
    data = world()
    attach_groups(data["agent"], ["area"])
    ag = data["agent"]
    order = np.argsort(ag.group_labels["area"].numpy(), kind="stable")
    first = ag.group_labels["area"][torch.from_numpy(order)][:50]
    assert len(set(first.tolist())) == 1 and len(ag.group_keys["area"]) == 3


def test_labels_follow_locality_order():
    from grad_june_amd.graph import locality_order

    data = world()
    ward = np.arange(769) % 5
    attach_groups(data["agent"], ["area", "ethnicity", {"ward": ward}])
    before = {k: v.clone() for k, v in data["agent"].group_labels.items()}
    ids = data["agent"].id.clone()
    data, original = locality_order(data, by="household")
    assert not torch.equal(original, torch.arange(769)), "the order did not change: the test shows nothing"
    ag = data["agent"]
    assert torch.equal(ag.id, ids[original])
    for name in ("area", "ethnicity", "ward"):
        assert torch.equal(ag.group_labels[name], before[name][original]), name
        # ... and still name the agent's own attribute
    assert np.array_equal(np.asarray(ag.group_keys["area"])[ag.group_labels["area"].numpy()], np.asarray(ag.area))
    assert np.array_equal(ag.group_labels["ward"].numpy(), ward[original.numpy()])
    assert ag.group_keys["ward"] == [0, 1, 2, 3, 4]


def _runner(groups=None, attach=None):
    data = world()
    ag = data["agent"]
    n = 769
    for k in ("susceptibility", "is_infected", "infection_time", "transmission"):
        ag[k] = torch.zeros(n)
    ag.symptoms = {k: torch.ones(n) for k in ("current_stage", "next_stage", "time_to_next_stage")}
    if attach:
        attach_groups(ag, attach)
    model = types.SimpleNamespace(device=torch.device("cpu"))
    kw = {} if groups is None else {"groups": groups}
    return Runner(model=model, data=data, timer=None, log_fraction_initial_cases=-2.0, save_path="unused",
                  parameters=None, **kw)


def test_runner_construction_with_and_without_groups():
    plain = _runner()
    assert plain.group_keys == {} and "group_labels" not in plain.data["agent"]
    r = _runner(groups=["area", "ethnicity"])
    assert list(r.group_keys) == ["area", "ethnicity"]
    assert np.array_equal(r.group_keys["ethnicity"], r.ethnicities)          # get_cases_by_ethnicity's column order
    assert r.data["agent"].group_labels["area"].dtype == torch.int32
    # what Runner.get_data leaves on the agents for `groups_to_save` is picked up; `groups=` adds to it
    r = _runner(attach=["area"], groups={"ward": np.arange(769) % 4})
    assert list(r.group_keys) == ["area", "ward"] and r.group_keys["ward"].tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="age"):
        _runner(groups=["age"])
    with pytest.raises(KeyError, match="msoa"):
        _runner(groups=["msoa"])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32}


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in the header"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append(C.c_void_p if "*" in arg else _CTYPES[arg.replace("const ", "").split()[0]])
    return out


@pytest.mark.parametrize("name,n_args", [("gj_group_stats", 9), ("gj_adjoint_group_stats", 10)])
def test_bindings_have_the_declared_signatures(name, n_args):
    restype, argtypes = N.SYMBOLS[name]
    assert restype is C.c_int
    assert argtypes == _declared(name) and len(argtypes) == n_args


def test_abi_version_is_unchanged_and_the_constants_agree():
    src = open(HEADER).read()
    assert N.GJ_ABI_VERSION == 7 and "#define GJ_ABI_VERSION 7" in src
    assert "#define GJ_MAX_GROUPS (1 << 28)" in src and N.GJ_MAX_GROUPS == 1 << 28
    assert "#define GJ_GROUP_ERR_LABEL 1u" in src and "#define GJ_GROUP_ERR_VALUE 2u" in src
    assert (N.GJ_GROUP_ERR_LABEL, N.GJ_GROUP_ERR_VALUE) == (1, 2)


def test_argument_errors_come_before_any_device_work():
    lib = N.load()
    one = C.c_void_p(8)                                                     # never dereferenced: the checks refuse first
    assert lib.gj_group_stats(10, one, 0, one, one, 7, one, one, None) == -2          # n_groups < 1
    assert lib.gj_group_stats(-1, one, 3, one, one, 7, one, one, None) == -2
    assert lib.gj_group_stats(10, one, N.GJ_MAX_GROUPS + 1, one, one, 7, one, one, None) == -2
    assert lib.gj_group_stats(10, one, 3, one, one, 7, None, one, None) == -1         # out
    assert lib.gj_group_stats(10, one, 3, one, one, 7, one, None, None) == -1         # workspace
    assert lib.gj_group_stats(10, None, 3, one, one, 7, one, one, None) == -1         # labels
    assert lib.gj_group_stats(10, one, 3, None, one, 7, one, one, None) == -1
    assert lib.gj_group_stats(10, one, 3, one, None, 7, one, one, None) == -1
    assert lib.gj_group_stats(0, None, 3, None, None, 7, one, one, None) == 0         # nothing to add
    assert lib.gj_adjoint_group_stats(10, one, 0, one, 7, one, one, one, one, None) == -2
    assert lib.gj_adjoint_group_stats(-1, one, 3, one, 7, one, one, one, one, None) == -2
    assert lib.gj_adjoint_group_stats(10, None, 3, one, 7, one, one, one, one, None) == -1
    assert lib.gj_adjoint_group_stats(10, one, 3, None, 7, one, one, one, one, None) == -1    # stage, for grad_stage
    assert lib.gj_adjoint_group_stats(10, one, 3, one, 0, one, one, one, one, None) == -2     # x / dead
    assert lib.gj_adjoint_group_stats(10, one, 3, one, 7, one, one, None, None, None) == 0    # no output asked for
    assert lib.gj_adjoint_group_stats(0, None, 3, None, 7, None, None, None, None, None) == 0
