"""CPU: the symptom-stage series - the C declarations of gj_stage_stats / gj_adjoint_stage_stats against the binding
table, their argument checks (which come before any device work) and the ``stages_to_save`` key of the YAML schema."""
import ctypes as C
import os
import re

import pytest

from grad_june_amd import _native as N
from grad_june_amd.groups import stages_to_save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gradjune_hip.h")
STAGES = ["recovered", "susceptible", "exposed", "infectious", "symptomatic", "severe", "critical", "dead"]
CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "float": C.c_float}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name,n_args", [("gj_stage_stats", 9), ("gj_adjoint_stage_stats", 10)])
def test_symbols_are_declared_in_the_header_and_the_binding_table(name, n_args):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in the header"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    restype, argtypes = N.SYMBOLS[name]
    assert restype is C.c_int and len(argtypes) == len(declared) == n_args
    for arg, ct in zip(declared, argtypes):
        if "*" in arg:
            assert ct is C.c_void_p, arg
        else:
            assert ct is CTYPES[arg.split()[0]], arg


def test_a_pure_addition_to_abi_7_and_the_exported_constants():
    src = _header()
    assert N.GJ_ABI_VERSION == 7 and "#define GJ_ABI_VERSION 7" in src
    for name in ("GJ_STAGE_ERR_LABEL", "GJ_STAGE_ERR_STAGE", "GJ_STAGE_LDS_BINS", "GJ_STAGE_ADJ_LDS_BINS",
                 "GJ_STAGE_LDS_THREADS", "GJ_STAGE_LDS_BLOCKS", "GJ_STAGE_GLOBAL_THREADS", "GJ_STAGE_GLOBAL_BLOCKS",
                 "GJ_STAGE_LANE_LOADS"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u?\s", src)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert "#define GJ_STAGE_MAX_AGENTS ((int64_t)1 << 40)" in src and N.GJ_STAGE_MAX_AGENTS == 1 << 40
    # 32-bit counters, two planes: the LDS regime's histogram is at most 64 KiB; an 8-bit field holds a lane's agents
    assert 2 * 4 * N.GJ_STAGE_LDS_BINS == 64 * 1024 and 4 * N.GJ_STAGE_LANE_LOADS + 1 < 256
    assert N.load().gj_version() == 7


def test_argument_errors_come_before_any_device_work():
    lib = N.load()
    one = C.c_void_p(8)                                            # never dereferenced: the checks refuse first

    def forward(n=10, group=one, G=3, S=8, stage=one, prev=one, out=one, err=one):
        return lib.gj_stage_stats(n, group, G, S, stage, prev, out, err, None)

    def adjoint(n=10, group=one, G=3, S=8, stage=one, prev=one, grad=one):
        return lib.gj_adjoint_stage_stats(n, group, G, S, stage, prev, one, one, grad, None)

    for call in (forward, adjoint):
        assert call(n=-1) == -2
        assert call(G=0) == -2 and call(G=N.GJ_MAX_GROUPS + 1) == -2
        assert call(S=0) == -2 and call(S=N.GJ_MAX_STAGES + 1) == -2
        assert call(G=N.GJ_MAX_GROUPS, S=8) == -2                  # 2^31 bins
        assert call(group=None, G=2) == -2                         # no labels: one group
        assert call(stage=None) == -1
        assert call(n=0) == 0 and call(n=0, group=None, G=1, prev=None) == 0
    assert forward(out=None) == -1 and forward(err=None) == -1
    assert adjoint(grad=None) == -1


# ---- stages_to_save ---------------------------------------------------------------------------------------------------
def test_stages_to_save_a_list_all_or_nothing():
    assert stages_to_save(["severe", "critical"], STAGES) == ["severe", "critical"]
    assert stages_to_save(("dead",), STAGES) == ["dead"]
    assert stages_to_save("all", STAGES) == STAGES
    assert stages_to_save("severe", STAGES) == ["severe"]
    assert stages_to_save(None, STAGES) == [] and stages_to_save([], STAGES) == []


def test_stages_to_save_refuses_unknown_and_shadowing_names():
    with pytest.raises(ValueError, match="hospitalised.*recovered.*dead"):      # the known names are listed
        stages_to_save(["severe", "hospitalised"], STAGES)
    for name in ("cases", "daily_cases", "deaths"):
        with pytest.raises(ValueError, match="shadow"):
            stages_to_save([name], STAGES + [name])
        with pytest.raises(ValueError, match="shadow"):
            stages_to_save("all", STAGES + [name])
    with pytest.raises(ValueError, match="shadow"):                  # new_<st> of one is <st> of the other
        stages_to_save(["severe", "new_severe"], STAGES + ["new_severe"])
    with pytest.raises(ValueError, match="twice"):
        stages_to_save(["severe", "severe"], STAGES)


class _Model:
    """What Runner.__init__ reads of a model."""
    device = "cpu"

    class symptoms_updater:
        class symptoms_sampler:
            stages = STAGES


def _runner(**kw):
    import torch

    from grad_june_amd.graph import HeteroData
    from grad_june_amd.runner import Runner

    data = HeteroData()
    ag = data["agent"]
    ag.id, ag.age, ag.sex = torch.arange(6), torch.tensor([5, 20, 30, 70, 80, 40]), torch.zeros(6, dtype=torch.long)
    ag.area = ["a", "b", "a", "b", "a", "c"]
    for k in Runner._STATE:
        ag[k] = torch.zeros(6)
    ag.symptoms = {k: torch.ones(6) for k in Runner._SYMPTOMS}
    return Runner(model=_Model(), data=data, timer=None, log_fraction_initial_cases=-2.0, save_path="unused",
                  parameters={}, **kw)


def test_runner_takes_the_stages_at_construction():
    plain = _runner()
    assert plain.stages_saved == [] and plain._stages() == {}        # absent: nothing to allocate, nothing to launch
    assert _runner(stages=["severe", "critical"]).stages_saved == ["severe", "critical"]
    assert _runner(stages="all", groups=["area"]).stages_saved == STAGES
    with pytest.raises(ValueError, match="no symptom stage"):
        _runner(stages=["severe", "ward"])


def test_from_parameters_passes_the_yaml_key(monkeypatch):
    """``stages_to_save`` reaches the constructor from the YAML schema; without the key there are no stage series."""
    from grad_june_amd import runner as R

    data = _runner().data
    monkeypatch.setattr(R.Runner, "get_data", staticmethod(lambda params: data))
    monkeypatch.setattr(R.GradJune, "from_parameters", classmethod(lambda cls, params: _Model()))
    monkeypatch.setattr(R.Timer, "from_parameters", classmethod(lambda cls, params: None))
    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused"}
    assert R.Runner.from_parameters(dict(params)).stages_saved == []
    assert R.Runner.from_parameters(dict(params, stages_to_save=["severe", "critical"])).stages_saved == ["severe", "critical"]
    assert R.Runner.from_parameters(dict(params, stages_to_save="all")).stages_saved == STAGES
    with pytest.raises(ValueError, match="known"):
        R.Runner.from_parameters(dict(params, stages_to_save=["icu"]))
