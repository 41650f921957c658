"""CPU: waning immunity's host side - schema, refusals, per-age tables - the closed form of the numpy restatement
(tests/gj_immunity_ref.py), the struct's layout and the entry points' argument checks.  The kernels are tested in
test_gpu_immunity.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import yaml

import gj_immunity_ref as R
from grad_june_amd import _native as N
from grad_june_amd.immunity import Immunity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gradjune_hip.h")
STAGES = ["recovered", "susceptible", "exposed", "infectious", "dead"]

CONFIG = """
immunity:
  half_life: {"0-50": 180, "50-100": .inf}
  residual_protection: 0.2
"""


def _params(text=CONFIG, stages=STAGES):
    params = yaml.safe_load(text) or {}
    params["system"] = {"device": "cpu"}
    params["symptoms"] = {"stages": stages}
    return params


def test_absent_key_is_none_and_the_package_exports_the_class():
    import grad_june_amd as G

    assert Immunity.from_parameters(_params("{}")) is None
    assert G.Immunity is Immunity


def test_a_number_beside_a_dict_is_broadcast_over_its_bands():
    im = Immunity.from_parameters(_params())
    assert im.half_life.dtype == torch.float32 and im.half_life.tolist() == [180.0, math.inf]
    assert im.residual_protection.dtype == torch.float32 and im.residual_protection.tolist() == [np.float32(0.2)] * 2
    assert im.band_of_age == [0] * 50 + [1] * 50 and im.n_bands == 2 and im.recovered_stage == 0
    other = Immunity(30, {"65-100": 0.5, "18-65": 0.1}, stages=["susceptible", "recovered"])      # file order
    assert other.half_life.tolist() == [30.0, 30.0] and other.residual_protection.tolist() == [0.5, np.float32(0.1)]
    assert other.band_of_age[17] == -1 and other.band_of_age[18] == 1 and other.band_of_age[65] == 0
    assert other.recovered_stage == 1


def test_plain_numbers_are_one_band_for_every_age():
    im = Immunity(90, 0.25)
    assert im.half_life.tolist() == [90.0] and im.residual_protection.tolist() == [0.25]
    assert im.band_of_age == [0] * 100
    assert Immunity(90).residual_protection.tolist() == [0.0]
    both = Immunity({"0-50": 10, "50-100": 20}, {"0-50": 0.1, "50-100": 0.3})
    assert both.half_life.tolist() == [10.0, 20.0] and both.residual_protection.tolist() == [np.float32(0.1), np.float32(0.3)]


@pytest.mark.parametrize("kwargs, match", [
    (dict(half_life=0), "half_life"),
    (dict(half_life=-3.0), "half_life"),
    (dict(half_life={"0-50": 10, "50-100": 0.0}), "half_life"),
    (dict(half_life=float("nan")), "half_life"),
    (dict(half_life=10, residual_protection=1.5), "residual_protection"),
    (dict(half_life=10, residual_protection={"0-50": -0.1}), "residual_protection"),
    (dict(half_life={"0-50": 10, "40-100": 20}), "overlapping"),
    (dict(half_life={"0-50": 10, "50-100": 20}, residual_protection={"50-100": 0.1, "0-50": 0.2}), "mismatched"),
    (dict(half_life={"0-50": 10, "50-100": 20}, residual_protection={"0-50": 0.1}), "mismatched"),
    (dict(half_life=10, stages=["susceptible", "infectious", "dead"]), "recovered"),
])
def test_refusals_say_which(kwargs, match):
    with pytest.raises(ValueError, match=match):
        Immunity(**kwargs)


def test_either_tensor_may_be_replaced_by_a_parameter():
    im = Immunity({"0-50": 10, "50-100": 20}, 0.5)
    assert not im.requires_grad()
    im.half_life = torch.nn.Parameter(torch.tensor([4.0, 8.0]))
    im.residual_protection = torch.nn.Parameter(torch.tensor([0.25, 0.75]))
    assert sorted(n for n, _ in im.named_parameters()) == ["half_life", "residual_protection"] and im.requires_grad()
    t = im.tables(4.0)
    assert t.keep[10] == 0.5 and t.keep[60] == np.float32(2.0 ** -0.5) and t.cap[10] == 0.75 and t.cap[60] == 0.25
    im.half_life = torch.nn.Parameter(torch.tensor([4.0]))
    with pytest.raises(ValueError, match="one value per band"):
        im.tables(1.0)
    im.half_life = torch.nn.Parameter(torch.tensor([4.0, -1.0]))      # a parameter an optimiser moved out of range
    with pytest.raises(ValueError, match="half_life"):
        im.tables(1.0)


def test_tables_are_rounded_once_and_match_the_restatement():
    im = Immunity({"18-65": 180, "65-100": math.inf, "5-18": 0.7}, {"18-65": 0.2, "65-100": 0.1, "5-18": 1.0})
    for dt in (1.0, 0.5, 1 / 3):
        t = im.tables(dt)
        cap, keep = R.tables(im.band_of_age, im.half_life.numpy(), im.residual_protection.numpy(), dt)
        assert np.array_equal(np.array(list(t.cap), dtype=np.float32), cap)
        assert np.array_equal(np.array(list(t.keep), dtype=np.float32), keep)
        assert keep[30] == np.float32(2.0 ** (-dt / 180.0)) and cap[30] == np.float32(1.0 - float(np.float32(0.2)))
        assert keep[70] == 1.0 and cap[70] == np.float32(1.0 - float(np.float32(0.1)))      # inf: never wanes
        assert keep[2] == 1.0 and cap[2] == 1.0                                             # a gap: no band
        assert keep[10] == np.float32(2.0 ** (-dt / float(np.float32(0.7)))) and cap[10] == 0.0


def test_closed_form_over_mixed_step_lengths():
    """From s = 0, 200 steps of 1 day and 0.5 day with h = 30: the float32 restatement against cap * (1 - 2^(-t / h)) in
    float64.  Each step rounds three times, each rounding at most 2^-24 relative of a value no larger than cap, and the
    error carried over contracts by keep <= 1: |difference| <= 3 * steps * 2^-24 * cap.  The float64 restatement of the
    same steps sits a thousand times closer (its only fp32 inputs are the tables, rounded once)."""
    h, r, steps = 30.0, 0.2, 200
    rng = np.random.default_rng(5)
    lengths = rng.choice([1.0, 0.5], steps)
    assert 40 < (lengths == 0.5).sum() < 160
    age, stage, inf = np.array([40]), np.array([0.0], dtype=np.float32), np.array([1.0], dtype=np.float32)
    cap = float(np.float32(1.0 - float(np.float32(r))))
    bound = 3 * steps * 2.0 ** -24 * cap
    s32, s64, t = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float64), 0.0
    worst = 0.0
    for dt in lengths:
        tabs = R.tables([0] * 100, [h], [r], dt)
        s32 = R.step(tabs, age, stage, 0, None, s32, inf)["susceptibility"]
        s64 = R.step64(tabs, age, stage, 0, None, s64, inf)["susceptibility"]
        t += dt
        worst = max(worst, abs(float(s32[0]) - R.closed_form(cap, t, h)))
        assert abs(float(s32[0]) - R.closed_form(cap, t, h)) <= bound, (t, float(s32[0]))
    assert 0 < float(s32[0]) < cap and t == lengths.sum()
    # the tables' one rounding of keep, compounded over the steps, is all that separates float64 steps from the closed form
    assert abs(float(s64[0]) - R.closed_form(cap, t, h)) <= steps * 2.0 ** -24 * cap
    print("closed form: largest difference", worst, "bound", bound)


def test_the_restatement_takes_each_branch():
    tabs = R.tables([0] * 50 + [-1] * 50, [2.0], [0.5], 2.0)      # keep 0.5, cap 0.5 below 50
    age = np.array([10, 10, 10, 10, 60, 10, 10, 10])
    stage = np.array([0, 0, 1, np.nan, 0, 0, 0, 2], dtype=np.float32)
    nw = np.array([0, 1, 0, 0, 0, 0, 1, 1], dtype=np.float32)
    s = np.array([0.0, 0.0, 0.25, 0.25, 0.25, 1.0, np.nan, 0.0], dtype=np.float32)
    inf = np.array([1, 2, 0, 1, 1, 1, 1, 3], dtype=np.float32)
    out = R.step(tabs, age, stage, 0, nw, s, inf)
    assert out["flags"].tolist() == [1, 2, 0, 0, 0, 1, 0, 2]
    assert out["susceptibility"].tolist()[:6] == [0.25, 0.0, 0.25, 0.25, 0.25, 0.75] and np.isnan(out["susceptibility"][6])
    assert out["is_infected"].tolist() == [1, 1, 0, 1, 1, 1, 1, 2] and out["count"] == 2
    assert out["susc_sum"] == int((0.25 * 4 + 0.75) * 2 ** 30)
    assert R.step(tabs, age, stage, 0, None, s, inf)["count"] == 0


def test_layout_equals_what_a_c_compiler_sees(tmp_path):
    import shutil
    import subprocess

    assert ctypes.sizeof(N.ImmunityTables) == 800
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gj_immunity_tables));']
    for field, _ in N.ImmunityTables._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(gj_immunity_tables, {field}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(N.ImmunityTables)
    for field, _ in N.ImmunityTables._fields_:
        assert int(got[field]) == getattr(N.ImmunityTables, field).offset, field


from test_launch_validation import lib  # noqa: E402,F401  (the fixture: the library, built if it is not there)


def test_the_abi_version_is_still_7(lib):  # noqa: F811
    assert N.GJ_ABI_VERSION == 7 and lib.gj_version() == 7
    assert hasattr(lib, "gj_immunity_step") and hasattr(lib, "gj_adjoint_immunity")


def test_the_entries_reject_bad_arguments_before_any_launch(lib):  # noqa: F811
    """The host never dereferences a device pointer: every case is rejected with a negative code before a launch (or,
    n == 0, returns at once)."""
    from test_launch_validation import E_NULL, E_RANGE, FAKE, OK

    t = N.ImmunityTables()
    step = lambda n=8, cls=FAKE, tab=t, stage=FAKE, rec=0, susc=FAKE, inf=FAKE: \
        lib.gj_immunity_step(n, cls, tab, stage, rec, None, susc, inf, None, None, None, None, None)
    assert lib.gj_immunity_step(0, None, None, None, 0, None, None, None, None, None, None, None, None) == OK
    assert step(n=-1) == E_RANGE and step(rec=-1) == E_RANGE and step(rec=N.GJ_MAX_STAGES) == E_RANGE
    assert step(cls=None) == E_NULL and step(tab=None) == E_NULL and step(stage=None) == E_NULL
    assert step(susc=None) == E_NULL and step(inf=None) == E_NULL
    plan = N.SeedPlan(8, 1, FAKE, FAKE, FAKE, FAKE)
    adj = lambda n=8, flags=FAKE, cls=FAKE, tab=t, s0=FAKE, band=FAKE, B=1, plan=plan, contrib=FAKE, partial=FAKE, \
        a=FAKE, b=FAKE: lib.gj_adjoint_immunity(n, flags, cls, tab, s0, None, None, band, B,
                                                 ctypes.byref(plan) if plan is not None else None, contrib, partial, a, b,
                                                 None, None, None, None)
    assert adj(n=-1) == E_RANGE and adj(B=0) == E_RANGE and adj(B=N.GJ_MAX_GROUPS + 1) == E_RANGE
    assert adj(a=None) == E_NULL and adj(b=None) == E_NULL and adj(plan=None) == E_NULL
    assert adj(flags=None) == E_NULL and adj(cls=None) == E_NULL and adj(tab=None) == E_NULL
    assert adj(s0=None) == E_NULL and adj(band=None) == E_NULL
    assert adj(contrib=None) == E_NULL and adj(partial=None) == E_NULL
    assert adj(plan=N.SeedPlan(9, 1, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more sorted agents than agents
    assert adj(plan=N.SeedPlan(8, 3, FAKE, FAKE, FAKE, FAKE)) == E_RANGE          # more chunks than the sizes allow
    assert adj(plan=N.SeedPlan(8, 1, None, FAKE, FAKE, FAKE)) == E_NULL
