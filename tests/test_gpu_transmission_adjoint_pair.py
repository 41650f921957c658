"""GPU: gj_adjoint_transmission and gj_adjoint_transmission_params are one kernel body, without and with the four
parameter outputs.  On the same inputs they must give the same grad_inf / grad_time bit for bit, and a call that asks for
some of the parameter outputs must give, in those, the bits of the call that asks for all."""
import ctypes as C

import pytest
import torch

from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

NOW = 10.0
KINDS = ("infected", "uninfected", "before_shift", "shape_one_at_shift", "nan_rate")
PARAM_OUTS = ("max_infectiousness", "shape", "rate", "shift")


def make_inputs(n, device, first_kind=0):
    """Agent i is of kind (first_kind + i) % 4 of the first four KINDS; with more than four agents, the middle one has a
    NaN rate."""
    g = torch.Generator().manual_seed(1000 + n)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    x = {"max_infectiousness": u(0.2, 2.0), "shape": u(0.5, 6.0), "rate": u(0.1, 1.5), "shift": u(0.0, 2.0),
         "infection_time": u(0.0, 7.0), "is_infected": torch.ones(n), "trans_bar": u(-1.0, 1.0), "g_inf": u(-1.0, 1.0),
         "grad_time": u(-1.0, 1.0)}
    kind = (first_kind + torch.arange(n)) % 4
    x["is_infected"][kind == 1] = 0.0
    x["shift"][kind == 2] = NOW + 1.0                       # t = now - infection_time < shift
    at = kind == 3                                          # shape == 1 and d * rate == 0: t == shift exactly
    x["shape"][at], x["infection_time"][at], x["shift"][at] = 1.0, 4.0, NOW - 4.0
    if first_kind == 4 or n > 4:
        x["rate"][n // 2] = float("nan")
    return {k: v.to(device) for k, v in x.items()}


def run(lib, x, outs=None):
    """outs None: gj_adjoint_transmission; else gj_adjoint_transmission_params writing the named parameter outputs."""
    n = x["trans_bar"].numel()
    st = N.AgentState()
    for k in ("max_infectiousness", "shape", "rate", "shift", "infection_time", "is_infected"):
        setattr(st, k, N.ptr(x[k]))
    r = {"inf": torch.full_like(x["trans_bar"], 7.0), "time": x["grad_time"].clone()}
    head = (n, C.byref(st), NOW, N.ptr(x["trans_bar"]), N.ptr(x["g_inf"]), N.ptr(r["inf"]), N.ptr(r["time"]))
    if outs is None:
        N.check(lib.gj_adjoint_transmission(*head, N.current_stream()), "gj_adjoint_transmission")
    else:
        for k in outs:
            r[k] = torch.full_like(x["trans_bar"], 7.0)
        N.check(lib.gj_adjoint_transmission_params(*head, *[N.ptr(r.get(k)) for k in PARAM_OUTS], N.current_stream()),
                "gj_adjoint_transmission_params")
    torch.cuda.synchronize()
    return r


def assert_same_bits(a, b, what):
    nan = torch.isnan(a)
    assert torch.equal(nan, torch.isnan(b)), what
    assert torch.equal(a[~nan], b[~nan]), what


@pytest.mark.parametrize("n,first_kind", [(1, k) for k in range(len(KINDS))] + [(255, 0), (257, 0)])
def test_both_entry_points_give_the_same_bits(device, n, first_kind):
    lib = N.load()
    x = make_inputs(n, device, first_kind)
    plain, full = run(lib, x), run(lib, x, PARAM_OUTS)
    if n > 4:                                               # the inputs hold every kind
        assert bool(torch.isnan(x["rate"]).any()) and bool((x["is_infected"] == 0).any())
        assert bool((x["shift"] > NOW).any()) and bool((x["shape"] == 1.0).any())
        assert bool(torch.isnan(full["inf"]).any()) and not bool(torch.isnan(full["inf"]).all())
    for k in ("inf", "time"):
        assert_same_bits(plain[k], full[k], (n, KINDS[first_kind], k))
    for outs in (("shape", "shift"), ("max_infectiousness",), ("rate",), ()):
        some = run(lib, x, outs)
        for k in ("inf", "time") + outs:
            assert_same_bits(some[k], full[k], (n, KINDS[first_kind], outs, k))
