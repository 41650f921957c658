"""GPU: the transmission profile's kernels, called directly - gj_transmission_update, gj_quarantine_transmission,
gj_adjoint_transmission_params, gj_adjoint_transmission - per agent at the edges, against the fp64 reference of
tests/gj_profile_ref.py (the grid, d <= 0, the digamma points; K = 2 * K_REF of tests/test_profile_ref.py).

Every launch of a test reads the same agents ("the points"); an arrangement is an index map into them, so that a
value can be compared with the first launch's bit for bit."""
import ctypes as C
import functools

import pytest
import torch

import gj_profile_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

STATE_IN = R.FIELDS
SENTINEL = -77.0
BIG_N = 4 * 256 * 4096 + 1027       # the first n whose float4 body takes the grid-stride loop, with a 3-agent tail


@functools.lru_cache(maxsize=None)
def points():
    """The agents, their fp64 reference and the fp32 oracle's values, computed once on the CPU and left unchanged."""
    x, kinds = R.all_points()
    T32, g32 = R.oracle32(x)
    return {"x": x, "kinds": kinds, "ref": R.reference(x), "T32": T32, "g32": g32, "n": x["shape"].numel()}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def same_bits_nan_as_class(a, b):
    """equal bits where neither is NaN, NaN in the same places (a NaN's sign and payload depend on who produced it)"""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(bits(a)[~nan], bits(b)[~nan])


class Launch:
    """Device copies of an arrangement of the points and the two forward entry points on them."""

    def __init__(self, device, idx=None, *, is_infected=None, stage=None):
        P = points()
        idx = torch.arange(P["n"]) if idx is None else idx
        self.idx, self.n, self.device = idx, idx.numel(), device
        self.lib = N.load()
        self.t = {k: P["x"][k][idx].to(device) for k in STATE_IN}
        if is_infected is not None:
            self.t["is_infected"] = is_infected.to(device)
        self.t["susceptibility"] = torch.ones(self.n, device=device)
        self.t["current_stage"] = (torch.zeros(self.n) if stage is None else stage).to(device)
        self.t["transmission"] = torch.full((self.n,), SENTINEL, device=device)
        self.t["q_transmission"] = torch.full((self.n,), SENTINEL, device=device)

    def _call(self, fn, n, offset, now, has_q, thr, clock):
        assert 0 <= offset and offset + n <= self.n        # the launch reads and writes [offset, offset + n) only
        plan = N.Plan()
        plan.n_agents = plan.n_ext_agents = n
        st = N.AgentState()
        for k, v in self.t.items():
            setattr(st, k, v.data_ptr() + 4 * offset)
        p = N.StepParams()
        p.now, p.has_quarantine, p.q_threshold, p.clock = now, has_q, thr, clock
        N.check(getattr(self.lib, fn)(C.byref(plan), C.byref(st), C.byref(p), N.current_stream()), fn)

    def update(self, n=None, offset=0, now=R.NOW, has_q=0, thr=0.0, clock=None):
        """gj_transmission_update on agents [offset, offset + n); returns (transmission, q_transmission) of all, on the CPU"""
        self._call("gj_transmission_update", self.n if n is None else n, offset, now, has_q, thr, clock)
        torch.cuda.synchronize()
        return self.t["transmission"].cpu(), self.t["q_transmission"].cpu()

    def quarantine(self, n, thr):
        self._call("gj_quarantine_transmission", n, 0, R.NOW, 1, thr, None)
        torch.cuda.synchronize()
        return self.t["q_transmission"].cpu()


@pytest.fixture(scope="module")
def first(device):
    """the first launch: every point once, in order"""
    return Launch(device).update()[0]


def report(what, q, P):
    v, i = R.worst(q)
    at = {k: float(P["x"][k][i]) for k in ("shape", "rate")}
    print(f"{what}: max err / (B * allowance) = {v:.2f} at point {i} ({P['kinds'][i]}, {at}, d = {float(P['ref']['d'][i]):.6g})")
    return v


def test_forward_against_fp64(first):
    """|got - ref| <= K * B * |ref| on the comparable points, K * B * |ref| + floor and the fp32 oracle's inf / NaN
    elsewhere.  Measured on an MI355X: max err / (B * |ref|) = 0.67 on the comparable points (shape 1.56, d = 1e-3,
    rate 1), 0.41 with the floor elsewhere (K = 12)."""
    P = points()
    q, placed = R.check_forward(first, P["ref"], P["T32"])
    c = P["ref"]["comparable"]
    report("forward, comparable points", torch.where(c, q, torch.zeros_like(q)), P)
    report("forward, other points", torch.where(c, torch.zeros_like(q), q), P)
    bad = torch.nonzero(~placed).flatten().tolist()
    assert not bad, [(i, P["kinds"][i], float(first[i]), float(P["T32"][i]), float(P["ref"]["T"][i])) for i in bad]
    assert R.worst(q)[0] <= R.K


def arrangements():
    n = points()["n"]
    g = torch.Generator().manual_seed(7)
    yield "permuted", torch.randperm(n, generator=g)
    for r in (1, 2, 3):
        yield f"rotated by {r}", torch.roll(torch.arange(n), r)
    for k in (1, 2, 3):                     # n % 4 == k: the last k agents are the tail's; every agent of a stride
        m = n - (n - k) % 4
        assert m % 4 == k
        yield f"last {k} in the tail", torch.roll(torch.arange(n), 5 * k)[:m]
    for m in (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1025):
        yield f"n = {m}", torch.arange(m) % n


@pytest.mark.parametrize("name", [a[0] for a in arrangements()])
def test_slot_cannot_change_a_bit(device, first, name):
    idx = dict(arrangements())[name]
    got = Launch(device, idx).update()[0]
    assert same_bits(got, first[idx])


def test_every_agent_through_the_tail(device, first):
    """n = 1, 2 and 3 (no float4 group: block 0's tail alone) at every offset of the points"""
    L = Launch(device)
    for k in (1, 2, 3):
        L.t["transmission"].fill_(SENTINEL)
        for off in range(0, L.n - k + 1, k):
            L._call("gj_transmission_update", k, off, R.NOW, 0, 0.0, None)
        torch.cuda.synchronize()
        m = (L.n // k) * k
        got = L.t["transmission"].cpu()
        assert same_bits(got[:m], first[:m]), k
        assert bool((got[m:] == SENTINEL).all())


def test_grid_stride_loop(device, first):
    idx = torch.arange(BIG_N) % points()["n"]
    got = Launch(device, idx).update()[0]
    assert same_bits(got, first[idx])


def test_infection_patterns(device, first):
    """Over 64 consecutive float4 groups each of the 16 zero / non-zero patterns of is_infected four times, and a tail
    of three with the middle one uninfected."""
    n = 64 * 4 + 3
    idx = torch.arange(n)
    pattern = (torch.arange(64) * 5 + 3) % 16                     # a fixed order that holds each pattern four times
    assert torch.bincount(pattern, minlength=16).tolist() == [4] * 16
    on = ((pattern[:, None] >> torch.arange(4)[None, :]) & 1).reshape(-1).float()
    on = torch.cat([on, torch.tensor([1.0, 0.0, 1.0])])
    base = points()["x"]["is_infected"][idx]
    assert bool((base != 0).all())
    got = Launch(device, idx, is_infected=base * on).update()[0]
    assert bool((bits(got)[on == 0] == 0).all())                  # exactly +0.0
    assert same_bits(got[on != 0], first[idx][on != 0])
    none = Launch(device, idx, is_infected=torch.zeros(n)).update()[0]
    assert bool((bits(none) == 0).all())
    twice = Launch(device, idx, is_infected=2.0 * base).update()[0]
    assert same_bits_nan_as_class(twice, 2.0 * first[idx])


def stages(thr, n):
    t = torch.tensor(thr, dtype=torch.float32)
    five = torch.stack([torch.nextafter(t, torch.tensor(-1e9)), t, torch.nextafter(t, torch.tensor(1e9)),
                        torch.tensor(0.0), torch.tensor(float("nan"))])
    return five[torch.arange(n) % 5]


def test_quarantine(device, first):
    """Every point with each of the five stages (threshold -+ one ulp, the threshold, 0, NaN)."""
    P, thr = points(), 4.0
    idx = torch.arange(5 * P["n"]) // 5
    st = stages(thr, idx.numel())
    L = Launch(device, idx, stage=st)
    trans, q = L.update(has_q=1, thr=thr)
    assert same_bits(trans, first[idx])
    want = (st < thr).float() * trans
    assert bool(torch.isinf(trans).any()) and bool(torch.isnan(want[torch.isinf(trans)]).any())     # 0 * inf = NaN
    assert bool((st < thr).any()) and not bool((st[torch.isnan(st)] < thr).any())
    assert same_bits_nan_as_class(q, want)
    # without a quarantine policy q_transmission is not written
    L = Launch(device, idx, stage=st)
    trans, q = L.update(has_q=0, thr=thr)
    assert same_bits(trans, first[idx]) and bool((q == SENTINEL).all())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_quarantine_alone_gives_the_update_s_bits(device, n):
    thr = 4.0
    P = points()
    inf_at = P["kinds"].index("d0_frac")                            # shape 0.5 at d == 0: pow(0, -0.5) = inf
    idx = (torch.arange(n) + inf_at - min(n - 1, 1)) % P["n"]       # (an infinite transmission among them)
    st = stages(thr, n)
    st[min(n - 1, 1)] = thr                                         # ... masked out: 0 * inf
    L = Launch(device, idx, stage=st)
    trans, q1 = L.update(has_q=1, thr=thr)
    assert bool(torch.isinf(trans).any())
    L.t["q_transmission"].fill_(SENTINEL)
    q2 = L.quarantine(n, thr)
    assert same_bits(q1, q2) and bool(torch.isnan(q2).any())


def test_device_clock(device, first):
    """params.clock set: `now` is read from the gj_clock in device memory, params.now is ignored."""
    from grad_june_amd.engine import StepClock

    clock = StepClock(device)
    clock.set(R.NOW, 0)
    got = Launch(device).update(now=R.NOW - 7.5, clock=clock.ptr)[0]
    assert same_bits(got, first)
    other = Launch(device).update(now=R.NOW - 7.5)[0]
    assert not same_bits(other, first)


# ---- the adjoints ----------------------------------------------------------------------------------------------------
OUTS = {"max_infectiousness": "mx", "shape": "shape", "rate": "rate", "shift": "shift"}


@functools.lru_cache(maxsize=None)
def upstream():
    n = points()["n"]
    g = torch.Generator().manual_seed(11)
    u = lambda: -1.0 + 2.0 * torch.rand(n, generator=g)
    tb = u()
    tb = torch.where(tb.abs() < 0.05, torch.full_like(tb, 0.5), tb)      # (an upstream gradient away from 0)
    return {"trans_bar": tb, "g_inf": u(), "grad_time": u()}


def adjoint(device, idx, params=True):
    """gj_adjoint_transmission_params with all four outputs (or gj_adjoint_transmission) on an arrangement; CPU results
    keyed by the field the gradient is of."""
    P, U, lib = points(), upstream(), N.load()
    n = idx.numel()
    x = {k: P["x"][k][idx].to(device) for k in STATE_IN}
    up = {k: v[idx].to(device) for k, v in U.items()}
    st = N.AgentState()
    for k in STATE_IN:
        setattr(st, k, N.ptr(x[k]))
    r = {"is_infected": torch.full((n,), SENTINEL, device=device), "infection_time": up["grad_time"].clone()}
    head = (n, C.byref(st), R.NOW, N.ptr(up["trans_bar"]), N.ptr(up["g_inf"]), N.ptr(r["is_infected"]),
            N.ptr(r["infection_time"]))
    if params:
        for k in OUTS:
            r[k] = torch.full((n,), SENTINEL, device=device)
        N.check(lib.gj_adjoint_transmission_params(*head, *[N.ptr(r[k]) for k in OUTS], N.current_stream()),
                "gj_adjoint_transmission_params")
    else:
        N.check(lib.gj_adjoint_transmission(*head, N.current_stream()), "gj_adjoint_transmission")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


@pytest.fixture(scope="module")
def first_adjoint(device):
    return adjoint(device, torch.arange(points()["n"]))


def check_adjoint(got, k):
    P, U = points(), upstream()
    scope = R.partial_scope(P["kinds"], P["T32"])
    incoming = {"is_infected": U["g_inf"], "infection_time": U["grad_time"]}.get(k)
    return R.check_partial(k, got[k], P["ref"], scope, U["trans_bar"], incoming)


def test_adjoints_against_fp64(first_adjoint):
    """Each of the six results within K * B * allowance (tests/gj_profile_ref.py), NaN and inf exactly where fp64
    autograd has them; grad_time_inout and grad_inf as accumulations onto the incoming values.  Measured on an MI355X,
    max err / (B * allowance) on the comparable points: max_infectiousness 0.65, shape 2.38 (shape 1.56 at d * rate = 1,
    where ln u - psi(shape) is small), rate 0.67, shift 0.71, infection_time 0.62, is_infected 0.57 (K = 12)."""
    P = points()
    c = P["ref"]["comparable"]
    worst = {}
    for k in R.FIELDS:
        q, placed = check_adjoint(first_adjoint, k)
        worst[k] = report(f"d/d {k}, comparable points", torch.where(c, q, torch.zeros_like(q)), P)
        report(f"d/d {k}, other points", torch.where(c, torch.zeros_like(q), q), P)
        bad = torch.nonzero(~placed).flatten().tolist()
        assert not bad, (k, [(i, P["kinds"][i], float(P["x"]["shape"][i]), float(first_adjoint[k][i])) for i in bad])
        assert R.worst(q)[0] <= R.K, k
    # an uninfected agent would give 0 in every parameter output: the points are all infected, so none is the sentinel
    for k in OUTS:
        assert not bool((first_adjoint[k] == SENTINEL).any())


@pytest.mark.parametrize("n", [1, 255, 257])
def test_adjoints_at_launch_shapes(device, first_adjoint, n):
    P = points()
    idx = (torch.arange(n) + P["n"] - 40) % P["n"]          # (the edge and digamma points, then the grid's front)
    got = adjoint(device, idx)
    for k in R.FIELDS:
        assert same_bits(got[k], first_adjoint[k][idx]), k


def test_plain_adjoint_gives_the_same_two_results(device, first_adjoint):
    got = adjoint(device, torch.arange(points()["n"]), params=False)
    for k in ("is_infected", "infection_time"):
        assert same_bits(got[k], first_adjoint[k]), k


def test_d_zero_with_integer_shape(first_adjoint):
    """t == shift exactly with shape 1, 2, 3, 4: grad_time and grad_shift are finite and autograd's (+r T, -r^2 max_inf,
    0, 0 times the upstream gradient); T * ((shape - 1) / d - r) was NaN in all four."""
    P = points()
    m = torch.tensor([k == "d0_int" for k in P["kinds"]])
    assert P["x"]["shape"][m].tolist() == [1.0, 2.0, 3.0, 4.0]
    for k in ("infection_time", "shift"):
        got = first_adjoint[k][m]
        assert bool(torch.isfinite(got).all()), (k, got.tolist())
        q, placed = check_adjoint(first_adjoint, k)
        assert bool(placed[m].all()) and float(torch.nan_to_num(q[m]).max()) <= R.K, (k, got.tolist(), q[m].tolist())
    tb = upstream()["trans_bar"][m].double()
    want = tb * torch.tensor([0.36517, -0.36517, 0.0, 0.0], dtype=torch.float64)
    assert torch.allclose(first_adjoint["shift"][m].double(), want, rtol=0.0, atol=5e-6)
