"""GPU: the infection sampler's two elementwise kernels, called directly - gj_adjoint_sample and gj_sample_infect - per
agent at the edges, against the fp64 reference of tests/gj_sampler_ref.py (the grid over ts, dt, draws and susc0, the
named points; K = 2 * K_REF of tests/test_sampler_ref.py).  Randomness is injected (exp_noise) except in the one
consistency test of the library's own draws, whose values are not pinned."""
import functools

import numpy as np
import pytest
import torch

import gj_oracle as O
import gj_sampler_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
SEED, STEP = 20240611, 3
SHAPES = (1, 63, 64, 65, 255, 256, 257, 1027)
BIG_N = 65536 + 64                      # just above 65536 agents: 257 workgroups


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_bits_nan_as_class(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def kind_mask(pts, kind):
    return np.array([k == kind for k in pts["kinds"]])


def adjoint_sample(device, pts, idx=None, drop=(), zero=(), own=False, agent_offset=0, pad=0):
    """gj_adjoint_sample on the arrangement ``idx`` of a point set; the three outputs on the CPU.  ``drop``: cotangents
    passed as NULL; ``zero``: passed as explicit zero arrays; ``own``: exp_noise NULL (the library's draws); ``pad``:
    the launch reads and writes [pad, pad + n) of buffers of n + 2 * pad agents whose rest holds sentinels, and the
    whole buffers are returned."""
    idx = np.arange(pts["n"]) if idx is None else idx
    n, m = len(idx), len(idx) + 2 * pad
    src = pts

    def buf(v, fill=SENTINEL):
        full = np.full(m, fill, dtype=np.float32)
        full[pad:pad + n] = v
        return dev(full, device)

    x = {k: buf(src[k][idx]) for k in ("susc0", "time0", "acc")}
    g = {k: buf(np.zeros(n, dtype=np.float32) if k in zero else src[k][idx]) for k in R.COTANGENTS}
    noise = None
    if not own:                             # [2, n] contiguous: the rows are n apart, whatever the padding
        noise = dev(np.concatenate([src["e0"][idx], src["e1"][idx]]), device)
    out = {k: torch.full((m,), SENTINEL, device=device) for k in R.OUTPUTS}
    at = lambda t: t.data_ptr() + 4 * pad
    N.check(N.load().gj_adjoint_sample(
        n, at(x["susc0"]), at(x["time0"]), at(x["acc"]), N.ptr(noise), SEED, STEP, agent_offset, pts["now"], pts["dt"],
        *[None if k in drop else at(g[k]) for k in R.COTANGENTS], *[at(out[k]) for k in R.OUTPUTS], N.current_stream()),
        "gj_adjoint_sample")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def point_sets():
    return R.all_point_sets()


@pytest.fixture(scope="module")
def first(device):
    """the first launch of every point set: every point once, in order"""
    return [adjoint_sample(device, pts) for pts in point_sets()]


def kernel_decision(pts, got):
    """nu as the kernel took it, read from grad_time_out = g_time * (1 - nu): g_time is non-zero on every point"""
    nu = 1.0 - got["grad_time"].astype(np.float64) / pts["g_time"].astype(np.float64)
    assert np.isin(nu, (0.0, 1.0)).all()
    return nu


def test_adjoint_against_fp64(first):
    """Every point of the six launches: |got - ref| <= K * bound per output (bound: B carried to the output, tests/
    gj_sampler_ref.py), NaN exactly where the reference has one, no wrong sign, and the decision - read from
    grad_time_out - the fp64 decision on every safe point.  Exact: grad_time_out == g_time * (1 - nu) bit for bit;
    ts_bar == 0 (x_out == 0) outside the clamp, for a NaN ts and for a NaN softmax; x_out == 0 at p in {0, 1}
    (ts = 100 at dt = 2, ts = 1e-6 at dt = 0.01): torch's autograd gives NaN there (0 * inf in d nu / d p), the library
    documents 0 (include/gradjune_hip.h); h == 0.5 at the tie susc0 == nu, read from grad_susc_out where ts_bar == 0.
    Measured on an MI355X, max err / bound: x_out 0.34 (ts = 1e-6 and 2e-6, draws (5, 0.01)), grad_susc_out 0.47
    (ts * dt = 0.1, draws (0.3, 0.31): the fp32 restatement's own worst point and value), grad_time_out 0 (K = 1.0);
    4 of the 3294 points are unsafe (p below fp32's range at dt = 2) and none of them decided otherwise than fp64."""
    worst = {k: 0.0 for k in R.OUTPUTS}
    n = unsafe = 0
    for pts, got in zip(point_sets(), first):
        nu = kernel_decision(pts, got)
        ref = R.reference(pts, nu=nu)
        assert np.array_equal(nu[ref["safe"]], ref["nu64"][ref["safe"]]), pts["dt"]
        n, unsafe = n + pts["n"], unsafe + int((~ref["safe"]).sum())
        print(f"dt {pts['dt']:.4g}: unsafe points {int((~ref['safe']).sum())}, of which the kernel decided otherwise than fp64: "
              f"{int((nu != ref['nu64']).sum())}")
        for k in R.OUTPUTS:
            q, ok = R.excess(got[k], ref[k], ref["bound"][k])
            assert ok.all(), (pts["dt"], k, [(i, pts["kinds"][i], float(got[k][i]), float(ref[k][i])) for i in np.nonzero(~ok)[0][:8]])
            v, i = R.worst(q)
            print(f"dt {pts['dt']:.4g} {k}: max err / bound = {v:.3f} at point {i} ({pts['kinds'][i]}, ts = {float(ref['ts'][i]):.6g}, "
                  f"p = {float(ref['p'][i]):.9g}, draws ({float(pts['e0'][i]):.3g}, {float(pts['e1'][i]):.3g}))")
            worst[k] = max(worst[k], v)
            assert v <= R.K, (pts["dt"], k, i)
        # the rules the header states, exactly
        want_time = (pts["g_time"] * (np.float32(1.0) - nu.astype(np.float32))).astype(np.float32)
        assert same_bits(got["grad_time"], want_time)
        zero = ~ref["inside"] | np.isnan(ref["y0"])
        assert zero.any() and (got["x_out"][zero] == 0).all()
        flat = zero & np.isfinite(pts["acc"])                      # grad_susc_out = g_susc * h + 0 * acc there
        h = np.where(pts["susc0"] - nu > 0, 1.0, np.where(pts["susc0"] - nu == 0, 0.5, 0.0)).astype(np.float32)
        assert same_bits((got["grad_susc"][flat] + np.float32(0.0)), (pts["g_susc"] * h)[flat] + np.float32(0.0))
        assert (h[flat] == 0.5).any() and (h[flat] == 1.0).any() and (h[flat] == 0.0).any() or pts["n"] < 100
    for dt, kind in ((0.01, "p_one"), (2.0, "p_zero")):
        (pts, got), = [(p, g) for p, g in zip(point_sets(), first) if abs(p["dt"] - dt) < 1e-6]
        m = kind_mask(pts, kind)
        assert m.sum() == 2 and (got["x_out"][m] == 0).all()
    print("gj_adjoint_sample, max err / bound per output:", {k: round(v, 3) for k, v in worst.items()}, f"unsafe {unsafe} of {n}")


@pytest.mark.parametrize("null", R.COTANGENTS)
def test_null_cotangent_is_an_explicit_zero_array(device, null):
    pts = point_sets()[3]
    a = adjoint_sample(device, pts, drop=(null,))
    b = adjoint_sample(device, pts, zero=(null,))
    for k in R.OUTPUTS:
        assert same_bits(a[k], b[k]), k
    c = adjoint_sample(device, pts, drop=R.COTANGENTS)
    assert (c["x_out"] == 0).all() and (c["grad_time"] == 0).all()


def arrangement(n, n_points):
    return (np.arange(n) * 7 + 3) % n_points if n < n_points else np.arange(n) % n_points


@pytest.mark.parametrize("n", SHAPES + (BIG_N,))
def test_adjoint_launch_shape_cannot_change_a_bit(device, first, n):
    pts, one = point_sets()[1], first[1]
    idx = arrangement(n, pts["n"])
    got = adjoint_sample(device, pts, idx)
    for k in R.OUTPUTS:
        assert same_bits(got[k], one[k][idx]), k


def test_adjoint_at_an_offset_inside_a_larger_buffer(device, first):
    pts, one = point_sets()[1], first[1]
    pad = 37                                                        # (not a multiple of 4: no 16-byte alignment)
    got = adjoint_sample(device, pts, pad=pad)
    for k in R.OUTPUTS:
        assert same_bits(got[k][pad:-pad], one[k]), k
        assert (got[k][:pad] == SENTINEL).all() and (got[k][-pad:] == SENTINEL).all(), k


def sample_infect(device, p, e0=None, e1=None, state=None, now=R.UPDATE_NOW, agent_offset=0, pad=0, want_new=True):
    """gj_sample_infect on [pad, pad + n) of padded buffers; returns (new_infected, susc, inf, time) whole, on the CPU
    (None for what was not passed)."""
    n, m = len(p), len(p) + 2 * pad

    def buf(v):
        full = np.full(m, SENTINEL, dtype=np.float32)
        full[pad:pad + n] = v
        return dev(full, device)

    pd = buf(p)
    noise = None if e0 is None else dev(np.concatenate([e0, e1]).astype(np.float32), device)
    new = torch.full((m,), SENTINEL, device=device) if want_new else None
    st = [None] * 3 if state is None else [buf(state[k]) for k in ("susc", "inf", "time")]
    at = lambda t: None if t is None else t.data_ptr() + 4 * pad
    N.check(N.load().gj_sample_infect(n, at(pd), N.ptr(noise), SEED, STEP, agent_offset, now, at(new), *[at(t) for t in st],
                                      N.current_stream()), "gj_sample_infect")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in [new] + st)


def test_own_draws_adjoint_takes_the_forward_s_decision(device):
    """exp_noise NULL: with g_time = 1 and the other cotangents zero, 1 - grad_time_out is gj_sample_infect's
    new_infected for the same seed, step and agent_offset in {0, 5}.  Exact by construction, the second of the two ways:
    the forward is fed p = k * 2^-23 in [1/32, 1/16) and [1/8, 1/4), the adjoint ts = -ln(p) with susc0 = 1, dt = 1.
    Every theta is an odd multiple of 2^-24, so none lies within 2^-24 of these p - 16 and 4 of their ulp - while the
    adjoint's own p is within 5 and 3 ulp of them (ts rounds to 2^-24 of |ln p| <= 3.5, the product by dt = 1 is exact,
    expf is good to one ulp): p < theta is the same comparison in both.  The infected share is held to its
    expectation as a rate.  p == 0 (ts = 100, dt = 2) always infects, p == 1 (ts = 1e-6, dt = 0.01) never."""
    g = np.random.default_rng(17)
    n = BIG_N
    k = np.where(np.arange(n) % 2 == 0, g.integers(2 ** 18, 2 ** 19, n), g.integers(2 ** 20, 2 ** 21, n))
    p = (k * 2.0 ** -23).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), k * 2.0 ** -23)
    one, zero = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    pts = {"n": n, "dt": 1.0, "now": R.NOW, "susc0": one, "acc": (-np.log(p.astype(np.float64))).astype(np.float32),
           "time0": zero, "e0": one, "e1": one, "g_susc": zero, "g_inf": zero, "g_time": one, "g_new": zero}
    for offset in (0, 5):
        new = sample_infect(device, p, agent_offset=offset)[0]
        got = adjoint_sample(device, pts, own=True, agent_offset=offset)
        assert np.isin(new, (0.0, 1.0)).all()
        assert np.array_equal(1.0 - got["grad_time"], new), offset
        rate = new.mean()
        print(f"agent_offset {offset}: infected {rate:.4f} of {n}, expected {np.mean(1.0 - p):.4f}")
        assert abs(rate - np.mean(1.0 - p.astype(np.float64))) < 5.0 * np.sqrt(0.25 / n)
    # p == 0: always infected (theta > 0); p == 1: never (theta < 1)
    m = 257
    for dt, ts, p_const in ((2.0, 100.0, 0.0), (0.01, 1e-6, 1.0)):
        e = {"n": m, "dt": float(np.float32(dt)), "acc": np.full(m, ts, dtype=np.float32)}
        small = {k_: (v[:m] if isinstance(v, np.ndarray) else v) for k_, v in pts.items()}
        got = adjoint_sample(device, dict(small, **e), own=True, agent_offset=5)
        new = sample_infect(device, np.full(m, p_const, dtype=np.float32), agent_offset=5)[0]
        assert (new == 1.0 - p_const).all() and np.array_equal(1.0 - got["grad_time"], new)


# ---- gj_sample_infect with injected draws ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward():
    fp = R.forward_points()
    nu64, safe, ruled = R.forward_decision(fp)
    oracle = O.sample_infected(torch.from_numpy(fp["p"]), torch.from_numpy(np.stack([fp["e0"], fp["e1"]]))).numpy()
    return {"fp": fp, "nu64": nu64, "safe": safe, "ruled": ruled, "oracle": oracle, "state": R.forward_state(fp["n"])}


@pytest.fixture(scope="module")
def first_forward(device):
    F = forward()
    return sample_infect(device, F["fp"]["p"], F["fp"]["e0"], F["fp"]["e1"], state=F["state"])


def test_forward_decisions(first_forward):
    """new_infected is the fp64 decision, exactly 0.0 or 1.0, on every safe point (unsafe: at most 1 % of the points;
    measured 0); the exact tie p == 0.5, e0 == e1 decides 0; NaN p, p == 0, p == 1 and a draw of 0 give what
    oracle.sample_infected (torch) gives - NaN for a NaN p and for a draw of 0."""
    F, new = forward(), first_forward[0]
    fp, safe, ruled = F["fp"], F["safe"], F["ruled"]
    unsafe = ~safe & ~ruled
    print(f"gj_sample_infect: {fp['n']} points, unsafe {int(unsafe.sum())}, ruled {int(ruled.sum())}, "
          f"unsafe points decided otherwise than fp64: {int((new[unsafe] != F['nu64'][unsafe]).sum())}")
    assert unsafe.mean() <= R.MAX_UNSAFE_SHARE
    assert same_bits(new[safe], F["nu64"][safe].astype(np.float32))
    assert np.isin(new[unsafe], (0.0, 1.0)).all()
    tie = kind_mask(fp, "tie")
    assert tie.sum() == 3 and (bits(new[tie]) == 0).all()
    assert ruled.sum() >= 18 and same_bits_nan_as_class(new[ruled], F["oracle"][ruled])
    assert np.isnan(new[ruled]).sum() == 12 and (new[ruled] == 1).any() and (new[ruled] == 0).any()


def test_forward_state_update_is_the_unfused_sequence(first_forward):
    """max(0, s - nu), i + nu, t + nu * (now - t), each operation rounded on its own, bit for bit - infection times and
    `now` with full mantissas, so that t + (now - t) is not `now` (with nu in {0, 1} a contracted multiply-add gives
    the same bits: tests/test_sampler_ref.py) - on susceptibilities 0, 0.3, one ulp below 1, 1 and 2.5.  A NaN nu (a
    NaN p, a draw of 0) makes all three NaN, as torch.maximum(0, NaN) does - the susceptibility of these 12 agents was
    0 (fmaxf swallows a NaN) until this test.  Agents with nu == 0 keep their bits."""
    F = forward()
    new, got = first_forward[0], first_forward[1:]
    want = R.infect_unfused(F["state"], new)
    st = F["state"]
    moved = want[2] != np.float32(st["now"])
    assert (moved & (new == 1)).sum() > 100
    for g, w, k in zip(got, want, ("susc", "inf", "time")):
        assert same_bits_nan_as_class(g, w), k
        assert same_bits(g[new == 0], st[k][new == 0]), k
    nan = np.isnan(new)
    assert nan.sum() == 12 and all(np.isnan(g[nan]).all() for g in got)
    frac = (new == 1) & (st["susc"] == np.float32(0.3))
    assert frac.any() and (got[0][frac] == 0).all()
    over = (new == 1) & (st["susc"] == np.float32(2.5))
    assert over.any() and (got[0][over] == 1.5).all()


def test_forward_keeps_the_state_of_the_uninfected(device):
    """nu == 0 everywhere (p == 1): a NaN with a payload, -0.0 and a subnormal in the state survive bit for bit."""
    n = 300
    odd = np.array([0x7FC01234, 0x80000000, 0x00000001, 0xFFC00001, 0x3F800000], dtype=np.uint32).view(np.float32)
    st = {k: odd[(np.arange(n) + s) % 5] for s, k in enumerate(("susc", "inf", "time"))}
    e = np.ones(n, dtype=np.float32)
    new, *got = sample_infect(device, e, 0.5 * e, 2.0 * e, state=st)
    assert (bits(new) == 0).all()
    for g, k in zip(got, ("susc", "inf", "time")):
        assert same_bits(g, st[k]), k


def test_forward_without_state_writes_new_infected_only(device, first_forward):
    fp = forward()["fp"]
    alone = sample_infect(device, fp["p"], fp["e0"], fp["e1"])
    assert alone[1:] == (None, None, None) and same_bits_nan_as_class(alone[0], first_forward[0])


@pytest.mark.parametrize("n", SHAPES + (BIG_N,))
def test_forward_launch_shape_cannot_change_a_bit(device, first_forward, n):
    F = forward()
    fp, st = F["fp"], F["state"]
    idx = arrangement(n, fp["n"])
    got = sample_infect(device, fp["p"][idx], fp["e0"][idx], fp["e1"][idx], state={k: st[k][idx] for k in ("susc", "inf", "time")})
    for g, w in zip(got, first_forward):
        assert same_bits_nan_as_class(g, w[idx])


def test_forward_at_an_offset_inside_a_larger_buffer(device, first_forward):
    F, pad = forward(), 37
    fp = F["fp"]
    got = sample_infect(device, fp["p"], fp["e0"], fp["e1"], state=F["state"], pad=pad)
    for g, w in zip(got, first_forward):
        assert same_bits_nan_as_class(g[pad:-pad], w)
        assert (g[:pad] == SENTINEL).all() and (g[-pad:] == SENTINEL).all()
