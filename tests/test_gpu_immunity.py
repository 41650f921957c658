"""GPU: waning immunity.  gj_immunity_step and gj_adjoint_immunity against their numpy restatement
(tests/gj_immunity_ref.py) over the shapes at which the kernels change form, then the whole model: the Runner with the
``immunity`` key against the same model without it, where the test itself applies the rule with torch ops between the
step and the symptoms update - series and final state bit for bit, the two gradients against autograd through the torch
ops - the half-life end to end, a config without the key, and two gloo ranks against one GPU."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import gj_immunity_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

RECOVERED, DEAD = 0, 7
#: ages 0-4: a gap; 65-100 never wanes
HALF_LIFE = {"18-65": 30.0, "65-100": math.inf, "5-18": 7.5}
RESIDUAL = {"18-65": 0.2, "65-100": 0.1, "5-18": 0.5}


def _bands():
    from grad_june_amd.utils import parse_age_probabilities

    return [int(b) for b in parse_age_probabilities({k: i for i, k in enumerate(HALF_LIFE)}, fill_value=-1)]


def _tables(dt=1.0):
    return R.tables(_bands(), list(HALF_LIFE.values()), list(RESIDUAL.values()), dt)


def _c_tables(tabs):
    t = N.ImmunityTables()
    t.cap[:] = [float(v) for v in tabs[0]]
    t.keep[:] = [float(v) for v in tabs[1]]
    return t


class Shifted:
    """Device copies of host arrays, either as allocated (16-byte aligned: four agents per lane) or one element into a
    longer allocation (no alignment: one agent per lane)."""

    def __init__(self, device, shift):
        self.device, self.shift = device, int(shift)

    def __call__(self, a, dtype=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if not self.shift:
            return torch.from_numpy(a).to(self.device)
        buf = torch.zeros(len(a) + 1, dtype=torch.from_numpy(a).dtype, device=self.device)
        buf[1:] = torch.from_numpy(a).to(self.device)
        return buf[1:]

    def full(self, n, value, dtype):
        return self(np.full(n, value, dtype=dtype))


def _agents(n, rng, tabs):
    """Ages in bands and in gaps; recovered, susceptible, infected and dead stages and a NaN stage; susceptibility at 0, at
    cap, above cap, NaN and in between; is_infected in 0 .. 3 with new_infected 0 / 1.  The first agents are fixed by hand
    so that the smallest n too meets a waning agent, and n >= 8 every combination of 'had one before' x 'new now'."""
    age = rng.integers(0, 100, n)
    stage = rng.choice(np.array([RECOVERED, 1, 3, DEAD, np.nan], dtype=np.float32), n, p=[0.5, 0.2, 0.15, 0.1, 0.05])
    inf = rng.integers(0, 4, n).astype(np.float32)
    nw = (rng.random(n) < 0.3).astype(np.float32)
    hand = [(30, RECOVERED, 1, 0), (40, RECOVERED, 1, 1), (50, 1, 0, 1), (10, 3, 2, 1), (70, RECOVERED, 3, 0),
            (2, RECOVERED, 1, 0), (33, 1, 0, 0), (12, np.nan, 2, 0)]
    for i, (a, st, f, w) in enumerate(hand[:n]):
        age[i], stage[i], inf[i], nw[i] = a, st, f + w, w      # (the step already added the new infection)
    cap = tabs[0][age]
    kind = rng.integers(0, 5, n)
    susc = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                     [np.zeros(n), cap, cap + 0.25, np.full(n, np.nan)], rng.random(n)).astype(np.float32)
    if n:
        susc[0] = 0.0
    cls = (rng.integers(0, 2, n) * 100 + age).astype(np.uint8)
    return cls, age, stage, nw, susc, inf


def _step(dev, cls, tabs, stage, nw, susc, inf, outputs=True, count_start=0, sum_start=0):
    n = len(cls)
    k, st, w, s, f = dev(cls), dev(stage), dev(nw), dev(susc), dev(inf)
    flags = dev.full(n, 0xEE, np.uint8) if outputs else None
    reinf = dev.full(n, np.nan, np.float32) if outputs else None
    count = torch.tensor([count_start], dtype=torch.int64, device=dev.device) if outputs else None
    total = torch.tensor([sum_start], dtype=torch.int64, device=dev.device) if outputs else None
    N.check(N.load().gj_immunity_step(n, N.ptr(k), _c_tables(tabs), N.ptr(st), RECOVERED, N.ptr(w), N.ptr(s), N.ptr(f),
                                      N.ptr(flags), N.ptr(reinf), N.ptr(count), N.ptr(total), N.current_stream()),
            "gj_immunity_step")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return {"susceptibility": host(s), "is_infected": host(f), "flags": host(flags), "reinfected": host(reinf),
            "count": None if count is None else int(count.item()), "susc_sum": None if total is None else int(total.item())}


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003, 9001])
def test_kernel_against_the_restatement(device, n):
    """Updated susceptibility and is_infected bit for bit, flags_out and reinfected_out equal, count_out and susc_sum_out
    exact and added onto non-zero starts, every optional output accepted as NULL, new_infected NULL = nobody (9001: several
    workgroups of 1024 lanes in either form).  Aligned arrays (four agents per lane) and arrays one element into their
    allocation (one agent per lane); step lengths 1 and 0.5; a launch in which nobody wanes or is reinfected leaves both
    arrays' bits as they were."""
    rng = np.random.default_rng(300 + n)
    seen = np.zeros(4, dtype=np.int64)
    for shift, dt in itertools.product((0, 1), (1.0, 0.5)):
        dev = Shifted(device, shift)
        tabs = _tables(dt)
        cls, age, stage, nw, susc, inf = _agents(n, rng, tabs)
        ref = R.step(tabs, age, stage, RECOVERED, nw, susc, inf)
        got = _step(dev, cls, tabs, stage, nw, susc, inf, count_start=1000, sum_start=5000)
        assert _same_bits(got["susceptibility"], ref["susceptibility"]), (shift, dt)
        assert _same_bits(got["is_infected"], ref["is_infected"]), (shift, dt)
        assert np.array_equal(got["flags"], ref["flags"]) and np.array_equal(got["reinfected"], ref["reinfected"])
        assert got["count"] == 1000 + ref["count"] and got["susc_sum"] == 5000 + ref["susc_sum"]
        bare = _step(dev, cls, tabs, stage, nw, susc, inf, outputs=False)
        assert bare["flags"] is None and bare["count"] is None
        assert _same_bits(bare["susceptibility"], ref["susceptibility"]) and _same_bits(bare["is_infected"], ref["is_infected"])
        # new_infected NULL: nobody is newly infected
        ref0 = R.step(tabs, age, stage, RECOVERED, None, susc, inf)
        k, st, s, f = dev(cls), dev(stage), dev(susc), dev(inf)
        fl = dev.full(n, 0xEE, np.uint8)
        N.check(N.load().gj_immunity_step(n, N.ptr(k), _c_tables(tabs), N.ptr(st), RECOVERED, None, N.ptr(s), N.ptr(f),
                                          N.ptr(fl), None, None, None, N.current_stream()), "gj_immunity_step")
        assert _same_bits(s.cpu().numpy(), ref0["susceptibility"]) and _same_bits(f.cpu().numpy(), inf)
        assert np.array_equal(fl.cpu().numpy(), ref0["flags"]) and ref0["count"] == 0
        # nobody wanes (every keep = 1) and nobody is newly infected: not a bit moves
        still = (tabs[0], np.ones(100, dtype=np.float32))
        idle = _step(dev, cls, still, stage, np.zeros(n, dtype=np.float32), susc, inf, sum_start=7)
        assert _same_bits(idle["susceptibility"], susc) and _same_bits(idle["is_infected"], inf)
        assert not idle["flags"].any() and not idle["reinfected"].any() and idle["count"] == 0
        assert idle["susc_sum"] == 7 + R.step(still, age, stage, RECOVERED, None, susc, inf)["susc_sum"]
        # the four combinations of "had an infection before" x "new now", and the waning agents
        before = (inf - nw) >= 1
        for i, (b, w) in enumerate(itertools.product((False, True), (False, True))):
            seen[i] += int((before == b)[nw == w].sum())
        assert (ref["flags"] & R.WANED).any() or n < 1
        if n >= 63:
            waned = (ref["flags"] & R.WANED) != 0
            assert (ref["flags"] & R.REINFECTED).any() and ref["count"] < int((nw != 0).sum())
            assert not waned[(age < 5) | (age >= 65)].any()                       # a gap, and the band that never wanes
            assert (ref["susceptibility"][waned] < susc[waned]).any()            # above cap: downward
            if n >= 257:
                assert np.isnan(ref["susceptibility"][waned]).any()               # a NaN stays a NaN
                assert (waned & (age >= 5) & (age < 18)).any() and (waned & (age >= 18)).any()      # both waning bands
    assert n < 8 or seen.min() > 0


def _adjoint(dev, tabs, flags, cls, susc0, g_susc, g_inf, band, n_bands, outputs=True):
    from grad_june_amd.groups import SeedPlan

    n = len(cls)
    lab = dev(band, np.int32)
    plan = SeedPlan(lab, n_bands, device=dev.device)
    nan64 = lambda m: torch.full((max(1, m),), float("nan"), dtype=torch.float64, device=dev.device)
    contrib, partial, sums = nan64(2 * n), nan64(2 * plan.n_chunks), nan64(2 * n_bands)
    outs = [dev.full(n, np.nan, np.float32) if outputs else None for _ in range(3)]
    keep = [dev(flags), dev(cls), dev(susc0), dev(g_susc), dev(g_inf)]
    N.check(N.load().gj_adjoint_immunity(n, N.ptr(keep[0]), N.ptr(keep[1]), _c_tables(tabs), N.ptr(keep[2]),
                                         N.ptr(keep[3]), N.ptr(keep[4]), N.ptr(lab), n_bands, C.byref(plan.c),
                                         N.ptr(contrib), N.ptr(partial), N.ptr(sums[:n_bands]), N.ptr(sums[n_bands:]),
                                         *[N.ptr(o) for o in outs], N.current_stream()), "gj_adjoint_immunity")
    torch.cuda.synchronize()
    sums = sums.cpu().numpy()
    return {"sum_A": sums[:n_bands], "sum_B": sums[n_bands:], "plan": plan,
            **{k: None if o is None else o.cpu().numpy() for k, o in zip(("g_susc_in", "g_inf_in", "g_new"), outs)}}


def _check_adjoint(device, tabs, flags, cls, age, susc0, g_susc, g_inf, band, n_bands):
    """Aligned and shifted, cotangents given and NULL: the three per-agent gradients the restatement's bit for bit; sum_A
    and sum_B equal to the float64 sums of the float64 terms, added in the plan's order; two launches the same bits."""
    for shift, given in itertools.product((0, 1), (True, False)):
        dev = Shifted(device, shift)
        gs, gi = (g_susc, g_inf) if given else (None, None)
        ref = R.adjoint(tabs, flags, age, susc0, gs, gi, band, n_bands)
        got = _adjoint(dev, tabs, flags, cls, susc0, gs, gi, band, n_bands)
        again = _adjoint(dev, tabs, flags, cls, susc0, gs, gi, band, n_bands, outputs=False)
        assert again["g_new"] is None
        for k in ("sum_A", "sum_B"):
            assert np.array_equal(got[k].view(np.int64), again[k].view(np.int64)), "two launches differ"
            assert np.array_equal(got[k], ref[k]), (k, shift, given, got[k], ref[k])
        for k in ("g_susc_in", "g_inf_in", "g_new"):
            assert _same_bits(got[k], ref[k]), (k, shift, given)
        if not given:
            assert not got["sum_A"].any() and not got["sum_B"].any() and not got["g_susc_in"].any()
    return R.adjoint(tabs, flags, age, susc0, g_susc, g_inf, band, n_bands)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003])
def test_adjoint_against_the_restatement(device, n):
    """The flags of the forward on the same agents, random cotangents, the bands as the module forms them (each agent's
    age's band; some agents by hand have none: they contribute nothing).  Every band fits one chunk of the plan."""
    rng = np.random.default_rng(400 + n)
    tabs = _tables(1.0)
    cls, age, stage, nw, susc0, inf = _agents(n, rng, tabs)
    susc0 = np.where(np.isnan(susc0), np.float32(1.5), susc0)      # (a NaN would make its band's sum_A a NaN on both sides)
    flags = R.step(tabs, age, stage, RECOVERED, nw, susc0, inf)["flags"]
    g_susc, g_inf = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    band = np.asarray(_bands())[age]
    waned = (flags & R.WANED) != 0
    if n > 1:      # labels outside [0, 3): no band, never an index - for every third waning agent, and some of the others
        band[np.flatnonzero(waned)[1::3]] = band[3::7] = [-1, 3, 2 ** 31 - 1][n % 3]
    ref = _check_adjoint(device, tabs, flags, cls, age, susc0, g_susc, g_inf, band, 3)
    assert waned.any() and np.isfinite(ref["sum_A"]).all()
    if n >= 63:
        lost = waned & ((band < 0) | (band >= 3))
        assert np.abs(ref["sum_A"]).sum() > 0 and np.abs(ref["sum_B"]).sum() > 0 and lost.any()
        assert not ref["term_A"][lost].any() and not ref["term_B"][lost].any()
        # with every agent in its age's band the sums differ: the agents without a band were left out, not misfiled
        full = R.adjoint(tabs, flags, age, susc0, g_susc, g_inf, np.asarray(_bands())[age], 3)
        assert not np.array_equal(full["sum_B"], ref["sum_B"])


@pytest.mark.parametrize("which", ["one-2500", "mixed", "mixed-sorted"])
def test_adjoint_bands_of_several_chunks(device, which):
    """Bands that span several (band, chunk) partials of GJ_SEED_CHUNK = 1024 agents: one band of 2500 (3 chunks), and
    sizes 3000, 1, 0, 1025, 1024, 950, 2049 - shuffled and sorted - next to 500 agents with no band.  Every agent wanes,
    so every term counts; the sums equal the restatement's in the plan's order."""
    rng = np.random.default_rng(len(which))
    if which == "one-2500":
        n_bands, band = 1, np.zeros(2500, dtype=np.int64)
    else:
        sizes = [3000, 1, 0, 1025, 1024, 950, 2049]
        n_bands = len(sizes)
        band = rng.permutation(np.concatenate((np.repeat(np.arange(n_bands), sizes), np.full(500, -1))))
        if which == "mixed-sorted":
            band = np.sort(band)
    n = len(band)
    tabs = _tables(1.0)
    age = rng.integers(5, 65, n)
    cls = age.astype(np.uint8)
    susc0 = rng.random(n).astype(np.float32)
    flags = R.step(tabs, age, np.zeros(n, dtype=np.float32), RECOVERED, None, susc0, np.ones(n, dtype=np.float32))["flags"]
    assert (flags == R.WANED).all()
    g_susc, g_inf = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ref = _check_adjoint(device, tabs, flags, cls, age, susc0, g_susc, g_inf, band, n_bands)
    plan = _adjoint(Shifted(device, 0), tabs, flags, cls, susc0, g_susc, g_inf, band, n_bands)["plan"]
    sizes = np.bincount(band[band >= 0], minlength=n_bands)
    assert plan.n_chunks == int(np.ceil(sizes / N.GJ_SEED_CHUNK).sum()) and plan.n_sorted == int(sizes.sum())
    # against plain float64 sums: the order moves the last bits only
    for k, t in (("sum_A", "term_A"), ("sum_B", "term_B")):
        plain = np.bincount(band[band >= 0], weights=ref[t][band >= 0], minlength=n_bands)
        scale = np.bincount(band[band >= 0], weights=np.abs(ref[t][band >= 0]), minlength=n_bands)
        assert np.all(np.abs(ref[k] - plain) <= 1e-13 * scale)


# ---- the half-life, through the Python layer ------------------------------------------------------------------------------
def test_half_life_end_to_end(device):
    """One agent, infected at the start (susceptibility 0, is_infected 1) and forced to ``recovered``, stepped with dt = 1
    for h = 30 days through ``Immunity.step``: its susceptibility is the float32 restatement's bit for bit and within
    3 * steps * 2^-24 * cap of cap / 2 (test_immunity.py derives the bound); the agents around it - susceptible, infected,
    dead - keep their bits."""
    from grad_june_amd.immunity import Immunity

    h, r = 30, 0.2
    im = Immunity(h, r, stages=["recovered", "susceptible", "exposed", "infectious", "dead"])
    stage = torch.tensor([1.0, 3.0, 0.0, 4.0, 1.0], device=device)
    start = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.75], device=device)
    data = {"agent": {"age": torch.tensor([30, 31, 32, 33, 34], device=device), "sex": torch.zeros(5, dtype=torch.long, device=device),
                      "susceptibility": start.clone(), "is_infected": torch.tensor([0.0, 1.0, 1.0, 1.0, 0.0], device=device),
                      "symptoms": {"current_stage": stage}}}
    tabs = R.tables([0] * 100, [h], [r], 1.0)
    ref = np.zeros(1, dtype=np.float32)
    with torch.no_grad():
        for _ in range(h):
            im.step(data, 1.0, torch.zeros(5, device=device))
            ref = R.step(tabs, [32], [0.0], 0, None, ref, [1.0])["susceptibility"]
    got = data["agent"]["susceptibility"].cpu().numpy()
    cap = float(np.float32(1.0 - float(np.float32(r))))
    assert _same_bits(got[2:3], ref)
    assert abs(float(got[2]) - cap / 2) <= 3 * h * 2.0 ** -24 * cap, (float(got[2]), cap / 2)
    assert _same_bits(got[[0, 1, 3, 4]], start.cpu().numpy()[[0, 1, 3, 4]])
    assert data["agent"]["is_infected"].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


# ---- the whole model ----------------------------------------------------------------------------------------------------
IMMUNITY = {"half_life": {"0-40": 2.0, "40-100": 3.0}, "residual_protection": 0.1}
#: a third band that never wanes: its gradients are exactly 0
IMMUNITY_3 = {"half_life": {"0-40": 2.0, "40-70": 3.0, "70-100": math.inf}, "residual_protection": 0.1}
DAYS, LOG_FRACTION, LOG_BETA_SHIFT = 40, -2.0, 1.0
GRAD_DAYS = 30


def _params(device, immunity=None, days=DAYS, groups=None, save_path=None):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = LOG_FRACTION
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += LOG_BETA_SHIFT
    if immunity is not None:
        p["immunity"] = immunity
    if groups:
        p["groups_to_save"] = list(groups)
    if save_path is not None:
        p["save_path"] = str(save_path)
    return p


def _fresh_runner(device, seed=21, cls=None, **kw):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return (cls or G.Runner).from_parameters(_params(device, **kw))


def _log_beta_parameters(runner):
    nets = runner.model.infection_networks.networks
    for net in nets.values():
        net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    return [net.log_beta for net in nets.values()]


class Emulation:
    """The rule restated with torch ops on a model WITHOUT the key: a forward pre-hook of the model's symptoms updater,
    armed while ``model(data, timer)`` runs (the seed calls the updater too), applies it between the step and the symptoms
    update.  The per-agent update is three float32 ops, as the kernel's; ``half_life`` / ``residual`` are float64 leaves
    [B] whose gradient comes through a float64 restatement of the same expression that adds an exact zero to the value."""

    def __init__(self, runner, immunity):
        from grad_june_amd.immunity import Immunity

        self.runner, dev = runner, runner.device
        self.parsed = Immunity(immunity["half_life"], immunity["residual_protection"],
                               stages=runner.model.symptoms_updater.symptoms_sampler.stages)
        self.half_life = self.parsed.half_life.double().to(dev).requires_grad_(True)
        self.residual = self.parsed.residual_protection.double().to(dev).requires_grad_(True)
        self.age = runner.data["agent"].age.to(dev).long()
        self.band = torch.tensor(self.parsed.band_of_age, device=dev)[self.age]
        self.armed = False
        runner.model.register_forward_pre_hook(self._arm)
        runner.model.register_forward_hook(self._disarm)
        runner.model.symptoms_updater.register_forward_pre_hook(self, with_kwargs=True)

    def reset(self):
        self.reinfections, self.susc_sums, self.both, self.waning = [0], [], 0, []

    @staticmethod
    def _fixed(s):
        zero, four = torch.zeros((), device=s.device), torch.full((), 4.0, device=s.device)
        return int((torch.fmin(torch.fmax(s.detach(), zero), four) * float(1 << 30)).long().sum().item())

    def _arm(self, model, args):
        self.armed = True
        if not self.susc_sums:      # row 0: the state the seed left
            self.susc_sums.append(self._fixed(args[0]["agent"].susceptibility.float()))

    def _disarm(self, model, args, out):
        self.armed = False

    def __call__(self, updater, args, kwargs):
        if not self.armed:
            return None
        ag, dt, nw = kwargs["data"]["agent"], kwargs["timer"].duration, kwargs["new_infected"]
        dev = self.runner.device
        cap_t, keep_t = R.tables(self.parsed.band_of_age, self.parsed.half_life.numpy(),
                                 self.parsed.residual_protection.numpy(), dt)
        cap, keep = torch.from_numpy(cap_t).to(dev)[self.age], torch.from_numpy(keep_t).to(dev)[self.age]
        stage = ag.symptoms["current_stage"].detach()
        s, inf = ag.susceptibility, ag.is_infected
        nu = nw.detach() != 0
        waned = (stage == float(self.parsed.recovered_stage)) & ~nu & (keep != 1)
        relaxed = cap - (cap - s) * keep                                   # three float32 ops
        if torch.is_grad_enabled():
            b = self.band.clamp(min=0)
            keep64 = torch.where(self.band >= 0, 2.0 ** (-dt / self.half_life[b]), torch.ones((), dtype=torch.float64, device=dev))
            cap64 = torch.where(self.band >= 0, 1.0 - self.residual[b], torch.ones((), dtype=torch.float64, device=dev))
            relaxed64 = cap64 - (cap64 - s.detach().double()) * keep64
            relaxed = relaxed + (relaxed64 - relaxed64.detach()).float()      # + 0, carrying d / d half_life, d / d residual
        before = inf - nw
        reinfected = nu & (before.detach() >= 1)
        ag.susceptibility = torch.where(waned, relaxed, s)
        ag.is_infected = torch.where(reinfected, before, inf)
        self.reinfections.append(int(reinfected.sum().item()))
        self.waning.append(int(waned.sum().item()))
        self.both += int(reinfected.any().item() and waned.any().item())
        self.susc_sums.append(self._fixed(ag.susceptibility))
        return None


def _run_pair(device, immunity, grad, groups=None, days=DAYS):
    """(results and is_infected of run A, the Runner with the key; of run B, the emulation; A's runner; B's runner; B's
    hook; the log_beta parameters of A and of B)."""
    from grad_june_amd import infection

    a = _fresh_runner(device, immunity=immunity, groups=groups, days=days)
    b = _fresh_runner(device, groups=groups, days=days)
    hook = Emulation(b, immunity)
    params_a = params_b = None
    if grad:
        im = a.model.immunity
        im.half_life = torch.nn.Parameter(im.half_life.detach().clone())
        im.residual_protection = torch.nn.Parameter(im.residual_protection.detach().clone())
        params_a, params_b = _log_beta_parameters(a), _log_beta_parameters(b)
    out = []
    for runner in (a, b):
        torch.manual_seed(21)
        infection._philox_step = itertools.count(1 << 40)      # the seeding's Philox stream: the same for both
        hook.reset()
        with torch.set_grad_enabled(grad):
            out.append(runner())
    return out[0], out[1], a, b, hook, params_a, params_b


_STATE = ("susceptibility", "is_infected", "infection_time")
_SYMPTOMS = ("current_stage", "next_stage", "time_to_next_stage")


def test_runner_against_the_torch_op_emulation(device, tmp_path):
    """Every result series of the run without the key and the final per-agent state, bit for bit; the new series against
    the emulation's own counts.  The emulation ALONE shows at least 20 reinfections and a step in which one agent is
    reinfected while another wanes, so the comparison is not an empty one."""
    import pandas as pd

    (res_a, inf_a), (res_b, inf_b), a, b, hook, _, _ = _run_pair(device, IMMUNITY, grad=False, groups=["area"])
    T, n = len(res_b["dates"]), a.n_agents
    print("reinfections", sum(hook.reinfections), "steps with both", hook.both, "waning", sum(hook.waning))
    assert sum(hook.reinfections) >= 20 and hook.both >= 1 and len(hook.reinfections) == T == DAYS + 1
    assert res_a["dates"] == res_b["dates"] and len(res_b) >= 6
    for k, v in res_b.items():
        if k != "dates":
            assert torch.equal(res_a[k], v), k
    assert torch.equal(inf_a, inf_b)
    ag_a, ag_b = a.data["agent"], b.data["agent"]
    for k in _STATE:
        assert torch.equal(ag_a[k], ag_b[k]), k
    for k in _SYMPTOMS:
        assert torch.equal(ag_a["symptoms"][k], ag_b["symptoms"][k]), k
    # the new series
    national = res_a["reinfections_per_timestep"]
    assert national.dtype == torch.float64 and national.tolist() == hook.reinfections and national[0] == 0
    assert national.sum() > 0 and not national.requires_grad
    assert res_a["reinfections_by_area"].shape == (T, len(a.group_keys["area"]))
    assert torch.equal(res_a["reinfections_by_area"].sum(1), national)
    assert (res_a["reinfections_by_area"].sum(0) > 0).sum() >= 2
    assert a._immunity_series[:T, 1].tolist() == hook.susc_sums
    susc = res_a["susceptibility_per_timestep"]
    assert susc.dtype == torch.float32 and torch.equal(
        susc.cpu(), (torch.tensor(hook.susc_sums, dtype=torch.float64) / float(1 << 30)).to(torch.float32))
    assert (torch.diff(susc) > 0).any() and (torch.diff(susc) < 0).any()      # it falls, and comes back
    # is_infected stays a flag; cases count agents, not infections
    assert float(ag_a["is_infected"].max()) == 1.0 and float(inf_a.max()) == 1.0
    assert float(res_a["cases_per_timestep"].max()) <= n
    plain, _ = _fresh_runner(device)()
    assert not torch.equal(plain["cases_per_timestep"], res_a["cases_per_timestep"]) and "reinfections_per_timestep" not in plain
    a.save_path = tmp_path / "out"
    a.save_results(res_a, inf_a)
    df = pd.read_csv(tmp_path / "out" / "results.csv")
    assert df["reinfections_per_timestep"].tolist() == national.tolist()
    assert np.array_equal(df["susceptibility_per_timestep"].to_numpy(dtype=np.float32), susc.cpu().numpy())
    by_area = pd.read_csv(tmp_path / "out" / "results_by_area.csv")
    assert by_area["reinfections"].tolist() == res_a["reinfections_by_area"].reshape(-1).tolist()


def _loss(results):
    return results["cases_per_timestep"].sum() + results["deaths_per_timestep"].sum()


#: measured on MI355X (printed with -s): the largest relative difference between the kernel's gradients and autograd's
#: through the float64 torch ops on this world; the tolerance is four times that, to cover other seeds
MEASURED_GRADIENT_AGREEMENT = 8.1e-8
GRADIENT_TOLERANCE = 4 * MEASURED_GRADIENT_AGREEMENT


def test_gradients_against_autograd_through_the_emulation(device):
    """half_life and residual_protection as nn.Parameters by band beside the log_beta parameters, the loss on cases plus
    deaths: their .grad against autograd through the emulation's float64 torch ops, d loss / d log_beta bit for bit, both
    new gradients non-zero in the bands that wane, and exactly 0 in the band in which nobody does (half_life = inf).  The
    kernel's terms are float32 products summed in float64: the tolerance is the measured agreement on this world times 4.
    Measured on MI355X: the largest relative difference over the four non-zero gradients was 8.1e-8 (printed with -s), so
    the test holds them to 3.24e-7."""
    (res_a, _), (res_b, _), a, b, hook, lb_a, lb_b = _run_pair(device, IMMUNITY_3, grad=True, days=GRAD_DAYS)
    assert res_a["cases_per_timestep"].requires_grad and sum(hook.reinfections) > 0 and sum(hook.waning) > 0
    for k in ("cases_per_timestep", "deaths_per_timestep"):
        assert torch.equal(res_a[k].detach(), res_b[k].detach()), k
    assert res_a["reinfections_per_timestep"].tolist() == hook.reinfections
    _loss(res_a).backward()
    _loss(res_b).backward()
    im = a.model.immunity
    worst = 0.0
    pairs = ((im.half_life.grad, hook.half_life.grad), (im.residual_protection.grad, hook.residual.grad))
    for got, ref in pairs:
        got, ref = got.double().cpu().tolist(), ref.cpu().tolist()
        assert len(got) == len(ref) == 3 and got[2] == 0.0 and ref[2] == 0.0, (got, ref)
        for g, r in zip(got[:2], ref[:2]):
            assert g != 0.0 and r != 0.0, (got, ref)
            worst = max(worst, abs(g - r) / abs(r))
    print("immunity gradients: largest relative difference", worst, [[t.tolist() for t in p] for p in pairs])
    assert worst <= GRADIENT_TOLERANCE, worst
    for pa, pb in zip(lb_a, lb_b):      # (a network no infection reached in this run has gradient 0, in both)
        assert pa.grad is not None and torch.equal(pa.grad, pb.grad), (pa.grad, pb.grad)
    assert sum(1 for pa in lb_a if pa.grad != 0) >= 2


def test_nothing_changes_without_it(device, monkeypatch):
    """Without the key no gj_immunity* symbol is called, in a plain and in a differentiable run; with half_life: .inf a
    run equals the run without the key bit for bit - every result series, the final state and log_beta.grad."""
    lib = N.load()
    calls = []

    def spy(name):
        real = getattr(lib, name)

        def wrapped(*args):
            calls.append(name)
            return real(*args)

        return wrapped

    for name in ("gj_immunity_step", "gj_adjoint_immunity"):
        monkeypatch.setattr(lib, name, spy(name))
    days = 12

    def run(immunity, grad):
        from grad_june_amd import infection

        runner = _fresh_runner(device, immunity=immunity, days=days)
        lb = _log_beta_parameters(runner) if grad else None
        torch.manual_seed(21)
        infection._philox_step = itertools.count(1 << 40)
        with torch.set_grad_enabled(grad):
            res, inf = runner()
        if grad:
            _loss(res).backward()
        return res, inf, runner, lb

    for grad in (False, True):
        ref, ref_inf, plain, lb_ref = run(None, grad)
        assert calls == [] and plain.model.immunity is None
        assert not any(k.startswith(("reinfections", "susceptibility")) for k in ref)
        res, inf, never, lb = run({"half_life": math.inf, "residual_protection": 0.3}, grad)
        assert "gj_immunity_step" in calls and ("gj_adjoint_immunity" in calls) == grad
        for k, v in ref.items():
            if k != "dates":
                assert torch.equal(res[k].detach(), v.detach()), k
        assert torch.equal(inf, ref_inf) and not res["reinfections_per_timestep"].any()
        for k in _STATE:
            assert torch.equal(never.data["agent"][k].detach(), plain.data["agent"][k].detach()), k
        for k in _SYMPTOMS:
            assert torch.equal(never.data["agent"]["symptoms"][k].detach(), plain.data["agent"]["symptoms"][k].detach()), k
        if grad:
            assert lb_ref[0].grad is not None and lb_ref[0].grad != 0
            for pa, pb in zip(lb, lb_ref):
                assert torch.equal(pa.grad, pb.grad), (pa.grad, pb.grad)
        calls.clear()


# ---- two ranks ----------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, R_, port, out):
    import os

    import torch.distributed as dist

    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.distributed_api import DistributedRunner

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=R_)
    try:
        params = lambda: _params("cuda:0", immunity=IMMUNITY, groups=["area"], days=DAYS)

        def run(runner):
            im = runner.model.immunity
            im.half_life = torch.nn.Parameter(im.half_life.detach().clone())
            im.residual_protection = torch.nn.Parameter(im.residual_protection.detach().clone())
            results, _ = runner()
            c = results["cases_per_timestep"]
            loss = (c * torch.linspace(0.5, 1.5, c.numel(), device=c.device)).sum() + results["deaths_per_timestep"].sum()
            loss.backward()
            return results, [im.half_life.grad.tolist(), im.residual_protection.grad.tolist()]

        torch.manual_seed(33)
        res, grads = run(DistributedRunner.from_parameters(params()))
        gathered = [None] * R_
        dist.all_gather_object(gathered, grads)
        assert gathered[0] == gathered[1], "every rank holds the whole gradient"
        if rank == 0:
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)
            ref_res, ref = run(G.Runner.from_parameters(params()))
            for k in ("cases_per_timestep", "deaths_per_timestep", "cases_by_area", "reinfections_per_timestep",
                      "reinfections_by_area", "susceptibility_per_timestep"):
                assert torch.equal(res[k].detach().cpu(), ref_res[k].detach().cpu()), k
            assert ref_res["reinfections_per_timestep"].sum() > 0
            for a, b in zip(sum(grads, []), sum(ref, [])):
                assert b != 0.0 and a == pytest.approx(b, rel=2e-5, abs=1e-7), (grads, ref)
            out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_gpu_series_and_immunity_gradients(device):
    import os

    import torch.multiprocessing as mp

    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_two_rank_worker, args=(2, 29800 + os.getpid() % 90, out), nprocs=2, join=True)
    assert out[0] == 1
