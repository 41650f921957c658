"""Differentiable hot-path step (row f3 of SURVEY section 8): gradients w.r.t. every network's
``log_beta`` and w.r.t. the incoming state, so that a loss on the infection counts can be
back-propagated through the timesteps like with the reference (example_scripts/run_model.py:9-11).

The forward of a step is the ordinary fused HIP step on fresh output tensors.  There is ONE step node, ``HotPathStep``,
for a single GPU and for a rank of a partitioned world: it is written against the few things a backward needs from "the
place the passes run" - ``engine``, ``run_step``, ``sparse_passes(bufs, io, p, between)``, ``venue_weights``,
``all_reduce_max``, ``all_reduce_sum`` - which ``distributed.DistributedHotPath`` provides for a rank (halo all-to-all
and partial-sum all-reduce inside the passes, real reductions) and ``_LocalPasses`` for one GPU (two launches, identity
reductions).  The backward is hand-written (``oracle/gj_oracle.py:adjoint_step`` is its dense CPU restatement, checked
against the reference's autograd):

* the two sparse passes are self-adjoint up to exchanging the per-network masks, so the gradient
  w.r.t. the transmissions is the SAME four tiled phases run with ``transpose = 1`` on the vector
  ``susceptibility * ts_bar``;
* d loss / d log_beta_n = ln(10) * sum_v cum_n[v] * cum'_n[v] / (beta_n * p_contact[v]) - a dot
  product of the forward and transposed per-venue sums;
* the rest (straight-through Gumbel-softmax, clamp/exp/clamp, infect_people, transmission profile)
  is elementwise: ``gj_adjoint_sample`` and ``gj_adjoint_transmission``.

What a step keeps for its backward (``KEEP_FORWARD_SUMS``): the pre-state (3 per-agent floats) and - by default -
the two products of the forward's sparse passes that the adjoint needs, the per-agent sums before the susceptibility
factor (``gj_step_io.agent_sums``, one float per agent) and the per-venue sums ``cum`` (a clone, a few MB): 4 floats
per agent and step, 160 MB per step of a 10 M-agent world out of 288 GB.  With ``GJ_BACKWARD_RECOMPUTE=1`` (or
``autograd.KEEP_FORWARD_SUMS = False``) a step keeps the pre-state only and its backward recomputes the two passes
first (round 2's form: 3 floats per agent and step; C3 at 10 M agents: a backward of 1.42 ms = 2.5x the forward instead
of 0.91 ms = 1.6x, profiles/r04_c3_10m_backward*.json).  Both give the same gradients bit for bit - the kept sums ARE
what the recomputation produces (tests/test_gradients.py::test_kept_forward_sums_equal_the_recomputation).
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

import os

from . import _native as N
from .engine import AgentBuffers
from .plan import SPLIT_SUFFIX
from .transmission import PROFILE

KEEP_FORWARD_SUMS = os.environ.get("GJ_BACKWARD_RECOMPUTE", "0") in ("", "0")


def _keep_sums(env) -> bool:
    return bool(env.get("keep_sums", KEEP_FORWARD_SUMS))


def _f32(g, device=None):
    """A tensor as the kernels read it - detached, contiguous float32, on ``device`` if given; None stays None."""
    return None if g is None else g.detach().to(device=device, dtype=torch.float32).contiguous()


def _to_devices(grads, devices):
    """Gradients handed back to the devices of their inputs; None (no gradient asked for) stays None."""
    return [None if g is None else g.to(d) for g, d in zip(grads, devices)]


def _ones(plan, n):
    """A constant vector of ones on the plan's device (the adjoint runs the passes with susceptibility = 1; the phases
    it calls only read it) - one per plan, not a fill launch per backward step."""
    t = getattr(plan, "_adjoint_ones", None)
    if t is None or t.numel() != n:
        t = torch.ones(n, dtype=torch.float32, device=plan.device)
        plan._adjoint_ones = t
    return t


def _clone_forward_cum(plan, nets):
    """{edge set: clone of its per-venue sums} for every set a network of ``nets`` (or its twin on a split set) runs on."""
    cum_fwd = {}
    for _, names in _names_with_twins(plan, nets):
        for name in names:
            es = plan.networks[name].edge_set
            if es not in cum_fwd:
                cum_fwd[es] = plan.cum_of(es).clone()
    return cum_fwd


class _LocalPasses:
    """One GPU seen as ``distributed.DistributedHotPath`` is seen by a differentiable step: the place the passes run.
    No peers, so the sparse passes have nothing to exchange and the two small reductions return their argument."""

    halo = None                                                    # (as on a rank without peers: nothing to reduce over)

    def __init__(self, engine):
        self.engine = engine

    def transmission_buffers(self):
        return {"transmission": _new_transmission(self.engine.plan)}

    def run_step(self, bufs, io, params_of):
        self.engine.step(bufs, params_of(None), io)

    def sparse_passes(self, bufs, io, p, between=None):
        self.engine.step_phase(bufs, p, io, 8)                     # phase A, then B + C in one launch (cum stays in place)
        if between is not None:
            between()
        self.engine.step_phase(bufs, p, io, 4)

    def venue_weights(self, set_name):
        return None

    def all_reduce_max(self, x):
        return x

    all_reduce_sum = all_reduce_max


def _passes_of(where):
    """``where``: a ``DistributedHotPath``, a ``_LocalPasses``, or a bare engine (wrapped)."""
    return where if hasattr(where, "sparse_passes") else _LocalPasses(where)


def _step_env(env):
    """(where the passes run, params_of, the step's transmission buffers as a callable) of a step's ``env``: one GPU
    gives ``engine`` and ``params``, a rank of a partitioned world ``hp`` (its ``DistributedHotPath``, which steps on its
    own extended transmission arrays) and ``params_of``."""
    if "hp" in env:
        hp = env["hp"]
        return hp, env["params_of"], lambda: {k: hp.state[k] for k in ("transmission", "q_transmission")}
    local = _LocalPasses(env["engine"])
    return local, lambda sets: env["params"], local.transmission_buffers


def _new_transmission(plan):
    """A transmission array for one call: uninitialised where the passes write all of it, zeros where it has halo or
    pad slots."""
    n, n_ext = plan.host.n_agents, plan.host.n_ext_agents
    return (torch.empty if n_ext == n else torch.zeros)(n_ext, dtype=torch.float32, device=plan.device)


def _require_tiled(plan):
    if plan.c.tiled is None or not bool(plan.c.tiled):
        raise NotImplementedError("the backward pass runs on the tiled layout")


def _forward_sums(where, p, bufs, acc, nets, compute_transmission: bool):
    """Forward of the two sparse passes with susceptibility = 1 in ``bufs``: fills ``acc`` with
    sum_n w_n * (L_n (m_n trans)) and returns {edge set: clone of its per-venue sums}."""
    passes = _passes_of(where)
    engine = passes.engine
    io = engine.io(trans_susc=acc)
    p.transpose = 0
    if compute_transmission:
        engine.step_phase(bufs, p, io, 0)                      # transmission (+ q * transmission)
    else:
        engine.quarantine_transmission(bufs, p)                # the caller supplied the transmissions
    cum_fwd = {}
    passes.sparse_passes(bufs, io, p, between=lambda: cum_fwd.update(_clone_forward_cum(engine.plan, nets)))
    return cum_fwd


def _transposed_passes(where, p, bufs, scratch, x, nets, betas, cum_fwd):
    """The transposed pipeline on x = susceptibility * ts_bar: returns (d loss / d transmission,
    [d loss / d log_beta per network of ``nets``]).  ``scratch`` is the transmission buffer of ``bufs``.  On a rank the
    passes communicate as the forward's do (the cotangents of halo agents travel by the same all-to-all as their
    transmissions, the transposed per-venue sums by the same all-reduce) and the beta gradients are summed over the
    ranks at the end: every rank returns the whole world's."""
    passes = _passes_of(where)
    engine = passes.engine
    plan = engine.plan
    n = plan.host.n_agents
    # The tiled passes sum in fixed point (2^-36 / 2^-32 resolution, |value| <= 16384 / 262144): scales chosen for the
    # forward's transmissions.  A cotangent has whatever magnitude the user's loss gives it (an MSE on case counts:
    # 1e5; a normalised loss: 1e-10), so x is brought to max |x| in [0.5, 1) by a power of two first - one scale for
    # the whole world - and the results are scaled back - exact, the passes being linear - without a host
    # synchronisation.
    lo, hi = torch.aminmax(x)                                  # (one reduction launch; max |x| = max(-lo, hi))
    scale = _power_of_two_scale(passes.all_reduce_max(torch.maximum(-lo, hi)))
    if scratch.numel() != n:
        scratch[n:].zero_()                                    # halo and pad slots (a recomputation filled the halo's)
    torch.div(x, scale, out=scratch[:n])
    tbar = torch.empty(n, dtype=torch.float32, device=plan.device)
    reduce = passes.halo is not None                           # peers: the ranks' fp64 dot products are summed first
    grads: List[torch.Tensor] = []

    def beta_gradients():                                      # cum' is complete
        gs = _beta_gradients(plan, nets, betas, cum_fwd, scale, weights_of=passes.venue_weights)
        grads.extend(gs if reduce else [g.to(torch.float32) for g in gs])

    p.transpose = 1
    try:
        engine.quarantine_transmission(bufs, p)                # q * x for the masked sets
        passes.sparse_passes(bufs, engine.io(trans_susc=tbar), p, between=beta_gradients)   # tbar: of x / scale
    finally:
        p.transpose = 0
    if reduce and grads:
        total = passes.all_reduce_sum(torch.stack(grads))
        grads = [total[i].to(torch.float32) for i in range(len(grads))]
    return tbar.mul_(scale), grads


def _names_with_twins(plan, nets):
    """(network, [its name and - on a set the multi-GPU partition split - its twin's]) for every network."""
    return [(net, [nm for nm in (net.name, net.name + SPLIT_SUFFIX) if nm in plan.networks]) for net in nets]


def _beta_gradients(plan, nets, betas, cum_fwd, scale, weights_of=None) -> List[torch.Tensor]:
    """ln(10) * sum_v cum_n[v] * cum'_n[v] / (beta_n * p_contact[v]) per network, from the forward's and the
    transposed pass's per-venue sums (``plan.cum_of`` holds the latter).  ``weights_of(edge set)``: this rank's
    weight of every venue (multi-GPU: the ranks' values are summed by the caller).  One launch per edge set + one to
    finish (gj_adjoint_beta_*: fp64, summed in a fixed order) - as torch ops this was ~10 small launches per network
    and what a backward step spent most of its host time on."""
    lib, dev = N.load(), plan.device
    partial = torch.zeros(N.GJ_ADJ_BETA_BLOCKS * N.GJ_MAX_NETS, dtype=torch.float64, device=dev)
    out = torch.zeros(max(1, len(nets)), dtype=torch.float64, device=dev)
    per_set, per_set_k = {}, {}
    for col, (net, names) in enumerate(_names_with_twins(plan, nets)):
        for name in names:
            es = plan.networks[name].edge_set
            k = per_set_k.get(es, 0)
            per_set_k[es] = k + 1
            per_set.setdefault(es, []).append((k, col, float(betas[net.name])))
    scale32 = scale.to(device=dev, dtype=torch.float32).reshape(1)
    keep = []
    for es, items in per_set.items():
        i = plan.host.set_index[es]
        nk = len(items)
        assert [k for k, _, _ in items] == list(range(nk))
        beta = (C.c_float * nk)(*[b for _, _, b in items])
        cols = (C.c_int32 * nk)(*[c for _, c, _ in items])
        w = weights_of(es) if weights_of is not None else None
        if w is not None:
            w = w.to(device=dev, dtype=torch.float64).contiguous()
        fwd, bwd = cum_fwd[es].contiguous(), plan.cum_of(es)
        keep.append((w, fwd))
        N.check(lib.gj_adjoint_beta_partial(plan.host.sets[i].n_venues, int(plan.c.sets[i].cum_stride), nk, N.ptr(fwd),
                                            N.ptr(bwd), N.ptr(plan.keep[i]["v_pc"]), N.ptr(w), beta, cols, N.ptr(partial),
                                            N.current_stream()), "gj_adjoint_beta_partial")
    N.check(lib.gj_adjoint_beta_finish(len(nets), N.ptr(partial), N.ptr(scale32), N.ptr(out), N.current_stream()),
            "gj_adjoint_beta_finish")
    return [out[i] for i in range(len(nets))]


def _power_of_two_scale(peak: torch.Tensor) -> torch.Tensor:
    scale = torch.where((peak > 0) & torch.isfinite(peak), torch.exp2(torch.ceil(torch.log2(peak.clamp_min(1e-45)))),
                        torch.ones_like(peak))
    return torch.where(torch.isfinite(scale) & (scale > 0), scale, torch.ones_like(scale))


def _param_grads(nets, grads):
    out = []
    for net, g in zip(nets, grads):
        lb = net.log_beta
        out.append(g.to(lb.device).reshape(lb.shape) if isinstance(lb, torch.Tensor) and lb.requires_grad else None)
    return out


def _adjoint_profile(n, st0, now, tbar, g_inf, grad_inf, grad_time, want, dev):
    """Through the transmission profile: grad_inf = g_inf + tbar * dT/d is_infected, grad_time += tbar * dT/dt, and -
    for each of the four profile parameters ``want`` flags - tbar * dT/d parameter (None for the others).  With no flag
    set this is the launch the step has always made (gj_adjoint_transmission); otherwise gj_adjoint_transmission_params,
    whose grad_inf / grad_time are the same bit for bit and which writes only the requested parameter gradients."""
    lib = N.load()
    if not any(want):
        N.check(lib.gj_adjoint_transmission(n, C.byref(st0.c), float(now), N.ptr(tbar), N.ptr(g_inf), N.ptr(grad_inf),
                                            N.ptr(grad_time), N.current_stream()), "gj_adjoint_transmission")
        return [None] * len(PROFILE)
    outs = [torch.empty(n, dtype=torch.float32, device=dev) if w else None for w in want]
    N.check(lib.gj_adjoint_transmission_params(n, C.byref(st0.c), float(now), N.ptr(tbar), N.ptr(g_inf),
                                               N.ptr(grad_inf), N.ptr(grad_time), *[N.ptr(o) for o in outs],
                                               N.current_stream()), "gj_adjoint_transmission_params")
    return outs


def _profile_wanted(ctx, n_nets):
    """Which of the four profile tensors (the inputs after the log_betas, when the caller passed them) need a gradient."""
    flags = tuple(ctx.needs_input_grad[4 + n_nets:])
    return flags if flags else (False,) * len(PROFILE)


def _profile_grads(ctx, n_nets, grads):
    """The profile gradients in the order of the node's inputs (nothing when the caller passed no profile tensors)."""
    if len(ctx.needs_input_grad) <= 4 + n_nets:
        return []
    return _to_devices(grads, ctx.profile_devices)


class HotPathStep(torch.autograd.Function):
    """(susceptibility, is_infected, infection_time, *log_betas[, max_infectiousness, shape, rate, shift]) ->
    (susceptibility', is_infected', infection_time', new_infected).  The four profile tensors are optional inputs
    (the step reads ``env["fixed"]``, their detached values): passed, they receive d loss / d parameter per agent.

    ``env``: ``fixed``, ``stage``, ``exp_noise``, ``nets``, ``betas``, optionally ``keep_sums``, and where the step runs
    (``_step_env``): ``engine`` and ``params`` on one GPU, or ``hp`` and ``params_of`` on one rank of a multi-GPU job
    (``distributed.DistributedHotPath``).  There the inputs and outputs are the rank's OWNED agents, the forward is the
    multi-rank launch sequence and the backward runs the transposed passes with the forward's communication pattern
    and ends with one all-reduce of the step's d loss / d log_beta - so every rank's ``log_beta.grad`` is the whole
    world's gradient, equal to the single-GPU run's.  Every rank must back-propagate the same graph (a loss built from
    the rank-summed result series: ``distributed_api.DistributedRunner``)."""

    @staticmethod
    def forward(ctx, env, susc, inf, time, *log_betas_and_profile):
        passes, params_of, transmission_buffers = _step_env(env)
        fixed, stage, exp_noise, nets = (env[k] for k in ("fixed", "stage", "exp_noise", "nets"))
        ctx.profile_devices = [t.device for t in log_betas_and_profile[len(nets):]]
        engine = passes.engine
        plan = engine.plan
        n = plan.host.n_agents
        out_s, out_i, out_t = (t.detach().to(torch.float32).clone().contiguous() for t in (susc, inf, time))
        new_inf = torch.empty(n, dtype=torch.float32, device=plan.device)
        bufs = AgentBuffers(plan, **fixed, infection_time=out_t, is_infected=out_i, susceptibility=out_s,
                            current_stage=stage, **transmission_buffers())
        keep = _keep_sums(env) and plan.c.tiled is not None and bool(plan.c.tiled)
        acc = torch.empty(n, dtype=torch.float32, device=plan.device) if keep else None
        passes.run_step(bufs, engine.io(new_infected=new_inf, exp_noise=exp_noise, agent_sums=acc), params_of)
        ctx.env = env
        ctx.save_for_backward(susc.detach().to(torch.float32).contiguous(), inf.detach().to(torch.float32).contiguous(),
                              time.detach().to(torch.float32).contiguous())
        ctx.transmission = bufs.tensors["transmission"]
        if env.get("keep_transmission") is not None:      # the infector series reads the step's transmissions after it
            env["keep_transmission"]["transmission"] = ctx.transmission
        ctx.kept = (acc, _clone_forward_cum(plan, nets)) if keep else None      # (cum: complete after the all-reduce)
        return out_s, out_i, out_t, new_inf

    @staticmethod
    def backward(ctx, g_susc, g_inf, g_time, g_new):
        env = ctx.env
        passes, params_of, _ = _step_env(env)
        fixed, stage, exp_noise, nets = (env[k] for k in ("fixed", "stage", "exp_noise", "nets"))
        susc0, inf0, time0 = ctx.saved_tensors
        plan, lib, dev = passes.engine.plan, N.load(), passes.engine.plan.device
        n = plan.host.n_agents
        _require_tiled(plan)
        p = params_of(None)
        g_susc, g_inf, g_time, g_new = _f32(g_susc), _f32(g_inf), _f32(g_time), _f32(g_new)
        ones = _ones(plan, n)
        scratch = _new_transmission(plan)
        bufs = AgentBuffers(plan, **fixed, infection_time=time0, is_infected=inf0, susceptibility=ones,
                            transmission=scratch, current_stage=stage)
        if ctx.kept is not None:      # the forward's per-agent and per-venue sums, kept by the step
            acc, cum_fwd = ctx.kept
        else:                         # recompute the forward of the two passes from the saved pre-state
            acc = torch.empty(n, dtype=torch.float32, device=dev)
            cum_fwd = _forward_sums(passes, p, bufs, acc, nets, compute_transmission=True)
        # ---- elementwise adjoint of epilogue + sampler + infect_people ------------------------------------
        x = torch.empty(n, dtype=torch.float32, device=dev)
        grad_susc = torch.empty(n, dtype=torch.float32, device=dev)
        grad_time = torch.empty(n, dtype=torch.float32, device=dev)
        N.check(lib.gj_adjoint_sample(n, N.ptr(susc0), N.ptr(time0), N.ptr(acc), N.ptr(exp_noise), int(p.seed),
                                      int(p.step), int(p.agent_offset), float(p.now), float(p.delta_time),
                                      N.ptr(g_susc), N.ptr(g_inf), N.ptr(g_time), N.ptr(g_new), N.ptr(x),
                                      N.ptr(grad_susc), N.ptr(grad_time), N.current_stream()), "gj_adjoint_sample")
        # ---- transposed passes on x = susc0 * ts_bar --------------------------------------------------------
        tbar, grads = _transposed_passes(passes, p, bufs, scratch, x, nets, env["betas"], cum_fwd)
        # ---- through the transmission profile ------------------------------------------------------------------
        # (tbar is complete for a rank's owned agents after the transposed passes: no collective here)
        grad_inf = torch.empty(n, dtype=torch.float32, device=dev)
        st0 = AgentBuffers(plan, **fixed, infection_time=time0, is_infected=inf0, susceptibility=ones,
                           transmission=scratch)
        pg = _adjoint_profile(n, st0, p.now, tbar, g_inf, grad_inf, grad_time, _profile_wanted(ctx, len(nets)), dev)
        return (None, grad_susc, grad_inf, grad_time, *_param_grads(nets, grads), *_profile_grads(ctx, len(nets), pg))


class TransmissionProfile(torch.autograd.Function):
    """The stand-alone ``TransmissionUpdater.forward`` (transmission.py:39-51) as an autograd node:
    (max_infectiousness, shape, rate, shift, infection_time, is_infected) -> transmission, differentiable w.r.t. all
    six like the reference's plain torch ops.  Forward = ``gj_transmission_update``; backward = one
    ``gj_adjoint_transmission_params`` launch that writes only the gradients autograd asks for."""

    @staticmethod
    def forward(ctx, env, mx, shape, rate, shift, time, inf):
        engine, p = env["engine"], env["params"]
        plan = engine.plan
        n, dev = plan.host.n_agents, plan.device
        vals = [_f32(t, dev) for t in (mx, shape, rate, shift, time, inf)]
        out = torch.empty(n, dtype=torch.float32, device=dev)
        bufs = AgentBuffers(plan, **dict(zip(PROFILE, vals[:4])), infection_time=vals[4], is_infected=vals[5],
                            susceptibility=_ones(plan, n), transmission=out)
        engine.transmission_update(bufs, p)
        ctx.engine, ctx.now = engine, float(p.now)
        ctx.devices = [t.device for t in (mx, shape, rate, shift, time, inf)]
        ctx.save_for_backward(*vals)
        return out

    @staticmethod
    def backward(ctx, g):
        plan = ctx.engine.plan
        n, dev = plan.host.n_agents, plan.device
        vals = ctx.saved_tensors
        tbar = _f32(g, dev)
        st0 = AgentBuffers(plan, **dict(zip(PROFILE, vals[:4])), infection_time=vals[4], is_infected=vals[5],
                           susceptibility=_ones(plan, n), transmission=tbar)
        grad_inf = torch.empty(n, dtype=torch.float32, device=dev)
        grad_time = torch.zeros(n, dtype=torch.float32, device=dev)
        want = ctx.needs_input_grad[1:5]
        outs = [torch.empty(n, dtype=torch.float32, device=dev) if w else None for w in want]
        N.check(N.load().gj_adjoint_transmission_params(n, C.byref(st0.c), ctx.now, N.ptr(tbar), None, N.ptr(grad_inf),
                                                        N.ptr(grad_time), *[N.ptr(o) for o in outs],
                                                        N.current_stream()), "gj_adjoint_transmission_params")
        grads = outs + [grad_time if ctx.needs_input_grad[5] else None, grad_inf if ctx.needs_input_grad[6] else None]
        return (None, *_to_devices(grads, ctx.devices))


class AllReduceSum(torch.autograd.Function):
    """Sum of a tensor over the ranks whose gradient is the identity: every rank evaluates the SAME loss on the
    summed value, so d loss / d (this rank's term) = d loss / d sum, which every rank already holds."""

    @staticmethod
    def forward(ctx, hp, x):
        return hp.all_reduce_sum(x.detach())

    @staticmethod
    def backward(ctx, g):
        return None, g


class NetworksForward(torch.autograd.Function):
    """The stand-alone ``InfectionNetworks.forward`` / ``InfectionNetwork.forward`` (base.py:61-84,118-141) as
    an autograd node: (transmission, susceptibility, *log_betas) -> not_infected_probs (or one network's
    trans_susc), differentiable w.r.t. all of them.  Same machinery as HotPathStep without the sampler."""

    @staticmethod
    def forward(ctx, env, transmission, susceptibility, *log_betas):
        engine, p, want = env["engine"], env["params"], env["want"]
        plan = engine.plan
        n = plan.host.n_agents
        dev = plan.device
        trans = torch.zeros(plan.host.n_ext_agents, dtype=torch.float32, device=dev)
        trans[:n].copy_(transmission.detach())
        susc = _f32(susceptibility, dev)
        bufs = AgentBuffers(plan, susceptibility=susc, transmission=trans, current_stage=env["stage"])
        out = torch.empty(n, dtype=torch.float32, device=dev)
        keep = _keep_sums(env) and plan.c.tiled is not None and bool(plan.c.tiled)
        acc = torch.empty(n, dtype=torch.float32, device=dev) if keep else None
        engine.quarantine_transmission(bufs, p)
        engine.venue_reduce(bufs, p)
        engine.agent_gather(bufs, p, engine.io(not_infected_probs=out, agent_sums=acc) if want == "probs"
                            else engine.io(trans_susc=out, agent_sums=acc), sample=False)
        snap = N.StepParams()
        C.memmove(C.byref(snap), C.byref(p), C.sizeof(N.StepParams))
        ctx.env = dict(env, params=snap)
        ctx.save_for_backward(trans, susc)
        ctx.kept = (acc, _clone_forward_cum(plan, env["nets"])) if keep else None
        return out

    @staticmethod
    def backward(ctx, g_out):
        env = ctx.env
        engine, p, nets, want = env["engine"], env["params"], env["nets"], env["want"]
        trans, susc = ctx.saved_tensors
        plan, dev = engine.plan, engine.plan.device
        n = plan.host.n_agents
        _require_tiled(plan)
        g = _f32(g_out)
        ones = _ones(plan, n)
        scratch = trans.clone()
        bufs = AgentBuffers(plan, susceptibility=ones, transmission=scratch, current_stage=env["stage"])
        if ctx.kept is not None:
            acc, cum_fwd = ctx.kept
        else:
            acc = torch.empty(n, dtype=torch.float32, device=dev)
            cum_fwd = _forward_sums(engine, p, bufs, acc, nets, compute_transmission=False)
        if want == "probs":                                       # clamp(exp(-clamp(ts, 1e-6, 100) * dt), 0, 1)
            ts = susc * acc
            inside = (ts >= 1e-6) & (ts <= 100.0)
            prob = torch.exp(-torch.clamp(ts, 1e-6, 100.0) * float(p.delta_time))
            ts_bar = torch.where(inside, g * (-float(p.delta_time)) * prob, torch.zeros_like(g))
        else:
            ts_bar = g
        grad_susc = ts_bar * acc
        tbar, grads = _transposed_passes(engine, p, bufs, scratch, (susc * ts_bar).contiguous(), nets, env["betas"],
                                         cum_fwd)
        return (None, tbar, grad_susc, *_param_grads(nets, grads))


class SeedByGroup(torch.autograd.Function):
    """The seed as an autograd node (``infection.infect_fraction_by_group``): (fractions [G], susceptibility,
    is_infected, infection_time) -> (new_infected, susceptibility', is_infected', infection_time').  Forward =
    ``gj_sample_infect`` on ``p_not[labels]`` and fresh state tensors; backward = ``gj_adjoint_seed``, which sums the
    per-agent terms of d loss / d fraction per group in fp64 in a fixed order.  ``env``: labels (None: one group), the
    labelling's ``groups.SeedPlan``, ``p_not`` (float32 [G], 1 - fraction), the noise or the (seed, step, agent_offset)
    of the Philox draws, ``now``, and - on a rank of a partitioned world - ``all_reduce``, the sum over the ranks that
    makes every rank's gradient the whole world's (as ``HotPathStep`` does for log_beta)."""

    @staticmethod
    def forward(ctx, env, fractions, susc, inf, time):
        from .infection import _launch_sample

        labels, p_not = env["labels"], env["p_not"]
        dev = p_not.device
        pre = [_f32(t, dev) for t in (susc, inf, time)]
        n = pre[0].numel()
        out_s, out_i, out_t = (t.clone() for t in pre)
        probs = p_not.expand(n).contiguous() if labels is None else p_not[labels.long()]
        new_inf = torch.empty(n, dtype=torch.float32, device=dev)
        _launch_sample(probs, env["exp_noise"], new_inf, now=env["now"], state=(out_s, out_i, out_t), seed=env["seed"],
                       step=env["step"], agent_offset=env["agent_offset"])
        ctx.env = env
        ctx.like = (fractions.device, fractions.dtype, fractions.shape)
        ctx.devices = [t.device for t in (susc, inf, time)]
        ctx.save_for_backward(pre[0], pre[2])
        return new_inf, out_s, out_i, out_t

    @staticmethod
    def backward(ctx, g_new, g_susc, g_inf, g_time):
        env = ctx.env
        susc0, time0 = ctx.saved_tensors
        labels, plan, p_not = env["labels"], env["plan"], env["p_not"]
        dev, n, G = p_not.device, susc0.numel(), p_not.numel()
        g_new, g_susc, g_inf, g_time = (_f32(g, dev) for g in (g_new, g_susc, g_inf, g_time))
        want_s, want_i, want_t = ctx.needs_input_grad[2:5]
        n_chunks = plan.n_chunks if labels is not None else (n + N.GJ_SEED_CHUNK - 1) // N.GJ_SEED_CHUNK
        contrib = torch.empty(max(1, n), dtype=torch.float64, device=dev)
        partial = torch.empty(max(1, n_chunks), dtype=torch.float64, device=dev)
        grad = torch.empty(G, dtype=torch.float64, device=dev)
        grad_s = torch.empty(n, dtype=torch.float32, device=dev) if want_s else None
        grad_t = torch.empty(n, dtype=torch.float32, device=dev) if want_t else None
        N.check(N.load().gj_adjoint_seed(n, N.ptr(p_not), N.ptr(labels), G, C.byref(plan.c) if labels is not None else None,
                                         N.ptr(susc0), N.ptr(time0), N.ptr(env["exp_noise"]), int(env["seed"]),
                                         int(env["step"]), int(env["agent_offset"]), float(env["now"]), N.ptr(g_susc),
                                         N.ptr(g_inf), N.ptr(g_time), N.ptr(g_new), N.ptr(contrib), N.ptr(partial),
                                         N.ptr(grad), N.ptr(grad_s), N.ptr(grad_t), N.current_stream()),
                "gj_adjoint_seed")
        if env.get("all_reduce") is not None:
            grad = env["all_reduce"](grad)                     # fp64: the world's gradient on every rank
        like_dev, like_dtype, like_shape = ctx.like
        grad_i = None
        if want_i:
            grad_i = g_inf if g_inf is not None else torch.zeros(n, dtype=torch.float32, device=dev)
        return (None, grad.to(device=like_dev, dtype=like_dtype).reshape(like_shape),
                *_to_devices((grad_s, grad_i, grad_t), ctx.devices))


class VaccinationStep(torch.autograd.Function):
    """One launch of a vaccination campaign as an autograd node (``policies.VaccinationPolicies.apply``): (efficacy [B],
    susceptibility) -> susceptibility'.  Forward = ``gj_vaccinate`` on a fresh tensor; backward =
    ``gj_adjoint_vaccinate``, which sums d loss / d efficacy per band in fp64 in the order of the bands' ``SeedPlan``.
    ``env``: the launch's decision inputs (agent classes, per-age tables, seed, stream, agent_offset), the optional
    outputs ``newly`` / ``count``, ``band`` (int32 per agent) with its ``plan`` and - on a rank of a partitioned world -
    ``all_reduce``, the sum over the ranks that makes every rank's gradient the whole world's (as ``SeedByGroup``)."""

    @staticmethod
    def forward(ctx, env, efficacy, susc):
        dev = env["cls"].device
        susc0 = _f32(susc, dev)
        out = susc0.clone()
        N.check(N.load().gj_vaccinate(out.numel(), N.ptr(env["cls"]), env["tables"], env["seed"], env["stream"],
                                      env["agent_offset"], N.ptr(out), N.ptr(env["newly"]), N.ptr(env["count"]),
                                      N.current_stream()), "gj_vaccinate")
        ctx.env = {k: env[k] for k in ("cls", "tables", "seed", "stream", "agent_offset", "band", "plan", "all_reduce")}
        ctx.like = (efficacy.device, efficacy.dtype, efficacy.shape)
        ctx.susc_device = susc.device
        ctx.save_for_backward(susc0)
        return out

    @staticmethod
    def backward(ctx, g_out):
        env = ctx.env
        (susc0,) = ctx.saved_tensors
        plan, dev, n = env["plan"], susc0.device, susc0.numel()
        g_out = _f32(g_out, dev)
        contrib = torch.empty(max(1, n), dtype=torch.float64, device=dev)
        partial = torch.empty(max(1, plan.n_chunks), dtype=torch.float64, device=dev)
        grad = torch.empty(plan.n_groups, dtype=torch.float64, device=dev)
        g_in = torch.empty(n, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        N.check(N.load().gj_adjoint_vaccinate(n, N.ptr(env["cls"]), env["tables"], env["seed"], env["stream"],
                                              env["agent_offset"], N.ptr(susc0), N.ptr(g_out), N.ptr(env["band"]),
                                              plan.n_groups, C.byref(plan.c), N.ptr(contrib), N.ptr(partial),
                                              N.ptr(grad), N.ptr(g_in), N.current_stream()), "gj_adjoint_vaccinate")
        if env.get("all_reduce") is not None:
            grad = env["all_reduce"](grad)                     # fp64: the world's gradient on every rank
        like_dev, like_dtype, like_shape = ctx.like
        grad_eff = grad.to(device=like_dev, dtype=like_dtype).reshape(like_shape) if ctx.needs_input_grad[1] else None
        return None, grad_eff, (None if g_in is None else g_in.to(ctx.susc_device))


class ImmunityStep(torch.autograd.Function):
    """One launch of the waning-immunity rule as an autograd node (``immunity.Immunity.step``): (half_life [B],
    residual_protection [B], susceptibility, is_infected, new_infected) -> (susceptibility', is_infected').  Forward =
    ``gj_immunity_step`` on fresh tensors, keeping its ``flags`` and the incoming susceptibility (5 B per agent and step);
    backward = ``gj_adjoint_immunity``, which sums ``sum_A`` / ``sum_B`` per band in fp64 in the order of the bands'
    ``SeedPlan``; the host turns them into the two gradients in doubles.  ``env``: agent classes, per-age tables, the stage
    and the index of ``recovered``, ``dt``, the optional outputs ``reinfected`` / ``count`` / ``susc_sum``, ``band`` with
    its ``plan`` and - on a rank of a partitioned world - ``all_reduce`` (as ``VaccinationStep``)."""

    @staticmethod
    def forward(ctx, env, half_life, residual, susc, inf, new_infected):
        dev = env["cls"].device
        susc0, nw = _f32(susc, dev), _f32(new_infected, dev)
        out_s, out_i = susc0.clone(), _f32(inf, dev).clone()
        flags = torch.empty(out_s.numel(), dtype=torch.uint8, device=dev)
        N.check(N.load().gj_immunity_step(out_s.numel(), N.ptr(env["cls"]), env["tables"], N.ptr(env["stage"]),
                                          env["recovered"], N.ptr(nw), N.ptr(out_s), N.ptr(out_i), N.ptr(flags),
                                          N.ptr(env["reinfected"]), N.ptr(env["count"]), N.ptr(env["susc_sum"]),
                                          N.current_stream()), "gj_immunity_step")
        ctx.env = {k: env[k] for k in ("cls", "tables", "dt", "band", "plan", "all_reduce")}
        ctx.values = (half_life.detach().to(torch.float32).cpu().tolist(), residual.detach().to(torch.float32).cpu().tolist())
        ctx.like = [(t.device, t.dtype, t.shape) for t in (half_life, residual)]
        ctx.devices = (susc.device, inf.device, new_infected.device)
        ctx.save_for_backward(susc0, flags)
        return out_s, out_i

    @staticmethod
    def backward(ctx, g_susc, g_inf):
        import math

        env = ctx.env
        susc0, flags = ctx.saved_tensors
        plan, dev, n = env["plan"], susc0.device, susc0.numel()
        g_susc, g_inf = _f32(g_susc, dev), _f32(g_inf, dev)
        B = plan.n_groups
        contrib = torch.empty(max(1, 2 * n), dtype=torch.float64, device=dev)
        partial = torch.empty(max(1, 2 * plan.n_chunks), dtype=torch.float64, device=dev)
        sums = torch.empty(2, B, dtype=torch.float64, device=dev)
        want_s, want_i, want_n = ctx.needs_input_grad[3:6]
        gs_in = torch.empty(n, dtype=torch.float32, device=dev) if want_s else None
        gn = torch.empty(n, dtype=torch.float32, device=dev) if want_n else None
        N.check(N.load().gj_adjoint_immunity(n, N.ptr(flags), N.ptr(env["cls"]), env["tables"], N.ptr(susc0),
                                             N.ptr(g_susc), N.ptr(g_inf), N.ptr(env["band"]), B, C.byref(plan.c),
                                             N.ptr(contrib), N.ptr(partial), N.ptr(sums[0]), N.ptr(sums[1]),
                                             N.ptr(gs_in), None, N.ptr(gn), N.current_stream()), "gj_adjoint_immunity")
        grads = [None, None]
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            if env.get("all_reduce") is not None:
                sums = env["all_reduce"](sums.reshape(-1)).reshape(2, B)      # fp64: the world's sums on every rank
            sum_a, sum_b = sums.cpu().tolist()
            dt, (hs, _) = env["dt"], ctx.values
            keep = [2.0 ** (-dt / h) for h in hs]
            d_h = [0.0 if math.isinf(h) else -a * k * math.log(2.0) * dt / (h * h) for a, k, h in zip(sum_a, keep, hs)]
            d_r = [-b * (1.0 - k) for b, k in zip(sum_b, keep)]
            for i, d in enumerate((d_h, d_r)):
                if ctx.needs_input_grad[1 + i]:
                    like_dev, like_dtype, like_shape = ctx.like[i]
                    grads[i] = torch.tensor(d, dtype=torch.float64).to(device=like_dev, dtype=like_dtype).reshape(like_shape)
        if want_i and g_inf is None:
            g_inf = torch.zeros(n, dtype=torch.float32, device=dev)
        return (None, *grads, *_to_devices((gs_in, g_inf if want_i else None, gn), ctx.devices))


class TestingStep(torch.autograd.Function):
    """One launch of a ``Testing`` policy as an autograd node (``policies.TestingPolicies.step``): (probability [B],
    current_stage, y) -> (y', row).  ``y`` is the policy's ``positive`` array on the graph: a deciding agent's ``y' =
    hard * stage / stage.detach()``, everybody else's is the incoming one; ``row`` is the launch's newly confirmed cases,
    ``sum due * y'``, a float32 scalar.  Forward = ``gj_testing_step`` on the policy's state, keeping its ``flags`` (1 B
    per agent and step); backward = ``gj_adjoint_testing``, which sums the cotangents of the deciding agents per band in
    fp64 in the order of the bands' ``SeedPlan`` (a straight-through estimator: ``d y / d probability := 1``) and hands
    ``g * hard / stage`` to the stage.  ``env``: what ``policies.testing_launch`` takes, ``band`` with its ``plan`` and -
    on a rank of a partitioned world - ``all_reduce`` (as ``VaccinationStep``)."""

    @staticmethod
    def forward(ctx, env, probability, stage, y):
        from .policies import testing_launch

        dev, n = env["cls"].device, env["n"]
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        testing_launch(dict(env, counts=counts), flags)
        if env["counts"] is not None:
            env["counts"].add_(counts)
        ctx.env = {k: env[k] for k in ("band", "plan", "all_reduce")}
        ctx.like = (probability.device, probability.dtype, probability.shape)
        ctx.devices = (stage.device, y.device)
        ctx.save_for_backward(env["stage"], flags)
        return env["held"]["positive"].clone(), counts[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g_y, g_row):
        env = ctx.env
        stage, flags = ctx.saved_tensors
        plan, dev, n = env["plan"], stage.device, stage.numel()
        g_y = _f32(g_y, dev)
        g_row = None if g_row is None else _f32(g_row, dev).reshape(1)
        B = plan.n_groups
        contrib = torch.empty(max(1, n), dtype=torch.float64, device=dev)
        partial = torch.empty(max(1, plan.n_chunks), dtype=torch.float64, device=dev)
        sums = torch.empty(B, dtype=torch.float64, device=dev)
        want_p, want_s, want_y = ctx.needs_input_grad[1:4]
        g_stage = torch.empty(n, dtype=torch.float32, device=dev) if want_s else None
        g_y_in = torch.empty(n, dtype=torch.float32, device=dev) if want_y else None
        N.check(N.load().gj_adjoint_testing(n, N.ptr(flags), N.ptr(stage), N.ptr(g_y), N.ptr(g_row), N.ptr(env["band"]),
                                            B, C.byref(plan.c), N.ptr(contrib), N.ptr(partial), N.ptr(sums),
                                            N.ptr(g_stage), N.ptr(g_y_in), N.current_stream()), "gj_adjoint_testing")
        g_prob = None
        if want_p:
            if env.get("all_reduce") is not None:
                sums = env["all_reduce"](sums)      # fp64: the world's sums on every rank
            like_dev, like_dtype, like_shape = ctx.like
            g_prob = sums.to(device=like_dev, dtype=like_dtype).reshape(like_shape)
        return (None, g_prob, *_to_devices((g_stage, g_y_in), ctx.devices))


class SymptomsStep(torch.autograd.Function):
    """(new_infected, current_stage, next_stage, time_to_next_stage) -> the three updated arrays, with the
    reference's gradient paths (symptoms.py:98,105-124,231-236): a loss on the stages - the deaths series of
    runner.py:198-215 - reaches ``log_beta`` through ``new_infected``.  All three outputs carry a gradient,
    as test_symptoms.py:208-231 expects.  Forward = ``gj_symptoms_update`` on
    fresh tensors; backward = ``gj_adjoint_symptoms`` replaying the branch each agent took."""

    @staticmethod
    def forward(ctx, env, new_infected, cur, nxt, ttn):
        lib = N.load()
        n = new_infected.numel()
        nw, cur0, nxt0, ttn0 = (_f32(t) for t in (new_infected, cur, nxt, ttn))
        out_c, out_x, out_t = cur0.clone(), nxt0.clone(), ttn0.clone()
        p = env["params"]
        N.check(lib.gj_symptoms_update(n, N.ptr(env["cls"]), N.ptr(nw), N.ptr(out_c), N.ptr(out_x), N.ptr(out_t),
                                       C.byref(p), N.ptr(env["progresses"]), N.ptr(env["dwell"]), N.current_stream()),
                "gj_symptoms_update")
        snap = N.SymptomsParams()                       # the caller reuses its struct: keep this call's clock / key
        C.memmove(C.byref(snap), C.byref(p), C.sizeof(N.SymptomsParams))
        ctx.env = {"cls": env["cls"], "progresses": env["progresses"], "dwell": env["dwell"], "params": snap,
                   "table": env.get("table")}
        ctx.save_for_backward(nw, cur0, nxt0, ttn0)
        return out_c, out_x, out_t

    @staticmethod
    def backward(ctx, g_cur, g_nxt, g_ttn):
        nw, cur0, nxt0, ttn0 = ctx.saved_tensors
        env = ctx.env
        n = nw.numel()
        g_cur, g_nxt, g_ttn = _f32(g_cur), _f32(g_nxt), _f32(g_ttn)
        g_cur_in, g_nxt_in, g_ttn_in, g_new = (torch.empty_like(nw) for _ in range(4))
        N.check(N.load().gj_adjoint_symptoms(n, N.ptr(env["cls"]), N.ptr(nw), N.ptr(cur0), N.ptr(nxt0), N.ptr(ttn0),
                                             C.byref(env["params"]), N.ptr(env["progresses"]), N.ptr(env["dwell"]),
                                             N.ptr(g_cur), N.ptr(g_nxt), N.ptr(g_ttn), N.ptr(g_cur_in),
                                             N.ptr(g_nxt_in), N.ptr(g_ttn_in), N.ptr(g_new), N.current_stream()),
                "gj_adjoint_symptoms")
        return None, g_new, g_cur_in, g_nxt_in, g_ttn_in


class GroupSeriesRow(torch.autograd.Function):
    """One row of the per-group result series as an autograd node: (is_infected, current_stage) -> (cases [G],
    deaths [G]), the float32 values of the fp64 sums ``sum_{group[a] == g} is_infected[a]`` and
    ``sum (stage == dead) * stage / dead`` (runner.py:198-215, 235-242 of the reference, for every group at once).
    ``env``: ``{"stats": groups.GroupStats, "dead": id of the dead stage}``.  Forward = ``gj_group_stats`` on a zeroed
    row; backward = ``gj_adjoint_group_stats``, a gather through the labels that writes only the gradients autograd
    asks for."""

    @staticmethod
    def forward(ctx, env, is_infected, current_stage):
        stats, dead = env["stats"], int(env["dead"])
        dev = stats.labels.device
        inf, stage = _f32(is_infected, dev), _f32(current_stage, dev)
        row = torch.zeros(2 * stats.n_groups, dtype=torch.float64, device=dev)
        stats.add(inf, stage, dead, row)
        ctx.stats, ctx.dead = stats, dead
        ctx.devices = (is_infected.device, current_stage.device)
        ctx.save_for_backward(stage)
        row = row.to(torch.float32)
        return row[: stats.n_groups].clone(), row[stats.n_groups:].clone()

    @staticmethod
    def backward(ctx, g_cases, g_deaths):
        stats = ctx.stats
        (stage,) = ctx.saved_tensors
        dev = stats.labels.device
        want_inf, want_stage = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grads = stats.gather(stage, ctx.dead, _f32(g_cases, dev), _f32(g_deaths, dev), want_inf, want_stage)
        return (None, *_to_devices(grads, ctx.devices))


class StageSeriesRow(torch.autograd.Function):
    """One row of the symptom-stage series as an autograd node: current_stage -> (occupancy [G, S], entries [G, S]),
    the float32 values of the counts of ``gj_stage_stats``, differentiable in the reference's form
    ``sum (stage == s) * stage / s`` (column 0, ``recovered``, is a plain count).  ``env``: ``{"stats":
    groups.StageStats, "prev": the previous row's stage, a detached constant, or None}``.  Forward = ``gj_stage_stats``
    on a zeroed row; backward = ``gj_adjoint_stage_stats``, a gather through (label, stage)."""

    @staticmethod
    def forward(ctx, env, current_stage):
        stats = env["stats"]
        dev = stats.device
        stage, prev = _f32(current_stage, dev), _f32(env.get("prev"), dev)
        row = torch.zeros(2, stats.n_groups, stats.n_stages, dtype=torch.int64, device=dev)
        stats.add(stage, prev, row)
        ctx.stats, ctx.prev, ctx.device = stats, prev, current_stage.device
        ctx.save_for_backward(stage)
        row = row.to(torch.float32)
        return row[0].clone(), row[1].clone()

    @staticmethod
    def backward(ctx, g_occupancy, g_entries):
        (stage,) = ctx.saved_tensors
        dev = ctx.stats.device
        grad = ctx.stats.gather(stage, ctx.prev, _f32(g_occupancy, dev), _f32(g_entries, dev))
        return None, grad.to(ctx.device)
