"""Stochastic flow layers: ``BrownianFlow`` (alias ``OverdampedLangevinFlow``), ``LangevinFlow`` (bgflow/nn/flow/stochastic/langevin.py)
and ``MetropolisMCFlow`` (stochastic/mcmc.py) with the reference's constructor signatures and attribute names.  ``forward(x)`` returns
``(x', dW)``, ``LangevinFlow.forward(q, v)`` returns ``(q', v', dW)``; dW [B, 1] is the log ratio of the forward and backward path
probabilities.  ``_inverse`` is ``_forward``; keyword arguments (``temperature``, ...) are ignored, as in the reference.

The general path restates the reference's formulas line for line in torch ops over ``energy_model.force`` / ``energy_model.energy``: any
energy, device, dtype or shape.  Two deliberate deviations: noise and dW are created on the input's device and in its dtype (the
reference creates f32 CPU tensors and cannot run on a GPU input), and the debugging attributes ``w``, ``w_``, ``q111`` are not kept.
While grad is enabled and an input requires grad the forces are ``-autograd.grad(E.sum(), x, create_graph=True)``, so the layer stays
twice differentiable (for the particle targets of this package over their torch formulas: the kernel's backward is once differentiable).

The fused path runs all ``nsteps`` in launches of at most ``LANGEVIN_MAX_STEPS_PER_LAUNCH`` steps of csrc/bgk_langevin.hip (entry
bgk_pair_langevin; ``MetropolisMCFlow``: one bgk_pair_energy launch for E0, then bgk_pair_mcmc, the chain kernel of sampling.py, split at
its own cap) on copies of the inputs.  It applies when ``energy_model`` is a particle-system target with a ``PairPlan`` at temperature 1
(2..64 particles in 1..3 dimensions), the inputs are contiguous f32 HIP tensors [B, n d] with B > 0, the settings are plain numbers
(``stepsize > 0``, ``mass > 0``, ``gamma >= 0``, ``kT > 0``) and no input requires grad while grad is enabled.  The class attribute
``fused = False`` forces the general path.

The fused backward is opt-in: with the class attribute ``fused_backward = True`` (default False: the general path stays twice
differentiable, the fused one is not) an input that requires grad while grad is enabled, under every other condition of the fused
path, runs the recording forward bgk_pair_langevin_record -- the same q, v and dW bit for bit, plus the state after every step -- and its
``autograd.Function`` (``_BrownianFn`` / ``_LangevinFn``, once differentiable) sweeps the recorded run backwards with
bgk_pair_langevin_backward, in launches of at most ``LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH`` steps, last segment first: one gradient
and one Hessian-vector product of the pair energy per state for Brownian, one Hessian-vector product for Langevin, whose noise the
kernel regenerates from the saved stream position (or reads from the fed slices).  The recorded states take ``nsteps B n d 4`` bytes
(twice that for Langevin); above ``LANGEVIN_BACKWARD_MAX_BYTES`` the layer takes the general path with a ``RuntimeWarning``.
``MetropolisMCFlow`` with ``fused_backward``: the fused forward, and g_x = g_y + g_dW (dE/dx(y) - dE/dx(x)) from two
bgk_pair_energy_backward launches (the reference's selection (1 - acc) x + acc xprop has the identity as its Jacobian).

Random numbers of the fused path come from the object's Philox stream (``_FusedSampling``: key from ``torch.initial_seed()``, rank and
stream id, the per-object counter is the index of the next step, both travel in ``state_dict``), unless ``feed_noise`` has handed the
object explicit ones; fed numbers are also what the general path then uses, one row per step.  ``chain_offset`` is the global index of
the batch's first row: a batch sharded over processes draws the numbers of the whole.

``AnnealedMCFlow`` (not in the reference) anneals between two energies along a schedule on the protocol of annealing.py (fused:
csrc/bgk_anneal.hip); its dW carries the nonequilibrium work.
"""
import math
import warnings

import torch

from .distributions import BoxPlan, Energy, PairPlan, _FusedSampling, _kernel_plan
from .flow import Flow
from .particles import _check_tensors, _energy_backward, _is_number, _target_args

__all__ = ["BrownianFlow", "OverdampedLangevinFlow", "LangevinFlow", "MetropolisMCFlow", "AnnealedMCFlow"]

# The most steps one launch of bgk_pair_langevin runs; longer runs are split (the same q and v bit for bit: the random stream does not
# depend on the split; dW is then the f32 sum of the launches' dW), so that no single launch holds a shared GPU for long.  Measured on
# an MI355X (tools/langevin_time.py, its last lines): at the widest shape of the envelope -- Lennard-Jones, n = 64, d = 3, 2^16 samples --
# one launch of 16 steps takes 38.66 ms for Brownian (2.42 ms per step) and 61.62 ms for Langevin (61.32 .. 61.95 over three rounds,
# 3.85 ms per step), so 64 steps of the slower one are 0.246 s.
LANGEVIN_MAX_STEPS_PER_LAUNCH = 64

# The most steps one launch of bgk_pair_langevin_backward sweeps, by the same rule: no launch longer than a quarter of a second at the
# widest shape.  Measured on an MI355X (tools/langevin_time.py --backward --cap-steps 4, its last lines): at Lennard-Jones, n = 64, d = 3,
# 2^16 samples one launch over 4 steps (the run's first segment: five states) takes 35.77 ms for Brownian (35.32 .. 36.15 over three
# rounds, 8.94 ms per step: a gradient and a Hessian-vector product per state) and 27.23 ms for Langevin (27.04 .. 27.32, 6.81 ms per
# step), 3.7 and 1.8 times the forward's step.  24 steps of the slower one are 0.215 s (27 would be 0.241 s).
LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH = 24

# The most bytes of recorded states (nsteps B n d 4, twice that for Langevin) the fused backward keeps; beyond, the general path.  A
# policy constant, not a measurement: 1 GiB beside the model's activations.
LANGEVIN_BACKWARD_MAX_BYTES = 2 ** 30


def _split(total, cap):
    cap = max(1, int(cap))
    return [min(cap, total - s) for s in range(0, total, cap)]


def _force(energy_model, x):
    """-dE/dx.  An input that carries a graph: through autograd with ``create_graph`` (a particle target of this package over its torch
    formulas); otherwise ``energy_model.force`` on a detached alias, so that the caller's tensor keeps its ``requires_grad``."""
    if torch.is_grad_enabled() and x.requires_grad:
        if isinstance(_kernel_plan(energy_model, 1.0), (PairPlan, BoxPlan)):
            e = Energy.energy(energy_model, x)
        else:
            e = energy_model.energy(x)
        return -torch.autograd.grad(e.sum(), x, create_graph=True)[0]
    with torch.enable_grad():
        return energy_model.force(x.detach()).detach()


def _row_sum(t):
    """sum over everything but the batch: [B, 1] (the reference's ``sum(axis=1, keepdims=True)`` of a [B, n d] tensor)"""
    return t.reshape(t.shape[0], -1).sum(dim=1, keepdim=True)


def _check_launch(name, plan, q, v, w1, w2, tensors):
    """the argument checks of the bgk_pair_langevin* wrappers: ``tensors`` = (tensor or None, shape) pairs"""
    nd = q.shape[1]
    if nd != plan.n_particles * plan.n_dims:
        raise ValueError(f"{name}: q has {nd} columns, the target {plan.n_particles} x {plan.n_dims}")
    if (w2 is not None) != (w1 is not None and v is not None):
        raise ValueError(f"{name}: w1 alone without velocities, w1 and w2 with them")
    _check_tensors(name, q, tensors)


def pair_langevin(plan, q, v, stepsize, mass, gamma, kT, n_steps, dW, w1=None, w2=None, seed=0, offset=0, row0=0, accumulate=False):
    """One launch of bgk_pair_langevin: ``n_steps`` Brownian (``v`` None) or Langevin steps of q (and v) [B, n d] (f32, contiguous, HIP;
    updated IN PLACE) on the target of the ``PairPlan``.  dW [B]: written, or added to with ``accumulate``.  w1 (and, with v, w2)
    [n_steps, B, n d], or neither (Philox numbers of (seed, offset + step, row row0 + b))."""
    from . import _lib
    B, nd = q.shape
    _check_launch("pair_langevin", plan, q, v, w1, w2,
                  ((q, (B, nd)), (v, (B, nd)), (dW, (B,)), (w1, (n_steps, B, nd)), (w2, (n_steps, B, nd))))
    with torch.cuda.device(q.device):
        st = _lib.lib().bgk_pair_langevin(_lib.ptr(q), _lib.ptr(v), B, *_target_args(plan), float(stepsize), float(mass), float(gamma),
                                          float(kT), int(n_steps), _lib.ptr(w1), _lib.ptr(w2), int(seed) & (2 ** 64 - 1),
                                          int(offset) & 0xffffffff, int(row0), _lib.ptr(dW), int(bool(accumulate)),
                                          _lib.stream_ptr(q.device))
    _lib.check(st, "bgk_pair_langevin")


def pair_langevin_record(plan, q, v, stepsize, mass, gamma, kT, n_steps, dW, traj_q, traj_v=None, w1=None, w2=None, seed=0, offset=0, row0=0,
                         accumulate=False):
    """One launch of bgk_pair_langevin_record: ``pair_langevin`` (the same q, v, dW bit for bit) that also writes the state after every
    step into traj_q [n_steps, B, n d] and, with velocities, traj_v."""
    from . import _lib
    B, nd = q.shape
    if (traj_v is None) != (v is None):
        raise ValueError("pair_langevin_record: traj_v exactly with velocities")
    _check_launch("pair_langevin_record", plan, q, v, w1, w2,
                  ((q, (B, nd)), (v, (B, nd)), (dW, (B,)), (w1, (n_steps, B, nd)), (w2, (n_steps, B, nd)), (traj_q, (n_steps, B, nd)),
                   (traj_v, (n_steps, B, nd))))
    with torch.cuda.device(q.device):
        st = _lib.lib().bgk_pair_langevin_record(_lib.ptr(q), _lib.ptr(v), B, *_target_args(plan), float(stepsize), float(mass),
                                                 float(gamma), float(kT), int(n_steps), _lib.ptr(w1), _lib.ptr(w2), int(seed) & (2 ** 64 - 1),
                                                 int(offset) & 0xffffffff, int(row0), _lib.ptr(dW), int(bool(accumulate)), _lib.ptr(traj_q),
                                                 _lib.ptr(traj_v), _lib.stream_ptr(q.device))
    _lib.check(st, "bgk_pair_langevin_record")


def pair_langevin_backward(plan, q0, v0, traj_q, traj_v, stepsize, mass, gamma, kT, g_dW, gq, gv, carry, first, w1=None, w2=None, seed=0,
                           offset=0, row0=0):
    """One launch of bgk_pair_langevin_backward: the reverse sweep over a recorded segment.  q0 (v0) [B, n d]: the state before the
    segment, traj_q (traj_v) [n_steps, B, n d]: the states after its steps, w1 / w2 or (seed, offset, row0): the noise of these steps as
    the forward launch had it, g_dW [B]: d L / d dW.  gq (gv) and carry [B, n d] are updated IN PLACE: before the last segment's sweep
    gq (gv) = d L / d (final state) and carry = 0; after the first segment's (``first``) gq (gv) = d L / d (initial state)."""
    from . import _lib
    B, nd = q0.shape
    n_steps = traj_q.shape[0]
    if not (v0 is None) == (traj_v is None) == (gv is None):
        raise ValueError("pair_langevin_backward: v0, traj_v and gv go together")
    _check_launch("pair_langevin_backward", plan, q0, v0, w1, w2,
                  ((q0, (B, nd)), (v0, (B, nd)), (traj_q, (n_steps, B, nd)), (traj_v, (n_steps, B, nd)), (g_dW, (B,)), (gq, (B, nd)),
                   (gv, (B, nd)), (carry, (B, nd)), (w1, (n_steps, B, nd)), (w2, (n_steps, B, nd))))
    with torch.cuda.device(q0.device):
        st = _lib.lib().bgk_pair_langevin_backward(_lib.ptr(q0), _lib.ptr(v0), _lib.ptr(traj_q), _lib.ptr(traj_v), B, *_target_args(plan),
                                                   float(stepsize), float(mass), float(gamma), float(kT), int(n_steps), _lib.ptr(w1),
                                                   _lib.ptr(w2), int(seed) & (2 ** 64 - 1), int(offset) & 0xffffffff, int(row0),
                                                   _lib.ptr(g_dW), _lib.ptr(gq), _lib.ptr(gv), _lib.ptr(carry), int(bool(first)),
                                                   _lib.stream_ptr(q0.device))
    _lib.check(st, "bgk_pair_langevin_backward")


class _IntegratorFn(torch.autograd.Function):
    """``BrownianFlow`` / ``LangevinFlow`` on the recording forward, with the adjoint sweep of bgk_pair_langevin_backward as backward:
    ``apply(flow, plan, *xs)`` -> (*ys, dW [B, 1]).  Saved: the inputs, the recorded states and, for Langevin, the fed slices (views of
    the caller's tensors) or the stream position."""

    @staticmethod
    def forward(ctx, flow, plan, *xs):
        q = xs[0]
        B, nd = q.shape
        n_steps = flow.nsteps
        fed, seed, offset = flow._stream(q, n_steps)
        settings = flow._launch_settings()
        state = [x.detach().clone() for x in xs]
        traj = [torch.empty((n_steps, B, nd), dtype=torch.float32, device=q.device) for _ in xs]
        dW = torch.empty(B, dtype=torch.float32, device=q.device)
        done = 0
        for k in _split(n_steps, LANGEVIN_MAX_STEPS_PER_LAUNCH):
            noise = [None, None] if fed is None else [t[done:done + k] for t in fed] + [None] * (2 - len(fed))
            pair_langevin_record(plan, state[0], state[1] if len(xs) == 2 else None, *settings, k, dW, traj[0][done:done + k],
                                 traj[1][done:done + k] if len(xs) == 2 else None, noise[0], noise[1], seed, offset + done,
                                 flow.chain_offset, accumulate=done > 0)
            done += k
        keep = (fed or []) if len(xs) == 2 else []      # the Brownian sweep needs no noise
        ctx.save_for_backward(*[x.detach() for x in xs], *traj, *keep)
        ctx.cfg = (plan, settings, len(xs), seed, offset, flow.chain_offset)
        return (*state, dW[:, None])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        plan, settings, n_in, seed, offset, row0 = ctx.cfg
        saved = ctx.saved_tensors
        x0, traj, fed = saved[:n_in], saved[n_in:2 * n_in], saved[2 * n_in:]
        n_steps = traj[0].shape[0]
        adj = [g.to(torch.float32).contiguous().clone() for g in grads[:n_in]]
        g_dW = grads[n_in].reshape(-1).to(torch.float32).contiguous()
        carry = torch.zeros_like(adj[0])
        sizes = _split(n_steps, LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH)
        starts = [sum(sizes[:i]) for i in range(len(sizes))]
        for s, k in reversed(list(zip(starts, sizes))):
            before = [x0[i] if s == 0 else traj[i][s - 1] for i in range(n_in)]
            noise = [t[s:s + k] for t in fed] + [None] * (2 - len(fed))
            pair_langevin_backward(plan, before[0], before[1] if n_in == 2 else None, traj[0][s:s + k], traj[1][s:s + k] if n_in == 2 else None,
                                   *settings, g_dW, adj[0], adj[1] if n_in == 2 else None, carry, s == 0, noise[0], noise[1], seed,
                                   offset + s, row0)
        return (None, None, *adj)


# Two names on purpose: an output's ``grad_fn`` says which layer made it (the tests assert the names).  Do not fold them into one.
class _BrownianFn(_IntegratorFn):
    """``BrownianFlow`` with the fused backward"""


class _LangevinFn(_IntegratorFn):
    """``LangevinFlow`` with the fused backward"""


class _MetropolisFn(torch.autograd.Function):
    """``MetropolisMCFlow`` on its fused forward; backward g_x = g_y + g_dW (dE/dx(y) - dE/dx(x)), two bgk_pair_energy_backward launches"""

    @staticmethod
    def forward(ctx, flow, setup, x):
        y, dW = flow._fused_forward(x, setup)
        ctx.save_for_backward(x.detach(), y)
        ctx.plan = setup[0]
        return y, dW

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y, g_dW):
        x, y = ctx.saved_tensors
        g = g_dW.reshape(-1).to(torch.float32).contiguous()
        out = g_y.to(torch.float32).clone()
        for state, g_u in ((y, g), (x, -g)):
            out += _energy_backward(ctx.plan, state, g_u)
        return None, None, out


class _StochasticFlow(Flow, _FusedSampling):
    """what the three layers share: the settings, fed random numbers, the conditions of the fused path and its Philox position"""
    fused = True
    fused_backward = False     # opt in to the once-differentiable fused backward (module docstring)

    def __init__(self, energy_model, nsteps, stepsize):
        super().__init__()
        self.energy_model = energy_model
        self.nsteps = nsteps
        self.stepsize = stepsize
        self.chain_offset = 0      # global index of the batch's first row
        self._fed = None

    def _inverse(self, *xs, **kwargs):
        """same as forward"""
        return self._forward(*xs, **kwargs)

    # -- fed random numbers
    def _feed(self, tensors, shapes):
        if all(t is None for t in tensors):
            self._fed = None
            return self
        if any(t is None for t in tensors) or any(t.dim() != d for t, d in zip(tensors, shapes)) or any(
                t.shape[:2] != tensors[0].shape[:2] for t in tensors):
            raise ValueError(f"feed_noise: {self._fed_doc}")
        self._fed = [[t.contiguous() for t in tensors], 0]
        return self

    def _fed_rows(self, like):
        """general path: the next row of every fed tensor, on ``like``'s device and in its dtype, or None"""
        fed = self._fed
        if fed is None:
            return None
        if fed[1] >= fed[0][0].shape[0]:
            raise ValueError(f"{type(self).__name__}: the fed random numbers are used up ({fed[1]} rows)")
        rows = [t[fed[1]].to(device=like.device, dtype=like.dtype) for t in fed[0]]
        fed[1] += 1
        return rows

    def _normal(self, like, row):
        return torch.randn_like(like) if row is None else row.reshape(like.shape)

    # -- the fused path
    def _settings_ok(self):
        return _is_number(self.stepsize) and self.stepsize > 0 and math.isfinite(self.stepsize)

    def _fused_setup(self, *xs):
        """(plan, B) if the kernels take these inputs, else None"""
        if not self.fused or not self._settings_ok() or not (isinstance(self.nsteps, int) and self.nsteps >= 1):
            return None
        plan = _kernel_plan(self.energy_model, 1.0)
        if not isinstance(plan, PairPlan):
            return None
        nd = plan.n_particles * plan.n_dims
        for x in xs:
            if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
                    and x.shape[0] > 0 and x.shape[1] == nd and x.shape == xs[0].shape and x.device == xs[0].device):
                return None
            if torch.is_grad_enabled() and x.requires_grad:
                return None
        return plan, xs[0].shape[0]

    def _traj_bytes(self, B, nd):
        """bytes of recorded states the fused backward keeps for a [B, n d] batch"""
        return 0

    def _fused_train_setup(self, *xs):
        """(plan, B) if the fused backward takes these inputs -- the conditions of ``_fused_setup`` but for the inputs' requires_grad,
        and the recorded states within ``LANGEVIN_BACKWARD_MAX_BYTES`` (else one RuntimeWarning) -- else None.  ``_forward`` asks only
        with ``fused_backward`` set, grad enabled and an input that requires grad."""
        with torch.no_grad():
            setup = self._fused_setup(*xs)
        if setup is None:
            return None
        need = self._traj_bytes(setup[1], xs[0].shape[1])
        if need > LANGEVIN_BACKWARD_MAX_BYTES:
            warnings.warn(f"{type(self).__name__}: the fused backward would record {need} bytes of states, more than "
                          f"LANGEVIN_BACKWARD_MAX_BYTES = {LANGEVIN_BACKWARD_MAX_BYTES}; taking the general path", RuntimeWarning, stacklevel=3)
            return None
        return setup

    def _trains_fused(self, *xs):
        """the setup of the fused backward, or None: asked only when the layer is to be differentiated"""
        if not (self.fused_backward and torch.is_grad_enabled() and any(torch.is_tensor(x) and x.requires_grad for x in xs)):
            return None
        return self._fused_train_setup(*xs)

    def _stream(self, x, total):
        """(fed tensors of the next ``total`` steps or None, seed, offset) and the stream / fed position advanced by ``total``"""
        fed = self._fed
        if fed is not None:
            left = fed[0][0].shape[0] - fed[1]
            if left < total or any(t.shape[1] != x.shape[0] or t.device != x.device or t.dtype != torch.float32 for t in fed[0]) \
                    or fed[0][0].shape[2:] != x.shape[1:]:
                raise ValueError(f"{type(self).__name__}: {total} steps of a {tuple(x.shape)} batch need as many rows of fed f32 numbers on "
                                 f"its device; {left} rows of {tuple(fed[0][0].shape[1:])} are left")
            pos, fed[1] = fed[1], fed[1] + total
            return [t[pos:pos + total] for t in fed[0]], 0, 0
        from . import dp
        st = self._philox_ids()
        seed = (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1)
        offset, st[1] = st[1], st[1] + total
        return None, seed, offset


class BrownianFlow(_StochasticFlow):
    """Overdamped Langevin / Brownian dynamics (langevin.py:7-49): per step, with h = ``stepsize`` and f = ``energy_model.force``,

        y = x + h f(x) + sqrt(2 h) w,    w_ = (x - y - h f(y)) / sqrt(2 h),    dW += 0.5 sum (w^2 - w_^2),    w ~ N(0, 1)

    f(y) of a step is f(x) of the next: one force evaluation per step, plus one at the start."""
    _fed_doc = "noise [S, B, n d]"

    def __init__(self, energy_model, nsteps=1, stepsize=0.01):
        super().__init__(energy_model, nsteps, stepsize)

    def feed_noise(self, noise):
        """explicit standard normals [S, B, n d] for the next steps instead of the random stream (fused path: f32, on the input's
        device); each step consumes one row, ``feed_noise(None)`` returns to the stream"""
        return self._feed([noise], [3])

    def _forward(self, x, **kwargs):
        setup = self._fused_setup(x)
        if setup is not None:
            return self._fused_forward(x, setup)
        setup = self._trains_fused(x)
        if setup is not None:
            return _BrownianFn.apply(self, setup[0], x)
        dW = torch.zeros((x.shape[0], 1), dtype=x.dtype, device=x.device)
        root = math.sqrt(2 * self.stepsize)
        f = _force(self.energy_model, x) if self.nsteps > 0 else None
        for _ in range(self.nsteps):
            rows = self._fed_rows(x)
            # forward noise
            w = self._normal(x, None if rows is None else rows[0])
            # forward step
            y = x + self.stepsize * f + root * w
            # backward noise
            f = _force(self.energy_model, y)
            w_ = (x - y - self.stepsize * f) / root
            # noise ratio
            dW = dW + 0.5 * _row_sum(w ** 2 - w_ ** 2)
            # update state
            x = y
        return x, dW

    def _traj_bytes(self, B, nd):
        return self.nsteps * B * nd * 4

    def _launch_settings(self):
        return self.stepsize, 1.0, 0.0, 1.0

    def _fused_forward(self, x, setup):
        plan, B = setup
        fed, seed, offset = self._stream(x, self.nsteps)
        y = x.detach().clone()
        dW = torch.empty(B, dtype=torch.float32, device=x.device)
        done = 0
        for k in _split(self.nsteps, LANGEVIN_MAX_STEPS_PER_LAUNCH):
            pair_langevin(plan, y, None, self.stepsize, 1.0, 0.0, 1.0, k, dW, None if fed is None else fed[0][done:done + k], None,
                          seed, offset + done, self.chain_offset, accumulate=done > 0)
            done += k
        return y, dW[:, None]


OverdampedLangevinFlow = BrownianFlow  # alias


class LangevinFlow(_StochasticFlow):
    """Langevin dynamics (langevin.py:54-122): per step, with h = ``stepsize``, gm = ``gamma * mass``, fac1 = sqrt(4 gm kT / h),
    fac2 = sqrt(gm h / kT) and two normal draws w1, w2,

        vh = v1 + h / (2 mass) (f(q1) - gm v1 + fac1 w1),    q2 = q1 + h vh,    v2 = (vh + h / (2 mass) (f(q2) + fac1 w2)) / (1 + gamma h / 2),
        w1_ = w2 - fac2 v2,    w2_ = w1 - fac2 v1,    dW += 0.5 sum (w1^2 + w2^2 - w1_^2 - w2_^2)

    f(q2) of a step is f(q1) of the next: one force evaluation per step, plus one at the start."""
    _fed_doc = "w1 and w2, each [S, B, n d]"

    def __init__(self, energy_model, nsteps=1, stepsize=0.01, mass=1.0, gamma=1.0, kT=1.0):
        super().__init__(energy_model, nsteps, stepsize)
        self.mass = mass
        self.gamma = gamma
        self.kT = kT

    def feed_noise(self, w1, w2):
        """explicit standard normals w1, w2 [S, B, n d] for the next steps instead of the random stream (fused path: f32, on the
        inputs' device); each step consumes one row of either, ``feed_noise(None, None)`` returns to the stream"""
        return self._feed([w1, w2], [3, 3])

    def _settings_ok(self):
        return (super()._settings_ok() and _is_number(self.mass, self.gamma, self.kT) and self.mass > 0 and self.gamma >= 0 and self.kT > 0
                and all(math.isfinite(v) for v in (self.mass, self.gamma, self.kT)))

    def _forward(self, q, v, **kwargs):
        setup = self._fused_setup(q, v)
        if setup is not None:
            return self._fused_forward(q, v, setup)
        setup = self._trains_fused(q, v)
        if setup is not None:
            return _LangevinFn.apply(self, setup[0], q, v)
        dW = torch.zeros((q.shape[0], 1), dtype=q.dtype, device=q.device)
        gamma_m = self.gamma * self.mass
        # naming convention: 1, h, 2 timesteps. _: backward
        q1 = q
        v1 = v
        fac1 = math.sqrt(4.0 * gamma_m * self.kT / self.stepsize)
        fac2 = math.sqrt(gamma_m * self.stepsize / self.kT)
        f1 = _force(self.energy_model, q1) if self.nsteps > 0 else None
        for _ in range(self.nsteps):
            rows = self._fed_rows(q)
            # forward noise
            w1 = self._normal(q, None if rows is None else rows[0])
            w2 = self._normal(q, None if rows is None else rows[1])
            # forward step
            vh = v1 + (self.stepsize / (2.0 * self.mass)) * (f1 - gamma_m * v1 + fac1 * w1)
            q2 = q1 + self.stepsize * vh
            f2 = _force(self.energy_model, q2)
            v2 = 1.0 / (1.0 + self.gamma * self.stepsize / 2.0) * (vh + (self.stepsize / (2.0 * self.mass)) * (f2 + fac1 * w2))
            # backward noises
            w1_ = w2 - fac2 * v2
            w2_ = w1 - fac2 * v1
            # noise ratio
            dW = dW + 0.5 * _row_sum(w1 ** 2 + w2 ** 2 - w1_ ** 2 - w2_ ** 2)
            # update state
            q1, v1, f1 = q2, v2, f2
        return q1, v1, dW

    def _traj_bytes(self, B, nd):
        return 2 * self.nsteps * B * nd * 4

    def _launch_settings(self):
        return self.stepsize, self.mass, self.gamma, self.kT

    def _fused_forward(self, q, v, setup):
        plan, B = setup
        fed, seed, offset = self._stream(q, self.nsteps)
        q2, v2 = q.detach().clone(), v.detach().clone()
        dW = torch.empty(B, dtype=torch.float32, device=q.device)
        done = 0
        for k in _split(self.nsteps, LANGEVIN_MAX_STEPS_PER_LAUNCH):
            w1, w2 = (None, None) if fed is None else (fed[0][done:done + k], fed[1][done:done + k])
            pair_langevin(plan, q2, v2, self.stepsize, self.mass, self.gamma, self.kT, k, dW, w1, w2, seed, offset + done,
                          self.chain_offset, accumulate=done > 0)
            done += k
        return q2, v2, dW[:, None]


class MetropolisMCFlow(_StochasticFlow):
    """Metropolis Monte Carlo with a Gaussian proposal of width ``stepsize`` (stochastic/mcmc.py:4-51): per step x' = x + stepsize w is
    accepted if r < exp(-(E(x') - E(x))), r ~ U(0, 1); dW = E(final) - E(start).

    The fused path is one bgk_pair_energy launch for E0 and the chain kernel bgk_pair_mcmc on a copy (``sampling.pair_mcmc``, split at
    ``sampling.MCMC_MAX_STEPS_PER_LAUNCH``).  The kernel's rule -(E' - E) >= log r and the reference's r < exp(-(E' - E)) decide alike
    except at ties (and where the rounding of exp and log differs by an ulp at the boundary).  E0 and the final energies are, bit for
    bit, what ``energy_model.energy`` gives for the states."""
    _fed_doc = "noise [S, B, n d] and uniforms [S, B]"

    def __init__(self, energy_model, nsteps=1, stepsize=0.01):
        super().__init__(energy_model, nsteps, stepsize)

    def feed_noise(self, noise, uniforms):
        """explicit random numbers for the next steps instead of the random stream: noise [S, B, n d] standard normals and uniforms
        [S, B] (fused path: f32, on the input's device); each step consumes one row of either, ``feed_noise(None, None)`` returns to
        the stream"""
        return self._feed([noise, uniforms], [3, 2])

    def _forward(self, x, **kwargs):
        setup = self._fused_setup(x)
        if setup is not None:
            return self._fused_forward(x, setup)
        setup = self._trains_fused(x)
        if setup is not None:
            return _MetropolisFn.apply(self, setup, x)
        E0 = self.energy_model.energy(x)
        E = E0
        batch = (x.shape[0],) + (1,) * (x.dim() - 1)
        for _ in range(self.nsteps):
            rows = self._fed_rows(x)
            # proposal step
            dx = self.stepsize * self._normal(x, None if rows is None else rows[0])
            xprop = x + dx
            Eprop = self.energy_model.energy(xprop)
            # acceptance step
            r = torch.rand(x.shape[0], 1, dtype=x.dtype, device=x.device) if rows is None else rows[1].reshape(-1, 1)
            acc = (r < torch.exp(-(Eprop - E))).to(x.dtype)  # selection variable: 0 or 1.
            x = (1 - acc.reshape(batch)) * x + acc.reshape(batch) * xprop
            E = (1 - acc) * E + acc * Eprop
        # Work is energy difference
        dW = E - E0
        return x, dW

    def _fused_forward(self, x, setup):
        from . import particles, sampling
        plan, B = setup
        fed, seed, offset = self._stream(x, self.nsteps)
        E0 = particles.pair_energy(plan, (x.detach(),))[:, 0]
        y, e = x.detach().clone(), E0.clone()
        done = 0
        for k in _split(self.nsteps, sampling.MCMC_MAX_STEPS_PER_LAUNCH):
            noise, unif = (None, None) if fed is None else (fed[0][done:done + k], fed[1][done:done + k])
            sampling.pair_mcmc(plan, y, e, True, 1.0, self.stepsize, k, noise, unif, seed, offset + done, self.chain_offset)
            done += k
        return y, (e - E0)[:, None]


class AnnealedMCFlow(Flow):
    """Annealed Metropolis Monte Carlo between ``energy_a`` (lambda = 0) and ``energy_b`` (lambda = 1): the protocol of
    ``annealing.AnnealedSwitching`` (its module docstring has the definitions) as a stochastic flow layer, ``nsteps`` steps of width
    ``stepsize`` at every stage of ``lambdas``.  Not in the reference, whose ``MetropolisMCFlow`` thermalises at one energy.

    ``_forward(x)`` returns ``(y, dW)``, dW [B, 1] in x's dtype:  dW = e_B(y) / T_B - e_A(x) / T_A - work.  With this convention
    ``log_weights_given_latent`` of a generator with prior A and target B gives ``-work``, the annealed-importance-sampling weight, and
    for A identical to B (work = 0) the layer reduces to ``MetropolisMCFlow``'s E - E0.  ``_inverse`` runs ``reverse()``, the mirrored
    protocol from B to A, with the mirrored dW = e_A(y) / T_A - e_B(x) / T_B - work'.  Keyword arguments are ignored, as in the other
    stochastic layers.  The protocols are ``switching`` and ``switching_reverse`` (``feed_noise``, ``chain_offset``, ``set_philox_stream``,
    ``fused``, ``n_accepted`` are theirs); the kernel runs only where the input needs no grad, otherwise the torch path."""

    def __init__(self, energy_a, energy_b, lambdas, nsteps=1, stepsize=0.01, temperature_a=1.0, temperature_b=1.0):
        super().__init__()
        from .annealing import AnnealedSwitching
        self.switching = AnnealedSwitching(energy_a, energy_b, lambdas, n_steps=nsteps, noise_std=stepsize, temperature_a=temperature_a,
                                           temperature_b=temperature_b)
        self.switching_reverse = self.switching.reverse()
        self.nsteps = nsteps
        self.stepsize = stepsize

    @staticmethod
    def _switch(protocol, x):
        y, work = protocol._run(x, start=True)
        dW = protocol.e_b.to(torch.float64) / protocol.temperature_b - protocol.e_a_start.to(torch.float64) / protocol.temperature_a - work
        return y, dW.to(x.dtype)[:, None]

    def _forward(self, x, **kwargs):
        return self._switch(self.switching, x)

    def _inverse(self, x, **kwargs):
        return self._switch(self.switching_reverse, x)
