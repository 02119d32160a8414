"""Equivariant kernel-dynamics flow for particle systems (csrc/bgk_kdyn.hip): ``KernelDynamics`` (bgflow/nn/flow/dynamics/kernel_dynamic.py:6-116
with utils/rbf_kernels.py:134-144 and utils/geometry.py:5-48, 93-111) integrated by ``DiffEqFlow`` (nn/flow/diffeq.py:11-96) in the fixed-step
mode (classical RK4 or explicit Euler over ``Nt`` steps).

A contiguous f32 HIP tensor of 2..64 particles in 1..3 dimensions with at most 64 distance and 16 time kernels is evaluated by one launch of
bgk_kdyn_eval (bgk_kdyn_eval_backward for the gradients of x, ``_weights``, ``_bias``, ``_importance`` and ``_neg_log_gammas_time``); without
grad a whole integration is one launch of bgk_kdyn_integrate.  Every other input -- CPU, f64, non-contiguous, more particles or kernels,
training the distance bandwidths -- is evaluated by ``KernelDynamics._forward_torch``, the same formulas as torch ops.

Deviations from the reference: ``mus_time=None`` constructs (the reference raises on ``-torch.log(None)``) and means no time modulation
(one output column, tau = 1); the fixed-step tableau is defined here (the reference delegates to the ``anode`` package): step h = t_max / Nt,
RK4 stages at t, t + h/2, t + h/2, t + h, the log-density change integrated with the same tableau as the positions.
"""
import numpy as np
import torch

from .flow import Flow

__all__ = ["KernelDynamics", "DiffEqFlow", "DensityDynamics", "InversedDynamics"]

KDYN_MAX_PARTICLES, KDYN_MAX_DIMS, KDYN_MAX_KERNELS, KDYN_MAX_TIME_KERNELS = 64, 3, 64, 16     # the envelope of csrc/bgk_kdyn.hip
_METHODS = {"rk4": 0, "euler": 1}


def _rbf_kernels(d, mu, neg_log_gamma, derivative=False):
    """normalised radial basis functions of d [..., 1] and their derivative as the reference forms it (utils/rbf_kernels.py:134-144):
    the second denominator is 1e-6 + s^2"""
    inv_gamma = torch.exp(neg_log_gamma)
    rbfs = torch.exp(-(d - mu).pow(2) * inv_gamma.pow(2))
    srbfs = rbfs.sum(dim=-1, keepdim=True)
    kernels = rbfs / (1e-6 + srbfs)
    if not derivative:
        return kernels, None
    drbfs = -2 * (d - mu) * inv_gamma.pow(2) * rbfs
    sdrbfs = drbfs.sum(dim=-1, keepdim=True)
    return kernels, drbfs / (1e-6 + srbfs) - rbfs * sdrbfs / (1e-6 + srbfs ** 2)


def _time_value(t):
    """the time as a host float (a python number costs nothing; a device tensor is read back)"""
    return float(t)


class _KernelDynamicsFn(torch.autograd.Function):
    """(forces [B, n d], divergence [B]) on bgk_kdyn_eval; backward: one launch of bgk_kdyn_eval_backward for g_x and the gradients of
    the time-contracted weights w [K] and offset c, then the chain to the parameters as torch ops on [K, O] tensors"""

    @staticmethod
    def forward(ctx, dyn, t, with_div, x2, weights, bias, importance, nlg_time):
        from . import _lib
        B, dev = x2.shape[0], x2.device
        forces = torch.empty_like(x2)
        div = torch.empty(B, dtype=torch.float32, device=dev) if with_div else None
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_kdyn_eval(_lib.ptr(x2), B, *dyn._launch_args(), t, _lib.ptr(forces), _lib.ptr(div), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_kdyn_eval")
        ctx.save_for_backward(x2, weights, bias, importance, nlg_time)
        ctx.cfg = (dyn, t)
        if not with_div:
            div = forces.new_zeros(0)
            ctx.mark_non_differentiable(div)
        return forces, div

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_forces, g_div):
        from . import _lib
        dyn, t = ctx.cfg
        x2, weights, bias, importance, nlg_time = ctx.saved_tensors
        B, dev, K = x2.shape[0], x2.device, dyn._n_kernels
        gf = g_forces.to(torch.float32).contiguous()
        gd = g_div.to(torch.float32).contiguous() if g_div is not None and g_div.numel() == B else None
        gx = torch.empty_like(x2)
        nblk = 1024
        partial = torch.empty((nblk, K + 1), dtype=torch.float32, device=dev)
        gwc = torch.empty(K + 1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_kdyn_eval_backward(_lib.ptr(x2), B, *dyn._launch_args(), t, _lib.ptr(gf), _lib.ptr(gd), _lib.ptr(gx),
                                                   _lib.ptr(partial), nblk, _lib.ptr(gwc), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_kdyn_eval_backward")
        grads = [None] * 4
        need = ctx.needs_input_grad[4:8]
        if any(need):
            with torch.enable_grad():
                params = [p.detach().requires_grad_(n) for p, n in zip((weights, bias, importance, nlg_time), need)]
                w, c = dyn._contract(t, *params)
                wanted = [p for p, n in zip(params, need) if n]
                got = iter(torch.autograd.grad([w, c], wanted, [gwc[:K], gwc[K]], allow_unused=True))
            grads = [next(got) if n else None for n in need]
        return (None, None, None, gx if ctx.needs_input_grad[3] else None, *grads)


class KernelDynamics(torch.nn.Module):
    """Equivariant dynamics with an exact divergence (kernel_dynamic.py:6-116): particle i moves along sum_{j != i} (x_i - x_j) F(d_ij, t),
    F a combination of normalised radial basis functions of the distance d_ij = sqrt(|x_i - x_j|^2 + 1e-6), modulated by normalised
    radial basis functions of the time.  ``forward(t, x)`` returns ``(forces, -divergence [B, 1])``.

    ``mus_time=None``: no time modulation (the reference cannot be constructed that way)."""

    def __init__(self, n_particles, n_dimensions, mus, gammas, mus_time=None, gammas_time=None, optimize_d_gammas=False, optimize_t_gammas=False):
        super().__init__()
        self._n_particles = n_particles
        self._n_dimensions = n_dimensions
        mus = torch.as_tensor(mus)
        neg_log_gammas = -torch.log(torch.as_tensor(gammas, dtype=mus.dtype)) * torch.ones_like(mus)
        self._n_kernels = mus.shape[0]
        self.register_buffer("_mus", mus)
        if optimize_d_gammas:
            self._neg_log_gammas = torch.nn.Parameter(neg_log_gammas)
        else:
            self.register_buffer("_neg_log_gammas", neg_log_gammas)
        if mus_time is None:
            self._n_out = 1
            self._mus_time = None
            self._neg_log_gammas_time = None
        else:
            mus_time = torch.as_tensor(mus_time)
            assert gammas_time is not None, "time kernels need their widths gammas_time"
            nlg_time = -torch.log(torch.as_tensor(gammas_time, dtype=mus_time.dtype)) * torch.ones_like(mus_time)
            assert nlg_time.shape[0] == mus_time.shape[0]
            self._n_out = mus_time.shape[0]
            self.register_buffer("_mus_time", mus_time)
            if optimize_t_gammas:
                self._neg_log_gammas_time = torch.nn.Parameter(nlg_time)
            else:
                self.register_buffer("_neg_log_gammas_time", nlg_time)
        self._weights = torch.nn.Parameter(torch.Tensor(self._n_kernels, self._n_out).normal_() * np.sqrt(1. / self._n_kernels))
        self._bias = torch.nn.Parameter(torch.Tensor(1, self._n_out).zero_())
        self._importance = torch.nn.Parameter(torch.Tensor(self._n_kernels).zero_())

    # ---- torch formulas (any device, any dtype) ----

    def _force_mag(self, t, d, derivative=False):
        rbfs, d_rbfs = _rbf_kernels(d, self._mus, self._neg_log_gammas, derivative=derivative)
        force_mag = (rbfs + self._importance.pow(2).view(1, 1, 1, -1)) @ self._weights + self._bias
        d_force_mag = d_rbfs @ self._weights if derivative else None
        if self._mus_time is not None:
            trbfs, _ = _rbf_kernels(t, self._mus_time, self._neg_log_gammas_time)
            force_mag = (force_mag * trbfs).sum(dim=-1, keepdim=True)
            if derivative:
                d_force_mag = (d_force_mag * trbfs).sum(dim=-1, keepdim=True)
        return force_mag, d_force_mag

    def _forward_torch(self, t, x, compute_divergence=True):
        """the reference's op chain (kernel_dynamic.py:100-116): [B, n, n - 1, d] distance vectors, [B, n, n - 1, K] kernels"""
        n_batch, n = x.shape[0], self._n_particles
        x = x.reshape(n_batch, n, self._n_dimensions)
        t = torch.as_tensor(t, dtype=x.dtype, device=x.device)
        r = x.unsqueeze(2) - x.unsqueeze(1)
        off = ~torch.eye(n, dtype=torch.bool, device=x.device)
        r = r[:, off].view(n_batch, n, n - 1, self._n_dimensions)
        d = (r.pow(2).sum(dim=-1) + 1e-6).sqrt().unsqueeze(-1)
        force_mag, d_force_mag = self._force_mag(t, d, derivative=compute_divergence)
        forces = (r * force_mag).sum(dim=-2).view(n_batch, -1)
        if not compute_divergence:
            return forces
        divergence = (d * d_force_mag + self._n_dimensions * force_mag).view(n_batch, -1).sum(dim=-1)
        return forces, -divergence.unsqueeze(-1)

    def _contract(self, t, weights, bias, importance, nlg_time):
        """w_k(t) = sum_o W_ko tau_o and c(t) = sum_k importance_k^2 w_k + sum_o b_o tau_o: what the kernels form per launch"""
        if self._mus_time is None:
            tau = torch.ones(1, dtype=weights.dtype, device=weights.device)
        else:
            tau = _rbf_kernels(torch.as_tensor(t, dtype=weights.dtype, device=weights.device), self._mus_time, nlg_time)[0]
        w = weights @ tau
        return w, (importance.pow(2) * w).sum() + (bias.reshape(-1) * tau).sum()

    # ---- kernel path ----

    def _launch_args(self):
        from . import _lib
        return (self._n_particles, self._n_dimensions, self._n_kernels, self._n_out, _lib.ptr(self._mus), _lib.ptr(self._neg_log_gammas),
                _lib.ptr(self._weights), _lib.ptr(self._bias), _lib.ptr(self._importance), _lib.ptr(self._mus_time),
                _lib.ptr(self._neg_log_gammas_time))

    def _kernel_rows(self, x):
        """the [B, n d] view of x if the kernels take it (and every parameter is theirs), else None"""
        n, d = self._n_particles, self._n_dimensions
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (2, 3) and x.shape[0] > 0):
            return None
        if x.numel() != x.shape[0] * n * d:
            return None
        if not (2 <= n <= KDYN_MAX_PARTICLES and 1 <= d <= KDYN_MAX_DIMS and 1 <= self._n_kernels <= KDYN_MAX_KERNELS
                and self._n_out <= KDYN_MAX_TIME_KERNELS):
            return None
        tensors = [self._mus, self._neg_log_gammas, self._weights, self._bias, self._importance]
        if self._mus_time is not None:
            tensors += [self._mus_time, self._neg_log_gammas_time]
        if not all(p.device == x.device and p.dtype == torch.float32 and p.is_contiguous() for p in tensors):
            return None
        if torch.is_grad_enabled() and self._neg_log_gammas.requires_grad:      # the distance bandwidths have no kernel-side gradient
            return None
        return x.view(x.shape[0], n * d)

    def forward(self, t, x, compute_divergence=True):
        x2 = self._kernel_rows(x)
        if x2 is None or (torch.is_tensor(t) and t.requires_grad):
            return self._forward_torch(t, x, compute_divergence)
        nlg_time = self._neg_log_gammas_time if self._mus_time is not None else self._bias.new_zeros(0)
        forces, div = _KernelDynamicsFn.apply(self, _time_value(t), bool(compute_divergence), x2, self._weights, self._bias, self._importance,
                                              nlg_time)
        return (forces, -div[:, None]) if compute_divergence else forces


class DensityDynamics(torch.nn.Module):
    """(t, (*xs, logp)) -> (*dxs, divergence): the instantaneous change of variables (dynamics/density.py:4-38)"""

    def __init__(self, dynamics):
        super().__init__()
        self._dynamics = dynamics
        self._n_evals = 0

    def forward(self, t, state):
        *dxs, dlogp = self._dynamics(t, *state[:-1])
        return (*dxs, -dlogp)


class InversedDynamics(torch.nn.Module):
    """the dynamics of the inverse flow: -f(t_max - t, .) (dynamics/inversed.py:4-34)"""

    def __init__(self, dynamics, t_max=1.0):
        super().__init__()
        self._dynamics = dynamics
        self._t_max = t_max

    def forward(self, t, state):
        *dxs, dlogp = self._dynamics(self._t_max - t, state)
        return [-dx for dx in dxs] + [-dlogp]


def integrate_fixed(dynamics, state, t_max, n_steps, method):
    """``n_steps`` steps h = t_max / n_steps of classical RK4 (stages at t, t + h/2, t + h/2, t + h) or explicit Euler of
    d state / dt = dynamics(t, state) over a tuple of tensors, every component with the same tableau"""
    h = t_max / n_steps
    state = tuple(state)
    for step in range(n_steps):
        t = step * h
        if method == "euler":
            k1 = dynamics(t, state)
            state = tuple(y + h * a for y, a in zip(state, k1))
            continue
        k1 = dynamics(t, state)
        k2 = dynamics(t + 0.5 * h, tuple(y + (0.5 * h) * a for y, a in zip(state, k1)))
        k3 = dynamics(t + 0.5 * h, tuple(y + (0.5 * h) * a for y, a in zip(state, k2)))
        k4 = dynamics(t + h, tuple(y + h * a for y, a in zip(state, k3)))
        state = tuple(y + (h / 6.0) * (a + 2.0 * b + 2.0 * c + e) for y, a, b, c, e in zip(state, k1, k2, k3, k4))
    return state


class DiffEqFlow(Flow):
    """Continuous normalising flow (nn/flow/diffeq.py:11-96) in its fixed-step mode: ``use_checkpoints=True`` with the options ``Nt``
    (steps, default 10) and ``method`` ("RK4" or "Euler") as keywords.  Without grad, a ``KernelDynamics`` inside the kernel's envelope
    is integrated by ONE launch of bgk_kdyn_integrate; under grad the same tableau is composed from ``dynamics.forward`` calls (the
    backward kernel of ``KernelDynamics`` trains); any other dynamics module ``forward(t, x) -> (dx, -divergence)`` is composed likewise.
    ``use_checkpoints=False`` (adaptive solvers with adjoint gradients) needs torchdiffeq and is not provided."""

    def __init__(self, dynamics, integrator="dopri5", atol=1e-10, rtol=1e-5, n_time_steps=2, t_max=1., use_checkpoints=False, **kwargs):
        super().__init__()
        self._dynamics = DensityDynamics(dynamics)
        self._inverse_dynamics = DensityDynamics(InversedDynamics(dynamics, t_max))
        self._integrator_method = integrator
        self._integrator_atol = atol
        self._integrator_rtol = rtol
        self._n_time_steps = n_time_steps
        self._t_max = t_max
        self._use_checkpoints = use_checkpoints
        self._kwargs = kwargs

    def _forward(self, *xs, **kwargs):
        return self._run_ode(*xs, inverse=False, **kwargs)

    def _inverse(self, *xs, **kwargs):
        return self._run_ode(*xs, inverse=True, **kwargs)

    def _run_ode(self, *xs, inverse, temperature=None, **kwargs):
        if not self._use_checkpoints:
            raise NotImplementedError(
                "DiffEqFlow(use_checkpoints=False) integrates with torchdiffeq's adaptive solvers, which this package does not provide; "
                "use the fixed-step mode: DiffEqFlow(dynamics, use_checkpoints=True, Nt=<steps>, method='RK4' or 'Euler')")
        options = {**self._kwargs, **{k: v for k, v in kwargs.items() if not k.startswith("_bgk")}}
        n_steps, method = int(options.get("Nt", 10)), str(options.get("method", "RK4")).lower()
        if method not in _METHODS or n_steps < 1:
            raise ValueError(f"DiffEqFlow: fixed-step options Nt={options.get('Nt')}, method={options.get('method')!r} (RK4 or Euler)")
        assert all(x.shape[0] == xs[0].shape[0] for x in xs[1:])
        inner = self._dynamics._dynamics
        if len(xs) == 1 and isinstance(inner, KernelDynamics) and not (torch.is_grad_enabled() and (
                xs[0].requires_grad or any(p.requires_grad for p in inner.parameters()))):
            x2 = inner._kernel_rows(xs[0])
            if x2 is not None:
                return self._integrate_kernel(inner, xs[0], x2, n_steps, method, inverse)
        logp = torch.zeros(xs[0].shape[0], 1).to(xs[0])
        dynamics = self._inverse_dynamics if inverse else self._dynamics
        *ys, dlogp = integrate_fixed(dynamics, (*xs, logp), float(self._t_max), n_steps, method)
        return (*ys, dlogp)

    def _integrate_kernel(self, dyn, x, x2, n_steps, method, inverse):
        from . import _lib
        B, dev = x2.shape[0], x2.device
        y = torch.empty_like(x2)
        dlogp = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_kdyn_integrate(_lib.ptr(x2), B, *dyn._launch_args(), float(self._t_max), n_steps, _METHODS[method],
                                               int(bool(inverse)), _lib.ptr(y), _lib.ptr(dlogp), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_kdyn_integrate")
        return y.view(x.shape), dlogp[:, None]
