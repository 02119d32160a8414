"""``MixtureDistribution`` (bgflow/distribution/mixture.py:12-47): a weighted mixture of distributions over one tensor, the standard
multimodal toy target and the usual multimodal prior.

The general path is the reference's formulas in torch ops -- any components, device, dtype, twice differentiable.  A mixture of this
package's ``NormalDistribution`` components (f32, no ``cov`` or a diagonal one, at most ``MIXTURE_MAX_COMPONENTS`` of width at most
``MIXTURE_MAX_WIDTH``) evaluated on a 2-d f32 HIP tensor runs on csrc/bgk_mixture.hip instead: one launch for the energy (optionally
with the KL integrand's sums, so ``KLTrainer`` keeps its fused loss path), one for the gradients of x and of the log-weights, one for
``sample_fused=True`` sampling with the sample's energy.  The kernel's arithmetic is defined in the header comment of that file.
"""
import numpy as np
import torch

from .distributions import (MIXTURE_MAX_COMPONENTS, MIXTURE_MAX_WIDTH, PHILOX_MAX_WIDTH, Energy, MixturePlan, NormalDistribution, Sampler,
                            _FusedSampling, _kernel_plan, _own_methods, kernel_energy)
from .utils import assert_numpy

__all__ = ["MixtureDistribution"]

_MAX_BLOCKS = 2048            # block partials of the two-stage reductions (loss sums, log-weight gradient)


def _is_number(t):
    return isinstance(t, (int, float)) and not isinstance(t, bool)


def _launch_energy(plan, tables, x, ld, logw, neg_e=None, dlogp=None, drop_nonfinite=False, want_sums=False):
    """one launch of bgk_mixture_energy on the rows of x (row stride ld): u [B] (and the f64 loss sums [2])"""
    from . import _lib
    B, dev = x.shape[0], x.device
    u = torch.empty(B, dtype=torch.float32, device=dev)
    partial = sums = None
    if want_sums:
        partial = torch.empty((_MAX_BLOCKS, 2), dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_mixture_energy(_lib.ptr(x), ld, B, plan.n_components, plan.dim, *[_lib.ptr(t) for t in tables], _lib.ptr(logw),
                                           float(plan.temperature), _lib.ptr(u), _lib.ptr(neg_e), _lib.ptr(dlogp), int(bool(drop_nonfinite)),
                                           _lib.ptr(partial), _MAX_BLOCKS, _lib.ptr(sums), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_mixture_energy")
    return u, sums


def _launch_backward(plan, tables, x, ld, logw, u, g_u, g_scalar, dlogp, drop_nonfinite, want_gx, want_gdl, want_gw):
    """one launch of bgk_mixture_energy_backward (+ the fixed-order merge of the log-weight gradient): (g_x, g_dlogp, g_logw)"""
    from . import _lib
    B, dev, K = x.shape[0], x.device, plan.n_components
    gx = torch.empty((B, plan.dim), dtype=torch.float32, device=dev) if want_gx else None
    g_dl = torch.empty(B, dtype=torch.float32, device=dev) if want_gdl else None
    gw = wpartial = None
    if want_gw:
        gw = torch.empty(K, dtype=torch.float32, device=dev)
        wpartial = torch.empty((_MAX_BLOCKS, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_mixture_energy_backward(_lib.ptr(x), ld, B, K, plan.dim, *[_lib.ptr(t) for t in tables], _lib.ptr(logw),
                                                    float(plan.temperature), _lib.ptr(u), _lib.ptr(g_u), _lib.ptr(g_scalar), _lib.ptr(dlogp),
                                                    int(bool(drop_nonfinite)), _lib.ptr(g_dl), _lib.ptr(gx), plan.dim, _lib.ptr(gw),
                                                    _lib.ptr(wpartial), _MAX_BLOCKS, _lib.stream_ptr(dev))
    _lib.check(st, "bgk_mixture_energy_backward")
    return gx, g_dl, gw


class _MixtureEnergyFn(torch.autograd.Function):
    """u = -logsumexp_k(-E_k(x) + logw_k) / T on bgk_mixture_energy; the gradients of x and of the log-weights are one launch of
    bgk_mixture_energy_backward"""

    @staticmethod
    def forward(ctx, plan, tables, x, logw):
        from . import _lib
        x2, ld = _lib.rowmajor(x)
        lw = logw.detach().contiguous()
        u, _ = _launch_energy(plan, tables, x2, ld, lw)
        ctx.save_for_backward(x2, lw, u)
        ctx.cfg = (plan, tables, ld)
        return u[:, None]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_u):
        plan, tables, ld = ctx.cfg
        x2, lw, u = ctx.saved_tensors
        g = g_u.reshape(-1).to(torch.float32).contiguous()
        gx, _, gw = _launch_backward(plan, tables, x2, ld, lw, u, g, None, None, False, ctx.needs_input_grad[2], False, ctx.needs_input_grad[3])
        return None, None, gx, gw


class _MixtureKLSumsFn(torch.autograd.Function):
    """[sum_b (u(x_b) - dlogp_b), number of samples kept] (f64 [2]) with the partial sums formed by the mixture kernel itself; backward:
    one launch for the gradients of x, dlogp and the log-weights"""

    @staticmethod
    def forward(ctx, plan, tables, drop_nonfinite, dlogp, x, logw):
        from . import _lib
        x2, ld = _lib.rowmajor(x)
        lw = logw.detach().contiguous()
        dl = dlogp.detach().reshape(-1).to(torch.float32).contiguous()
        u, sums = _launch_energy(plan, tables, x2, ld, lw, dlogp=dl, drop_nonfinite=drop_nonfinite, want_sums=True)
        ctx.save_for_backward(x2, lw, u, dl)
        ctx.cfg = (plan, tables, ld, bool(drop_nonfinite), dlogp.shape)
        u2 = u[:, None]
        ctx.mark_non_differentiable(u2)
        return sums, u2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sums, _g_u):
        plan, tables, ld, drop, dl_shape = ctx.cfg
        x2, lw, u, dl = ctx.saved_tensors
        gs = g_sums[0:1].to(torch.float32).contiguous()
        gx, g_dl, gw = _launch_backward(plan, tables, x2, ld, lw, u, None, gs, dl, drop, ctx.needs_input_grad[4], ctx.needs_input_grad[3],
                                        ctx.needs_input_grad[5])
        return None, None, None, None if g_dl is None else g_dl.reshape(dl_shape), gx, gw


def _kernel_operands(plan, xs):
    """(x, tables, live log-weights) if the mixture kernel takes this input, else None"""
    if len(xs) != 1 or not torch.is_tensor(xs[0]):
        return None
    x, dist = xs[0], plan.dist
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == plan.dim and x.shape[0] > 0):
        return None
    w = dist._unnormed_log_weights
    if w.device != x.device or w.dtype != torch.float32:
        return None
    tables = dist._device_tables(x.device)
    return None if tables is None else (x, tables, dist._log_weights)


def mixture_energy(plan, xs):
    """the [B, 1] energy of a MixturePlan on bgk_mixture_energy, or None if the input is not the kernel's"""
    ops = _kernel_operands(plan, xs)
    return None if ops is None else _MixtureEnergyFn.apply(plan, ops[1], ops[0], ops[2])


def mixture_kl_loss_sums(plan, xs, dlogp, drop_nonfinite=False):
    """(sums, u) of distributions.kl_loss_sums for a MixturePlan, or None"""
    ops = _kernel_operands(plan, xs)
    if ops is None or not (torch.is_tensor(dlogp) and dlogp.is_cuda and dlogp.numel() == xs[0].shape[0]):
        return None
    return _MixtureKLSumsFn.apply(plan, ops[1], bool(drop_nonfinite), dlogp, ops[0], ops[2])


class MixtureDistribution(Energy, Sampler, _FusedSampling):
    """Mixture of ``components`` (equal ``dim``) with weights ``softmax(unnormed_log_weights)`` (distribution/mixture.py:12-47):
    ``_energy(x) = -logsumexp_k(-E_k(x) + log w_k)`` of shape [B, 1]; ``energy(x, temperature)`` divides that by the temperature
    (energy/base.py:124-146) -- it is NOT the tempered mixture.  ``sample(n)`` draws ``np.random.multinomial(n, w)`` counts and
    concatenates ``c.sample(n_k)`` in component order; a temperature other than 1.0 raises ``NotImplementedError`` like the reference.

    With ``NormalDistribution`` components (f32; no ``cov`` or a diagonal one) the energy of a 2-d f32 HIP tensor, its gradients (to x and,
    with ``trainable_weights``, to the log-weights) and the KL loss sums run on csrc/bgk_mixture.hip, without a host read.
    ``fused``: True or "always" (the kernel wherever it applies: it was measured faster at every shape, DESIGN.md "Gaussian mixture"),
    False (the torch formulas).

    ``sample_fused=True`` (not in the reference; buffers on a HIP device, ``dim <= PHILOX_MAX_WIDTH``): component, sample and the
    sample's energy come from one launch of the counter-based generator.  The rows are then i.i.d. draws -- NOT grouped by component as
    the reference's concatenation returns them -- which is why it is opt-in.  The components drawn last are kept as
    ``last_assignments`` (int32 [n])."""
    fused = True

    def __init__(self, components, unnormed_log_weights=None, trainable_weights=False, sample_fused=False):
        assert all([c.dim == components[0].dim for c in components]), "All mixture components must have the same dimensionality."
        super().__init__(components[0].dim)
        self._components = torch.nn.ModuleList(components)
        if unnormed_log_weights is None:
            unnormed_log_weights = torch.zeros(len(components))
        else:
            assert len(unnormed_log_weights.shape) == 1, "Mixture weights must be a Tensor of shape `[n_components]`."
            assert len(unnormed_log_weights) == len(components), "Number of mixture weights does not match number of components."
        if trainable_weights:
            self._unnormed_log_weights = torch.nn.Parameter(unnormed_log_weights)
        else:
            self.register_buffer("_unnormed_log_weights", unnormed_log_weights)
        self.sample_fused = sample_fused
        self.last_assignments = None

    @property
    def _log_weights(self):
        return torch.log_softmax(self._unnormed_log_weights, dim=-1)

    # ---- general path (the reference's formulas) ----
    def _energy(self, x):
        energies = torch.stack([c.energy(x) for c in self._components], dim=-1)
        return -torch.logsumexp(-energies + self._log_weights.view(1, 1, -1), dim=-1)

    def _sample(self, n_samples):
        if self.sample_fused:
            out = self._sample_kernel(n_samples)
            if out is not None:
                return out
        weights_numpy = assert_numpy(self._log_weights.exp())
        ns = np.random.multinomial(n_samples, weights_numpy, 1)[0]
        samples = [c.sample(n) for n, c in zip(ns, self._components)]
        return torch.cat(samples, dim=0)

    def _log_assignments(self, x):
        """-E_k(x) stacked on the last axis, [B, 1, K], without the weights"""
        if not (torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad):
            plan = _kernel_plan(self, 1.0)
            ops = _kernel_operands(plan, (x,)) if isinstance(plan, MixturePlan) else None
            if ops is not None:
                from . import _lib
                x2, ld = _lib.rowmajor(x)
                neg_e = torch.empty((x.shape[0], plan.n_components), dtype=torch.float32, device=x.device)
                _launch_energy(plan, ops[1], x2, ld, ops[2].detach().contiguous(), neg_e=neg_e)
                return neg_e[:, None, :]
        energies = torch.stack([c.energy(x) for c in self._components], dim=-1)
        return -energies

    # ---- the kernel path ----
    def _host_tables(self):
        """(mu [K, d], h [K, d], logz [K]) as f32 host arrays if every component is a kernel normal, else None; rebuilt only when a
        component's buffers change (the check of ``_rot`` reads it on the host)"""
        comps = list(self._components)
        K, d = len(comps), self.dim
        if not (1 <= K <= MIXTURE_MAX_COMPONENTS and 1 <= d <= MIXTURE_MAX_WIDTH):
            return None
        if not all(isinstance(c, NormalDistribution) and _own_methods(c, NormalDistribution) for c in comps):
            return None
        key = tuple((id(c), c._mean.data_ptr(), c._mean._version, c._mean.dtype) +
                    ((c._log_diag.data_ptr(), c._log_diag._version, c._rot.data_ptr(), c._rot._version) if c._has_cov else ()) for c in comps)
        hit = self.__dict__.get("_mix_tables")
        if hit is not None and hit[0] == key:
            return hit[1]
        host = self._build_tables(comps, K, d)
        self.__dict__["_mix_tables"] = (key, host, {})
        return host

    @staticmethod
    def _build_tables(comps, K, d):
        mu = np.zeros((K, d), np.float32)
        h = np.ones((K, d), np.float64)
        logz = np.full(K, d / 2 * np.log(2 * np.pi), np.float64)
        for k, c in enumerate(comps):
            if c._mean.dtype != torch.float32:
                return None
            mu[k] = c._mean.detach().cpu().numpy()
            if not c._has_cov:
                continue
            # a diagonal covariance: eigh's rotation is a signed permutation -- exactly one entry of magnitude 1 per row and column.
            # energy: ((x - mean) @ rot)_i^2 exp(-log_diag_i), so input column j = the row of column i's entry has h_j = exp(-log_diag_i)
            rot = np.abs(c._rot.detach().cpu().numpy().astype(np.float64))
            if not (((rot == 0) | (rot == 1)).all() and (rot.sum(0) == 1).all() and (rot.sum(1) == 1).all()):
                return None
            log_diag = c._log_diag.detach().cpu().numpy().reshape(-1).astype(np.float64)       # (the stored + 1e-6 included)
            h[k, rot.argmax(axis=0)] = np.exp(-log_diag)
            logz[k] += 0.5 * log_diag.sum()
        return mu, h.astype(np.float32), logz.astype(np.float32)

    def _device_tables(self, device):
        host = self._host_tables()
        if host is None:
            return None
        cache = self.__dict__["_mix_tables"][2]
        if device not in cache:
            cache[device] = tuple(torch.from_numpy(t).to(device) for t in host)
        return cache[device]

    def _mixture_kernel(self, temperature=1.0):
        """the MixturePlan of this mixture at ``temperature``, or None (then the torch formulas run)"""
        if self.fused is False or not (_is_number(temperature) and temperature > 0):
            return None
        if self._unnormed_log_weights.dtype != torch.float32 or self._host_tables() is None:
            return None
        return MixturePlan(self, len(self._components), self.dim, float(temperature))

    def energy(self, x, temperature=1.0):
        cached = self._fused_energy((x,), temperature) if _is_number(temperature) else None
        if cached is not None:
            return cached
        fast = kernel_energy(self, (x,), temperature) if torch.is_tensor(x) and x.dim() == 2 else None
        if fast is not None:
            return fast
        return super().energy(x, temperature=temperature)

    def _sample_kernel(self, n_samples):
        """component, sample and the sample's energy from bgk_mixture_sample, or None"""
        from . import _lib
        w = self._unnormed_log_weights
        if not (w.is_cuda and w.dtype == torch.float32 and self.dim <= PHILOX_MAX_WIDTH):
            return None
        if not isinstance(_kernel_plan(self, 1.0), MixturePlan):        # (a subclass with its own energy: the cached energy would not be its)
            return None
        tables = self._device_tables(w.device)
        dev, K, d = w.device, len(self._components), self.dim
        x = torch.empty((n_samples, d), dtype=torch.float32, device=dev)
        assign = torch.empty(n_samples, dtype=torch.int32, device=dev)
        energy = torch.empty(n_samples, dtype=torch.float32, device=dev)
        seed, off = self._philox_next()
        if n_samples > 0:
            logw = self._log_weights.detach().contiguous()
            with torch.cuda.device(dev):
                status = _lib.lib().bgk_mixture_sample(seed, off & 0xffffffff, 0, n_samples, K, d, *[_lib.ptr(t) for t in tables], _lib.ptr(logw),
                                                       _lib.ptr(x), d, _lib.ptr(assign), _lib.ptr(energy), _lib.stream_ptr(dev))
            _lib.check(status, "bgk_mixture_sample")
        self._philox_remember([x], 1.0, energy[:, None])
        self.last_assignments = assign
        return x
