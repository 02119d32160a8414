"""Many-particle targets and their prior (csrc/bgk_pair.hip): ``LennardJonesPotential`` (bgflow/distribution/energy/lennard_jones.py:14-72),
``MultiDoubleWellPotential`` (energy/multi_double_well_potential.py:7-43) and ``MeanFreeNormalDistribution`` (distribution/normal.py:253-283)
with the reference's constructor signatures, attribute names and ``two_event_dims`` semantics (event shape [n, d] by default, [dim] otherwise).

``energy()`` of a contiguous f32 HIP tensor of 2..64 particles in 1..3 dimensions at a scalar temperature is one launch of
bgk_pair_energy (one more for the gradient); every other input -- f64, CPU, non-contiguous, more particles, a tensor-valued
temperature -- is evaluated by ``_energy``, the same formulas as torch ops.  ``distributions.kl_loss_sums`` forms the KL loss sums of
such a target inside the energy launch (``BoltzmannGenerator.kldiv_mean`` / ``KLTrainer`` keep their fused loss path).
"""
import torch

from .distributions import Energy, PairPlan, Sampler

__all__ = ["LennardJonesPotential", "MultiDoubleWellPotential", "MeanFreeNormalDistribution"]

PAIR_MAX_PARTICLES, PAIR_MAX_DIMS = 64, 3         # the kernel's envelope (csrc/bgk_pair.hip)


def _number(*values):
    return all(isinstance(v, (int, float)) for v in values)


def _pair_rows(plan, xs):
    """the [B, n d] view of the one input tensor if the kernel takes it, else None"""
    if len(xs) != 1 or not torch.is_tensor(xs[0]):
        return None
    x, nd = xs[0], plan.n_particles * plan.n_dims
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (2, 3) and x.shape[0] > 0):
        return None
    if tuple(x.shape[1:]) not in ((nd,), (plan.n_particles, plan.n_dims)):
        return None
    return x.view(x.shape[0], nd)


def _launch_args(plan, x2):
    from . import _lib
    return (_lib.ptr(x2), x2.shape[1], x2.shape[0], plan.n_particles, plan.n_dims, plan.kind, plan.p0, plan.p1, plan.p2, plan.p3,
            plan.osc_scale, plan.temperature)


class _PairEnergyFn(torch.autograd.Function):
    """u = e(x) / T on bgk_pair_energy; the gradient is one launch of bgk_pair_energy_backward"""

    @staticmethod
    def forward(ctx, plan, x2):
        from . import _lib
        u = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        with torch.cuda.device(x2.device):
            st = _lib.lib().bgk_pair_energy(*_launch_args(plan, x2), _lib.ptr(u), _lib.stream_ptr(x2.device))
        _lib.check(st, "bgk_pair_energy")
        ctx.save_for_backward(x2)
        ctx.plan = plan
        return u[:, None]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_u):
        from . import _lib
        (x2,) = ctx.saved_tensors
        g = g_u.reshape(-1).to(torch.float32).contiguous()
        gx = torch.empty_like(x2)
        with torch.cuda.device(x2.device):
            st = _lib.lib().bgk_pair_energy_backward(*_launch_args(ctx.plan, x2), _lib.ptr(g), None, None, None, 0, None, _lib.ptr(gx),
                                                     gx.shape[1], _lib.stream_ptr(x2.device))
        _lib.check(st, "bgk_pair_energy_backward")
        return None, gx


class _PairKLSumsFn(torch.autograd.Function):
    """[sum_b (u(x_b) - dlogp_b), number of samples kept] (f64 [2]) with the partial sums formed by the pair kernel itself;
    backward: one launch for the gradients of x and dlogp"""

    @staticmethod
    def forward(ctx, plan, drop_nonfinite, dlogp, x2):
        from . import _lib
        B, dev = x2.shape[0], x2.device
        u = torch.empty(B, dtype=torch.float32, device=dev)
        dl = dlogp.detach().reshape(-1).to(torch.float32).contiguous()
        nblk = 2048
        partial = torch.empty((nblk, 2), dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_pair_energy_kl_sums(*_launch_args(plan, x2), _lib.ptr(u), _lib.ptr(dl), int(bool(drop_nonfinite)),
                                                    _lib.ptr(partial), nblk, _lib.ptr(sums), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_pair_energy_kl_sums")
        ctx.save_for_backward(u, dl, x2)
        ctx.cfg = (plan, bool(drop_nonfinite), dlogp.shape)
        u2 = u[:, None]
        ctx.mark_non_differentiable(u2)
        return sums, u2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sums, _g_u):
        from . import _lib
        plan, drop, dl_shape = ctx.cfg
        u, dl, x2 = ctx.saved_tensors
        gs = g_sums[0:1].to(torch.float32).contiguous()
        gx = torch.empty_like(x2)                      # (the launch writes both gradients: x is what the flow's backward continues from)
        g_dl = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(x2.device):
            st = _lib.lib().bgk_pair_energy_backward(*_launch_args(plan, x2), None, _lib.ptr(gs), _lib.ptr(u), _lib.ptr(dl), int(drop),
                                                     _lib.ptr(g_dl), _lib.ptr(gx), gx.shape[1], _lib.stream_ptr(x2.device))
        _lib.check(st, "bgk_pair_energy_backward")
        return None, None, None if g_dl is None else g_dl.reshape(dl_shape), gx


def pair_energy(plan, xs):
    """the [B, 1] energy of a PairPlan on bgk_pair_energy, or None if the input is not the kernel's"""
    x2 = _pair_rows(plan, xs)
    return None if x2 is None else _PairEnergyFn.apply(plan, x2)


def pair_energy_hvp(plan, x2, u2):
    """(g, Hu) = (d u / d x, (d^2 u / d x^2) u2) of the PairPlan's energy u = e / T at the rows of x2 [B, n d] on bgk_pair_energy_hvp: one
    pass over the pairs of a sample for both; x2 and u2 contiguous f32 HIP tensors.  A missing kernel is an error, not a fallback."""
    from . import _lib
    nd = plan.n_particles * plan.n_dims
    for t in (x2, u2):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == x2.device and t.dtype == torch.float32 and t.is_contiguous()
                and t.dim() == 2 and t.shape == x2.shape and t.shape[1] == nd):
            raise ValueError(f"pair_energy_hvp: expected two contiguous float32 HIP tensors [B, {nd}]")
    g, hu = torch.empty_like(x2), torch.empty_like(x2)
    with torch.cuda.device(x2.device):
        st = _lib.lib().bgk_pair_energy_hvp(*_launch_args(plan, x2), _lib.ptr(u2), _lib.ptr(g), _lib.ptr(hu), _lib.stream_ptr(x2.device))
    _lib.check(st, "bgk_pair_energy_hvp")
    return g, hu


def pair_kl_loss_sums(plan, xs, dlogp, drop_nonfinite=False):
    """(sums, u) of distributions.kl_loss_sums for a PairPlan, or None"""
    x2 = _pair_rows(plan, xs)
    if x2 is None or not (torch.is_tensor(dlogp) and dlogp.is_cuda and dlogp.numel() == x2.shape[0]):
        return None
    return _PairKLSumsFn.apply(plan, bool(drop_nonfinite), dlogp, x2)


def _pair_sq_distances(x):
    """|x_i - x_j|^2 of x [B, n, d] for the pairs i < j in ascending (i, j) order: [B, n (n - 1) / 2]"""
    n = x.shape[1]
    i, j = torch.triu_indices(n, n, offset=1, device=x.device)
    return (x[:, i] - x[:, j]).pow(2).sum(dim=-1)


def _centroid_energy(x):
    """0.5 sum_i |x_i - xbar|^2 of x [B, n, d]: [B]"""
    return 0.5 * (x - x.mean(dim=1, keepdim=True)).pow(2).sum(dim=(1, 2))


class _ParticleEnergy(Energy):
    """event shape [n_particles, dim // n_particles] (``two_event_dims``) or [dim]; ``energy`` on the pair kernel where it applies"""

    def __init__(self, dim, n_particles, two_event_dims):
        super().__init__([n_particles, dim // n_particles] if two_event_dims else dim)

    def _plan(self, temperature, kind, n, d, p, osc_scale):
        if not (_number(temperature, osc_scale, *p) and temperature > 0 and 2 <= n <= PAIR_MAX_PARTICLES and 1 <= d <= PAIR_MAX_DIMS):
            return None
        return PairPlan(kind, n, d, *(float(v) for v in p), float(osc_scale), float(temperature))

    def energy(self, *xs, temperature=1.0, **kwargs):
        if not kwargs:
            from .distributions import kernel_energy
            fast = kernel_energy(self, xs, temperature)
            if fast is not None:
                return fast
        return super().energy(*xs, temperature=temperature, **kwargs)


class LennardJonesPotential(_ParticleEnergy):
    """Lennard-Jones cluster: eps sum_{i<j} [(rm / r)^12 - 2 (rm / r)^6] with r = sqrt(|x_i - x_j|^2 + 1e-6), plus (``oscillator``)
    oscillator_scale 0.5 sum_i |x_i - centroid|^2 (energy/lennard_jones.py:14-72)."""

    def __init__(self, dim, n_particles, eps=1.0, rm=1.0, oscillator=True, oscillator_scale=1., two_event_dims=True):
        super().__init__(dim, n_particles, two_event_dims)
        self._n_particles = n_particles
        self._n_dims = dim // n_particles
        self._eps = eps
        self._rm = rm
        self.oscillator = oscillator
        self._oscillator_scale = oscillator_scale

    def _pair_kernel(self, temperature=1.0):
        osc = self._oscillator_scale if self.oscillator else 0.0
        return self._plan(temperature, 0, self._n_particles, self._n_dims, (self._eps, self._rm, 0.0, 0.0), osc)

    def _energy(self, x):
        x = x.reshape(-1, self._n_particles, self._n_dims)
        q = (self._rm / (_pair_sq_distances(x) + 1e-6).sqrt()) ** 6
        e = self._eps * (q * q - 2 * q).sum(dim=-1)
        if self.oscillator:
            e = e + _centroid_energy(x) * self._oscillator_scale
        return e[:, None]


class MultiDoubleWellPotential(_ParticleEnergy):
    """Pairwise double wells sum_{i<j} [a (d - offset)^4 + b (d - offset)^2 + c], d = |x_i - x_j| (energy/multi_double_well_potential.py:7-43).
    Two coincident particles contribute the gradient 0, as through ``torch.cdist``."""

    def __init__(self, dim, n_particles, a, b, c, offset, two_event_dims=True):
        super().__init__(dim, n_particles, two_event_dims)
        self._dim = dim
        self._n_particles = n_particles
        self._n_dimensions = dim // n_particles
        self._a = a
        self._b = b
        self._c = c
        self._offset = offset

    def _pair_kernel(self, temperature=1.0):
        return self._plan(temperature, 1, self._n_particles, self._n_dimensions, (self._a, self._b, self._c, self._offset), 0.0)

    def _energy(self, x):
        d2 = _pair_sq_distances(x.reshape(-1, self._n_particles, self._n_dimensions))
        apart = d2 > 0
        dist = torch.where(apart, torch.where(apart, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        t = dist - self._offset
        return (self._a * t ** 4 + self._b * t ** 2 + self._c).sum(dim=-1, keepdim=True)


class MeanFreeNormalDistribution(_ParticleEnergy, Sampler):
    """Normal distribution on the mean-free subspace of a particle system: u = 0.5 sum_i |x_i - centroid|^2 / std^2
    (distribution/normal.py:253-283); ``sample`` draws independent normal numbers and removes their centroid."""

    def __init__(self, dim, n_particles, std=1., two_event_dims=True):
        super().__init__(dim, n_particles, two_event_dims)
        self._two_event_dims = two_event_dims
        self._dim = dim
        self._n_particles = n_particles
        self._spacial_dims = dim // n_particles
        self.register_buffer("_std", torch.as_tensor(std))

    def _std_host(self):
        """std as a host float, read back once per state of the buffer (no device-to-host sync per energy call)"""
        s = self._std
        key = (s.data_ptr(), s._version, s.device)
        hit = self.__dict__.get("_std_cache")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_std_cache"] = (key, float(s ** 2) if s.numel() == 1 else None)
        return hit[1]

    def _pair_kernel(self, temperature=1.0):
        var = self._std_host()
        if var is None or not var > 0:
            return None
        return self._plan(temperature, 2, self._n_particles, self._spacial_dims, (0.0, 0.0, 0.0, 0.0), 1.0 / var)

    def _energy(self, x):
        e = _centroid_energy(x.reshape(-1, self._n_particles, self._spacial_dims))
        return (e / self._std ** 2)[:, None]

    def sample(self, n_samples, temperature=1.):
        """independent normal numbers of width std, projected onto the mean-free subspace (``temperature`` is not used, as in the
        reference); no host read of the std buffer"""
        x = torch.randn(n_samples, self._n_particles, self._spacial_dims, dtype=self._std.dtype, device=self._std.device) * self._std
        x = x - x.mean(dim=1, keepdim=True)
        return x if self._two_event_dims else x.reshape(n_samples, self._dim)
