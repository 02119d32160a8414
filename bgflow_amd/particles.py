"""Many-particle targets and their prior (csrc/bgk_pair.hip): ``LennardJonesPotential`` (bgflow/distribution/energy/lennard_jones.py:14-72),
``MultiDoubleWellPotential`` (energy/multi_double_well_potential.py:7-43) and ``MeanFreeNormalDistribution`` (distribution/normal.py:253-283)
with the reference's constructor signatures, attribute names and ``two_event_dims`` semantics (event shape [n, d] by default, [dim] otherwise).

``energy()`` of a contiguous f32 HIP tensor of 2..64 particles in 1..3 dimensions at a scalar temperature is one launch of
bgk_pair_energy (one more for the gradient); every other input -- f64, CPU, non-contiguous, more particles, a tensor-valued
temperature -- is evaluated by ``_energy``, the same formulas as torch ops.  ``distributions.kl_loss_sums`` forms the KL loss sums of
such a target inside the energy launch (``BoltzmannGenerator.kldiv_mean`` / ``KLTrainer`` keep their fused loss path).

The particle box -- ``RepulsiveParticles`` and ``HarmonicParticles`` (bgflow/distribution/energy/particles.py:51-381): a bistable dimer in a
bath of repulsive solvent particles in a 2-d box -- runs on the same kernels through the bgk_box_* entries under a ``BoxPlan``
(2..64 particles); ``force`` of a kernel input is one backward launch.
"""
import ctypes

import numpy as np
import torch

from .distributions import BoxPlan, Energy, PairPlan, Sampler

__all__ = ["LennardJonesPotential", "MultiDoubleWellPotential", "MeanFreeNormalDistribution", "RepulsiveParticles", "HarmonicParticles"]

PAIR_MAX_PARTICLES, PAIR_MAX_DIMS = 64, 3         # the kernel's envelope (csrc/bgk_pair.hip)


def _is_number(*values):
    return all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in values)


def _check_tensors(name, like, tensors, dtype=torch.float32):
    """the argument check of the launch wrappers: every (tensor or None, shape) pair is a contiguous ``dtype`` tensor of that shape on
    the device of ``like``"""
    for t, shape in tensors:
        if t is None:
            continue
        if not (t.is_cuda and t.device == like.device and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{name}: expected a contiguous {dtype} HIP tensor of shape {shape}, got {t.dtype} {tuple(t.shape)} on {t.device}")


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


def _box_params(plan):
    """the host parameter array of the bgk_box_* entries"""
    return (ctypes.c_float * len(plan.params))(*plan.params)


def _entry(plan, name):
    """the C entry ``name`` of the plan's family: bgk_pair_<name> or, for a BoxPlan, bgk_box_<name>"""
    from . import _lib
    full = ("bgk_box_" if isinstance(plan, BoxPlan) else "bgk_pair_") + name
    return getattr(_lib.lib(), full), full


def _target_args(plan):
    """the target in a C entry's argument list, after B: of the bgk_box_* entries for a BoxPlan, else of the bgk_pair_* entries"""
    if isinstance(plan, BoxPlan):
        return (plan.n_particles, plan.kind, _box_params(plan), len(plan.params))
    return (plan.n_particles, plan.n_dims, plan.kind, plan.p0, plan.p1, plan.p2, plan.p3, plan.osc_scale)


def _launch_args(plan, x2):
    from . import _lib
    return (_lib.ptr(x2), x2.shape[1], x2.shape[0], *_target_args(plan), plan.temperature)


def _energy_backward(plan, x2, g):
    """g[b] (d e / d x)(x2[b]) / T: one launch of bgk_pair_energy_backward / bgk_box_energy_backward; g: f32 [B], contiguous"""
    from . import _lib
    gx = torch.empty_like(x2)
    with torch.cuda.device(x2.device):
        fn, name = _entry(plan, "energy_backward")
        st = fn(*_launch_args(plan, x2), _lib.ptr(g), None, None, None, 0, None, _lib.ptr(gx), gx.shape[1], _lib.stream_ptr(x2.device))
    _lib.check(st, name)
    return gx


class _PairEnergyFn(torch.autograd.Function):
    """u = e(x) / T on bgk_pair_energy (bgk_box_energy for a BoxPlan); the gradient is one launch of the entry's _backward"""

    @staticmethod
    def forward(ctx, plan, x2):
        from . import _lib
        u = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        with torch.cuda.device(x2.device):
            fn, name = _entry(plan, "energy")
            st = fn(*_launch_args(plan, x2), _lib.ptr(u), _lib.stream_ptr(x2.device))
        _lib.check(st, name)
        ctx.save_for_backward(x2)
        ctx.plan = plan
        return u[:, None]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_u):
        (x2,) = ctx.saved_tensors
        return None, _energy_backward(ctx.plan, x2, g_u.reshape(-1).to(torch.float32).contiguous())


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
            fn, name = _entry(plan, "energy_kl_sums")
            st = fn(*_launch_args(plan, x2), _lib.ptr(u), _lib.ptr(dl), int(bool(drop_nonfinite)), _lib.ptr(partial), nblk,
                    _lib.ptr(sums), _lib.stream_ptr(dev))
        _lib.check(st, name)
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
            fn, name = _entry(plan, "energy_backward")
            st = fn(*_launch_args(plan, x2), None, _lib.ptr(gs), _lib.ptr(u), _lib.ptr(dl), int(drop), _lib.ptr(g_dl), _lib.ptr(gx),
                    gx.shape[1], _lib.stream_ptr(x2.device))
        _lib.check(st, name)
        return None, None, None if g_dl is None else g_dl.reshape(dl_shape), gx


def pair_energy(plan, xs):
    """the [B, 1] energy of a PairPlan on bgk_pair_energy (a BoxPlan: bgk_box_energy), or None if the input is not the kernel's"""
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
    """(sums, u) of distributions.kl_loss_sums for a PairPlan or a BoxPlan, or None"""
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
        if not (_is_number(temperature, osc_scale, *p) and temperature > 0 and 2 <= n <= PAIR_MAX_PARTICLES and 1 <= d <= PAIR_MAX_DIMS):
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


# ---- the particle box ---------------------------------------------------------------------------------------------------------------
def _where_sqrt(keep, d2):
    """sqrt(d2) where ``keep``, else 0, with a finite (zero) derivative of every order where it is dropped"""
    return torch.where(keep, torch.where(keep, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))


class RepulsiveParticles(Energy):
    """A bistable dimer (particles 0 and 1) in a bath of ``nsolvent`` purely repulsive particles in a 2-d box with soft walls
    (bgflow/distribution/energy/particles.py:51-344); a sample is the row [x0, y0, x1, y1, ...] of ``dim = 2 (nsolvent + 2)`` numbers:

        eps sum (rm^2 / d_ij^2)^6 over the pairs i < j except (0, 1)  (the reference's 0.5 sum over both orders under ``mask_matrix``)
        + dimer_k (x0 + x1)^2 + dimer_k y0^2 + dimer_k y1^2 + dimer_slope t - dimer_a t^2 + dimer_b t^4,  t = 2 (|r0 - r1| - dimer_dmid)
        + (sign(delta) + 1) box_k delta^2 for every coordinate c and delta = -(c + box_halfsize), c - box_halfsize

    ``energy`` of a contiguous f32 HIP [B, dim] tensor of 2..64 particles at a scalar temperature is one launch of bgk_box_energy, its
    gradient one of bgk_box_energy_backward, and ``force`` of such a tensor is that one backward launch; every other input runs the torch
    formulas, which sum over the pairs i < j and take roots only of terms that are kept: the reference's values, with finite first and
    second derivatives.

    Deviations from the reference:
      * ``RepulsiveParticles()`` uses ``params_default`` (the reference reads ``params["nsolvent"]`` before its ``None`` check: TypeError);
      * ``box_force_torch`` reshapes to ``self.dim`` (the reference: to a hard-coded 76);
      * ``forward``, ``hamiltonian``, ``surrogate_hamiltonian``, ``force_autograd`` and ``plot_dimer_energy`` call methods that the
        reference does not have (``energy_torch``, ``dimer_energy``) and are left out;
      * ``LJ_energy_surrogate_torch`` is the reference's for ``rc < 1`` (its masked entries, shifted to D2 + 1, then stay above the cutoff);
      * ``grid_k`` is unused, as in the reference."""

    params_default = {
        "nsolvent": 36,
        "eps": 1.0,            # prefactor of the repulsion
        "rm": 1.1,             # particle size
        "dimer_slope": -1,     # dimer: linear term
        "dimer_a": 25.0,       # dimer: quadratic term
        "dimer_b": 10.0,       # dimer: quartic term
        "dimer_dmid": 1.5,     # dimer: distance of the transition state
        "dimer_k": 20.0,       # dimer: force constant of the restraints
        "box_halfsize": 3.0,
        "box_k": 100.0,        # force constant of the walls
        "grid_k": 0.0,         # unused
        "rc": 0.9,             # cutoff of the surrogate and of the harmonic repulsion
    }

    _box_kind = 3

    def __init__(self, params=None):
        if params is None:
            params = self.__class__.params_default
        self.nparticles = params["nsolvent"] + 2
        super().__init__(2 * self.nparticles)
        self.params = params
        self.rm = self.params["rm"]
        self.rm12 = self.params["rm"] ** 12
        self.a_surrogate = 21.0 * self.params["rm"] ** 6 / self.params["rc"] ** 8
        self.b_surrogate = 6.0 * self.params["rm"] ** 6 / self.params["rc"] ** 7
        self.c_surrogate = self.params["rm"] ** 6 / self.params["rc"] ** 6
        # 1 for the pairs that interact: not a particle with itself, not the two dimer particles
        self.mask_matrix = np.ones((self.nparticles, self.nparticles), dtype=np.float32)
        self.mask_matrix[0, 1] = 0.0
        self.mask_matrix[1, 0] = 0.0
        for i in range(self.nparticles):
            self.mask_matrix[i, i] = 0.0
        self.mask_matrix_torch = torch.from_numpy(self.mask_matrix)

    # -- the kernel plan
    def _spring(self):
        return 0.0

    def _pair_kernel(self, temperature=1.0):
        p = self.params
        names = ("eps", "rm", "rc", "dimer_slope", "dimer_a", "dimer_b", "dimer_dmid", "dimer_k", "box_halfsize", "box_k")
        spring = self._spring()
        if not (_is_number(temperature, spring, *(p[k] for k in names)) and temperature > 0 and isinstance(self.nparticles, int)
                and 2 <= self.nparticles <= PAIR_MAX_PARTICLES):
            return None
        values = (p["eps"], p["rm"] ** 2, p["rc"], p["rc"] ** 2, spring, p["dimer_slope"], p["dimer_a"], p["dimer_b"], p["dimer_dmid"],
                  p["dimer_k"], p["box_halfsize"], p["box_k"])
        return BoxPlan(self._box_kind, self.nparticles, tuple(float(v) for v in values), float(temperature))

    def energy(self, *xs, temperature=1.0, **kwargs):
        if not kwargs:
            from .distributions import kernel_energy
            fast = kernel_energy(self, xs, temperature)
            if fast is not None:
                return fast
        return super().energy(*xs, temperature=temperature, **kwargs)

    # -- the terms as torch ops
    def dimer_distance(self, x):
        sqrt = torch.sqrt if torch.is_tensor(x) else np.sqrt
        return sqrt((x[:, 2] - x[:, 0]) ** 2 + (x[:, 3] - x[:, 1]) ** 2)

    def _pairs(self, x):
        """(i, j, x [B, n, 2], d2 [B, pairs]) of the interacting pairs i < j in ascending order: all but the dimer's (0, 1), the first"""
        x = x.reshape(x.shape[0], self.nparticles, 2)
        n = self.nparticles
        i, j = torch.triu_indices(n, n, offset=1, device=x.device)
        i, j = i[1:], j[1:]
        return i, j, x, (x[:, i] - x[:, j]).pow(2).sum(dim=-1)

    def LJ_energy_torch(self, x):
        d2 = self._pairs(x)[3]
        return self.params["eps"] * ((self.params["rm"] ** 2) / d2).pow(6).sum(dim=-1)

    def LJ_energy_surrogate_torch(self, x):
        """the repulsion beyond ``rc``, a parabola that continues it below (not scaled by eps, as in the reference)"""
        d2 = self._pairs(x)[3]
        rc = self.params["rc"]
        far = d2 > rc ** 2
        t = _where_sqrt(~far, d2) - rc
        e_h = self.a_surrogate * t ** 2 - self.b_surrogate * t + self.c_surrogate
        e_lj = self.params["eps"] * ((self.params["rm"] ** 2) / torch.where(far, d2, torch.ones_like(d2))).pow(6)
        return torch.where(far, e_lj, e_h).sum(dim=-1)

    def LJ_force_torch(self, x):
        i, j, xp, d2 = self._pairs(x)
        pair = (12 * self.params["eps"] * self.rm12 / d2.pow(7))[..., None] * (xp[:, i] - xp[:, j])
        f = torch.zeros_like(xp).index_add_(1, i, pair).index_add_(1, j, -pair)
        return f.reshape(x.shape[0], self.dim)

    def dimer_energy_torch(self, x):
        k = self.params["dimer_k"]
        d = torch.sqrt((x[:, 0] - x[:, 2]) ** 2 + (x[:, 1] - x[:, 3]) ** 2)
        t = 2 * (d - self.params["dimer_dmid"])
        t2 = t * t
        restraint = k * (x[:, 0] + x[:, 2]) ** 2 + (k * x[:, 1] ** 2 + k * x[:, 3] ** 2)
        return restraint + (self.params["dimer_slope"] * t - self.params["dimer_a"] * t2 + self.params["dimer_b"] * (t2 * t2))

    def dimer_force_torch(self, x):
        k = self.params["dimer_k"]
        f = torch.zeros_like(x)
        f[:, 0] = f[:, 2] = -2 * k * (x[:, 0] + x[:, 2])
        f[:, 1] = -2 * k * x[:, 1]
        f[:, 3] = -2 * k * x[:, 3]
        d = x[:, :2] - x[:, 2:4]
        r = d.pow(2).sum(dim=1).sqrt()
        t = 2 * (r - self.params["dimer_dmid"])
        pull = (-2 * self.params["dimer_slope"] + 4 * self.params["dimer_a"] * t - 8 * self.params["dimer_b"] * t ** 3)[:, None] * (d / r[:, None])
        f[:, :2] += pull
        f[:, 2:4] -= pull
        return f

    def _wall_depths(self, x):
        """how far every coordinate is beyond the lower and the upper wall (negative inside): two [B, dim] tensors"""
        h = self.params["box_halfsize"]
        return -(x + h), x - h

    def box_energy_torch(self, x):
        k = self.params["box_k"]
        return sum(((torch.sign(d) + 1) * k * d ** 2).sum(dim=1) for d in self._wall_depths(x))

    def box_force_torch(self, x):
        k = self.params["box_k"]
        lo, hi = self._wall_depths(x)
        return (2 * (torch.sign(lo) + 1) * k * lo - 2 * (torch.sign(hi) + 1) * k * hi).reshape(-1, self.dim)

    def _energy(self, x):
        return (self.LJ_energy_torch(x) + self.dimer_energy_torch(x) + self.box_energy_torch(x)).view(-1, 1)

    def surrogate_energy(self, x):
        return self.LJ_energy_surrogate_torch(x) + self.box_energy_torch(x) + self.dimer_energy_torch(x)

    def _kernel_force(self, x):
        """-d e / d x of a kernel input as ONE launch of bgk_box_energy_backward (g_u = -1), else None"""
        from .distributions import _kernel_plan
        plan = _kernel_plan(self, 1.0)
        if not isinstance(plan, BoxPlan) or not torch.is_tensor(x) or x.dim() != 2:
            return None
        x2 = _pair_rows(plan, (x.detach(),))
        if x2 is None:
            return None
        return _energy_backward(plan, x2, torch.full((x2.shape[0],), -1.0, dtype=torch.float32, device=x2.device))

    def _torch_force(self, x):
        return self.LJ_force_torch(x) + self.dimer_force_torch(x) + self.box_force_torch(x)

    def force(self, x):
        fast = self._kernel_force(x)
        return fast if fast is not None else self._torch_force(x)


class HarmonicParticles(RepulsiveParticles):
    """The particle box with a cut-off harmonic repulsion in place of the r^-12 one (bgflow/distribution/energy/particles.py:347-381):
    spring_constant sum (d_ij - rc)^2 over the pairs i < j except (0, 1) with d_ij < rc, plus the dimer and box terms.

    Deviations from the reference, beside those of ``RepulsiveParticles``: the reference takes the root of its whole [B, n, n] matrix,
    zero diagonal included, so its autograd gradient is NaN in every entry; here the root is taken of the kept pairs only, the gradient is
    finite and a pair at distance 0 contributes the gradient 0.  ``force`` is minus the gradient of THIS energy (the reference inherits
    the repulsive class's analytic force, which belongs to another pair term)."""

    _box_kind = 4

    def __init__(self, spring_constant=200.0, params=None):
        if params is None:
            params = RepulsiveParticles.params_default
        super().__init__(params)
        self.spring_constant = spring_constant

    def _spring(self):
        return self.spring_constant

    def _pair_kernel(self, temperature=1.0):
        # NOT dead code: distributions._kernel_plan hands out a plan only while ``energy`` / ``_energy`` are those of the class that
        # DEFINES ``_pair_kernel``.  This class overrides ``_energy`` (kind 4 computes that one), so it has to define the plan too;
        # without this method every harmonic target would silently take the torch path.  (tests/test_host_box.py asserts the BoxPlan.)
        return super()._pair_kernel(temperature)

    def harmonic_energy_torch(self, x):
        d2 = self._pairs(x)[3]
        rc = self.params["rc"]
        close = d2 < rc ** 2
        t = _where_sqrt(close & (d2 > 0), d2) - rc
        return self.spring_constant * torch.where(close, t ** 2, torch.zeros_like(d2)).sum(dim=-1)

    def _energy(self, x):
        return (self.harmonic_energy_torch(x) + self.dimer_energy_torch(x) + self.box_energy_torch(x)).view(-1, 1)

    def _torch_force(self, x):
        with torch.enable_grad():
            xg = x.detach().requires_grad_(True)
            return -torch.autograd.grad(self._energy(xg).sum(), xg)[0]
