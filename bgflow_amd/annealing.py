"""Annealed switching between two energies with the nonequilibrium work of every chain: ``InterpolatedEnergy``, ``AnnealedSwitching``,
``annealed_importance_sampling`` and ``jarzynski_free_energy``.  Not in the reference.  The work of a forward protocol and of its
``reverse()`` is what ``bennett_acceptance_ratio`` consumes; annealed importance sampling (AIS) from a prior A to a target B is the forward
protocol from samples of A, with the log weight ``-work`` per chain.  ``stochastic.AnnealedMCFlow`` is the same protocol as a flow layer.

Definitions (both paths; csrc/bgk_anneal.hip states them again for the kernel):

  ends          two energies A and B over the same tensor; their temperatures ``temperature_a`` and ``temperature_b`` are positive numbers
  schedule      ``lambdas = [l_0, ..., l_M]``, each in [0, 1], M >= 1; monotonicity is not required
  coefficients  stage m has cA_m = (1 - l_m) / T_A and cB_m = l_m / T_B, formed on the host in f64 and rounded to f32 once
                (``anneal_coefficients``); both paths compute with the rounded values
  reduced energy  u_m(x) = cA_m e_A(x) + cB_m e_B(x), e_A and e_B the raw energies at temperature 1 (on the fused path the f32 energies
                the lane carries, bit for bit what ``energy.energy`` returns for the row).  A coefficient that is exactly 0 drops its
                term: 0 * inf would be a NaN and freeze the chain
  protocol      global steps s = 0 .. M K - 1, K = ``n_steps`` per stage, stage m = s // K + 1.  At the first step of a stage, first the
                work increment of the current state, W += (cA_m - cA_{m-1}) e_A + (cB_m - cB_{m-1}) e_B, in f64 (a difference that is
                exactly 0 drops its term, for the same reason); then the Metropolis step at u_m: x' = x + noise_std xi_s, accepted iff
                -(u_m(x') - u_m(x)) >= log r_s -- false for a NaN on either side.  Steps are taken at every stage, the last included
  results       the final state, ``work`` (f64 [B]), ``e_a`` / ``e_b`` of the final state, per-chain ``n_accepted`` and ``n_proposed``.
                The AIS log weight of a chain is ``-work``

The general path runs this in torch ops for any ``Energy``, device and dtype.  The fused path (csrc/bgk_anneal.hip, entries
bgk_pair_anneal / bgk_box_anneal) runs a whole protocol in one launch -- in launches of at most ``ANNEAL_MAX_STEPS_PER_LAUNCH`` steps, the
same bits however it is split -- when both ends give ``PairPlan``s of equal (n, d) or ``BoxPlan``s of equal n, x is one contiguous f32
HIP tensor [B, n d] or [B, n, d] with B > 0 that needs no grad, and ``noise_std``, the temperatures and the schedule are numbers.
``fused = True`` (the default) takes the kernel only where it was measured faster than the general path, tiles of the full 64 rows
(n d <= 123, ``ANNEAL_FUSED_MIN_ROWS``); ``fused = "always"`` takes it wherever it applies, ``fused = False`` never.
"""
import math

import torch

from .distributions import BoxPlan, Energy, PairPlan, _FusedSampling, _kernel_plan
from .particles import _check_tensors, _target_args
from .sampling import _chain_launch_checks, mcmc_tile_rows

__all__ = ["InterpolatedEnergy", "AnnealedSwitching", "annealed_importance_sampling", "jarzynski_free_energy", "anneal_coefficients",
           "anneal_fused_by_default", "pair_anneal", "ANNEAL_MAX_STEPS_PER_LAUNCH", "ANNEAL_FUSED_MIN_ROWS"]

# The most annealed Metropolis steps one launch of bgk_pair_anneal runs; longer protocols are split (bitwise the same chains: the random
# stream, the carried f32 energies and the f64 work do not depend on the split), so that no single launch holds a shared GPU for long.
# The start value is ``sampling.MCMC_MAX_STEPS_PER_LAUNCH // 2``: a step evaluates two row energies, at most twice the Metropolis step
# measured at 1.10 ms (Lennard-Jones, n = 64, d = 3, 2^16 chains), so 112 steps are about 0.25 s.  Measured on an MI355X
# (tools/anneal_time.py, its last lines): at that shape, mean-free normal -> Lennard-Jones, one launch of 32 steps takes 35.21 ms
# (35.01 .. 35.88 over three rounds), 1.100 ms per step, next to 1.058 ms per Metropolis step of bgk_pair_mcmc on the same chains
# (33.85 ms for 32 steps): the second end costs 4 % there, because the mean-free normal has no pair term.  Two ends WITH pair terms at
# that shape (Lennard-Jones -> double wells) were not timed; at twice the pair work they stay within the factor 2 the start value
# assumes, so the constant stays at 112: 0.123 s as measured, at most about 0.25 s with two pair ends.
ANNEAL_MAX_STEPS_PER_LAUNCH = 112

# The tile height from which ``fused = True`` takes the kernel (``anneal_fused_by_default``): the lowest at which it was measured
# faster than the general path -- in fact the full height: every measured shape with 64 rows per tile (n d <= 123) is faster, the
# shapes with fewer are slower or level.  tools/anneal_time.py on an MI355X, 2^16 chains, in-kernel Philox, ms per step fused (kernel
# forced) / general (both ends' energy kernels per proposal and the accept chain in torch ops), mean-free normal -> Lennard-Jones:
# n = 13 (64 rows) 0.026 / 0.190; n = 26 (64) 0.077 / 0.236; n = 32 (64) 0.188 / 0.238; n = 41 (64) 0.287 / 0.302; n = 48 (54 rows)
# 0.532 / 0.373; n = 56 (46 rows) 0.709 / 0.719; n = 64 (41 rows) 1.082 / 0.784.  The particle box of 38 -> its ``biased_system``
# (64 rows): 0.151 / 0.247.  Below 64 rows fewer chains are in flight per CU while a lane still walks all pairs alone, and the
# general path's energy kernels keep one tile per chain.  Not measured: ends that both have pair terms, boxes of other sizes.
ANNEAL_FUSED_MIN_ROWS = 64


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def anneal_coefficients(lambdas, temperature_a=1.0, temperature_b=1.0):
    """the table [M + 1, 2] (f32, CPU) of the stages' coefficients (cA_m, cB_m) = ((1 - l_m) / T_A, l_m / T_B): formed in f64, rounded once"""
    lam = torch.tensor([float(v) for v in lambdas], dtype=torch.float64)
    return torch.stack([(1.0 - lam) / float(temperature_a), lam / float(temperature_b)], dim=1).to(torch.float32)


def _reduced(c_a, c_b, e_a, e_b):
    """c_a e_a + c_b e_b; a coefficient that is exactly 0 drops its term"""
    u = c_a * e_a if c_a != 0 else torch.zeros_like(e_a)
    return u + c_b * e_b if c_b != 0 else u + torch.zeros_like(e_b)


class InterpolatedEnergy(Energy):
    """u(x) = (1 - lam) / T_A e_A(x) + lam / T_B e_B(x), the reduced energy of a stage (module docstring), as an ``Energy``: a target of
    ``MCMCStep`` or ``HMCStep`` at temperature 1, and the building block of the general path.  ``lam`` is a plain attribute."""

    def __init__(self, energy_a, energy_b, lam=0.0, temperature_a=1.0, temperature_b=1.0):
        super().__init__(energy_a.event_shapes)
        if [tuple(s) for s in energy_a.event_shapes] != [tuple(s) for s in energy_b.event_shapes]:
            raise ValueError("InterpolatedEnergy: both ends must have the same event shapes")
        if not (_is_number(temperature_a) and temperature_a > 0 and _is_number(temperature_b) and temperature_b > 0):
            raise ValueError("InterpolatedEnergy: the temperatures must be positive numbers")
        self.energy_a, self.energy_b = energy_a, energy_b
        self.lam = lam
        self.temperature_a, self.temperature_b = temperature_a, temperature_b

    def _energy(self, *xs, **kwargs):
        c = anneal_coefficients([self.lam], self.temperature_a, self.temperature_b)[0].tolist()
        return _reduced(c[0], c[1], self.energy_a.energy(*xs, **kwargs), self.energy_b.energy(*xs, **kwargs))


def pair_anneal(plan_a, plan_b, x, schedule, n_steps, step_begin, step_end, noise_std, e_a, e_b, e_valid, work, noise=None, uniforms=None,
                seed=0, offset=0, row0=0, n_accepted=None, accumulate=False):
    """One launch of bgk_pair_anneal (bgk_box_anneal for two ``BoxPlan``s): the global steps [step_begin, step_end) of the protocol of
    ``schedule`` (f32 [M + 1, 2] on the device, ``anneal_coefficients``) with ``n_steps`` steps per stage on the chains x [B, n d] (f32,
    contiguous, HIP; updated IN PLACE).  e_a, e_b [B]: raw energies of the ends, read if ``e_valid``, written for the final state; work [B]
    (f64) and n_accepted [B] (int32): written, or continued with ``accumulate``.  noise [M n_steps, B, n d] and uniforms [M n_steps, B]
    (row s for step s, whatever the launch), or neither (Philox numbers of (seed, offset + s, chain row0 + b))."""
    from . import _lib
    B, nd = x.shape
    box = isinstance(plan_a, BoxPlan)
    if box != isinstance(plan_b, BoxPlan) or plan_a.n_particles != plan_b.n_particles or plan_a.n_dims != plan_b.n_dims:
        raise ValueError("pair_anneal: both ends must be pair targets of equal (n, d) or boxes of equal n")
    if schedule.dim() != 2 or schedule.shape[0] < 2 or schedule.shape[1] != 2:
        raise ValueError("pair_anneal: schedule [M + 1, 2], M >= 1")
    M, K = schedule.shape[0] - 1, int(n_steps)
    if K < 1 or not 0 <= step_begin <= step_end <= M * K:
        raise ValueError(f"pair_anneal: steps [{step_begin}, {step_end}) of {M} stages of {K} steps")
    _chain_launch_checks("pair_anneal", plan_a, x, None, noise, uniforms, M * K, n_accepted,
                         [(schedule, (M + 1, 2)), (e_a, (B,)), (e_b, (B,))], noun="targets")
    _check_tensors("pair_anneal", x, [(work, (B,))], dtype=torch.float64)
    if box:
        name = "bgk_box_anneal"
        ends = (plan_a.n_particles, *_target_args(plan_a)[1:], *_target_args(plan_b)[1:])
    else:
        name = "bgk_pair_anneal"
        ends = (plan_a.n_particles, plan_a.n_dims, *_target_args(plan_a)[2:], *_target_args(plan_b)[2:])
    with torch.cuda.device(x.device):
        st = getattr(_lib.lib(), name)(_lib.ptr(x), B, *ends, _lib.ptr(schedule), M, K, int(step_begin), int(step_end), float(noise_std),
                                       _lib.ptr(noise), _lib.ptr(uniforms), int(seed) & (2 ** 64 - 1), int(offset) & 0xffffffff, int(row0),
                                       _lib.ptr(e_a), _lib.ptr(e_b), int(bool(e_valid)), _lib.ptr(work), _lib.ptr(n_accepted),
                                       int(bool(accumulate)), _lib.stream_ptr(x.device))
    _lib.check(st, name)


def anneal_fused_by_default(plan_a, plan_b):
    """whether ``fused = True`` takes the kernel for these ends: where tools/anneal_time.py measured it faster than the general path,
    tiles of at least ``ANNEAL_FUSED_MIN_ROWS`` rows (its comment has the numbers).  ``fused = "always"`` takes the kernel wherever it
    accepts the state."""
    return mcmc_tile_rows(plan_a.n_particles * plan_a.n_dims) >= ANNEAL_FUSED_MIN_ROWS


class AnnealedSwitching(_FusedSampling):
    """The protocol of the module docstring from ``energy_a`` (lambda = 0) to ``energy_b`` (lambda = 1): ``forward(x)`` returns
    ``(x_final, work)``, work f64 [B]; the raw energies of the final state are kept as ``.e_a`` / ``.e_b`` ([B]), the accepted steps per
    chain of this run as ``n_accepted`` (int32 [B]) and its steps as ``n_proposed``.  ``reverse()`` is the mirrored protocol: ends
    swapped, schedule reversed.

    Conventions of ``MCMCStep``: ``fused`` (True: the kernel where it applies and was measured faster, ``anneal_fused_by_default``;
    "always": wherever it applies; False: the general path), ``feed_noise(noise [S, B, n d], uniforms [S, B])`` -- a run consumes M K rows of
    either, on both paths --, ``chain_offset`` (the global index of the batch's first chain) and ``set_philox_stream``; the Philox counter is
    the index of the next step.  Without fed numbers the general path draws ``torch.randn_like(x)`` and ``torch.rand_like(u)`` once per step."""
    fused = True

    def __init__(self, energy_a, energy_b, lambdas, n_steps=1, noise_std=0.1, temperature_a=1.0, temperature_b=1.0):
        super().__init__()
        lambdas = [float(v) for v in (lambdas.tolist() if torch.is_tensor(lambdas) else lambdas)]
        if len(lambdas) < 2 or not all(0.0 <= v <= 1.0 for v in lambdas):
            raise ValueError("AnnealedSwitching: lambdas must be at least two numbers in [0, 1]")
        if not (isinstance(n_steps, int) and not isinstance(n_steps, bool) and n_steps >= 1):
            raise ValueError("AnnealedSwitching: n_steps must be an integer, at least 1")
        for t in (temperature_a, temperature_b):
            if not (_is_number(t) and t > 0 and math.isfinite(t)):
                raise ValueError("AnnealedSwitching: the temperatures must be positive numbers")
        if _is_number(noise_std) and not noise_std >= 0:
            raise ValueError("AnnealedSwitching: noise_std must not be negative")
        self.energy_a, self.energy_b = energy_a, energy_b
        self.lambdas = lambdas
        self.n_steps = n_steps
        self.noise_std = noise_std
        self.temperature_a, self.temperature_b = temperature_a, temperature_b
        self.schedule = anneal_coefficients(lambdas, temperature_a, temperature_b)
        self.chain_offset = 0
        self.n_accepted = None
        self.n_proposed = 0
        self.e_a = self.e_b = None
        self.e_a_start = None          # raw e_A of the start state of the last run, where it was computed (``_run(..., start=True)``)
        self._fed = None

    @property
    def n_stages(self):
        return len(self.lambdas) - 1

    def reverse(self):
        """the mirrored protocol, from ``energy_b`` back to ``energy_a``: lambdas 1 - l_M, ..., 1 - l_0 between the swapped ends"""
        out = AnnealedSwitching(self.energy_b, self.energy_a, [1.0 - v for v in reversed(self.lambdas)], n_steps=self.n_steps,
                                noise_std=self.noise_std, temperature_a=self.temperature_b, temperature_b=self.temperature_a)
        if "fused" in self.__dict__:
            out.fused = self.fused
        return out

    def feed_noise(self, noise, uniforms):
        """explicit random numbers for the next runs instead of the random stream: noise [S, B, n d] standard normals and uniforms [S, B]
        (fused path: f32, on the samples' device); a run consumes M K rows of either; ``feed_noise(None, None)`` returns to the stream"""
        if noise is None and uniforms is None:
            self._fed = None
            return self
        if noise is None or uniforms is None or noise.dim() != 3 or uniforms.dim() != 2 or uniforms.shape != noise.shape[:2]:
            raise ValueError("feed_noise: noise [S, B, n d] and uniforms [S, B]")
        self._fed = [noise.contiguous(), uniforms.contiguous(), 0]
        return self

    def _take_fed(self, x, total):
        fed = self._fed
        if fed is None:
            return None, None
        B = x.shape[0]
        if fed[0].shape[0] - fed[2] < total or fed[0].shape[1] != B or fed[0].shape[2] != x[0].numel():
            raise ValueError(f"AnnealedSwitching: {total} steps of {tuple(x.shape)} chains need as many rows of fed noise; "
                             f"{fed[0].shape[0] - fed[2]} rows of {tuple(fed[0].shape[1:])} are left")
        pos, fed[2] = fed[2], fed[2] + total
        return fed[0][pos:pos + total], fed[1][pos:pos + total]

    # -- the fused path
    def _fused_setup(self, x):
        """(plan_a, plan_b) if the kernel takes this input, else None"""
        if not self.fused or not (_is_number(self.noise_std) and self.noise_std >= 0 and math.isfinite(self.noise_std)):
            return None
        plan_a, plan_b = _kernel_plan(self.energy_a, 1.0), _kernel_plan(self.energy_b, 1.0)
        if not ((isinstance(plan_a, PairPlan) and isinstance(plan_b, PairPlan)) or (isinstance(plan_a, BoxPlan) and isinstance(plan_b, BoxPlan))):
            return None
        if plan_a.n_particles != plan_b.n_particles or plan_a.n_dims != plan_b.n_dims:
            return None
        if self.fused != "always" and not anneal_fused_by_default(plan_a, plan_b):
            return None                # measured slower than the general path, or not measured
        nd = plan_a.n_particles * plan_a.n_dims
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (2, 3) and x.shape[0] > 0):
            return None
        if tuple(x.shape[1:]) not in ((nd,), (plan_a.n_particles, plan_a.n_dims)):
            return None
        if torch.is_grad_enabled() and x.requires_grad:
            return None
        return plan_a, plan_b

    def _fused_run(self, x, setup, start):
        from . import particles
        plan_a, plan_b = setup
        B, K, total = x.shape[0], self.n_steps, self.n_stages * self.n_steps
        dev = x.device
        noise, unif = self._take_fed(x, total)
        if noise is not None:
            if noise.device != dev or noise.dtype != torch.float32 or unif.dtype != torch.float32:
                raise ValueError("AnnealedSwitching: the fused path takes fed f32 numbers on the samples' device")
            seed = offset = 0
        else:
            from . import dp
            st = self._philox_ids()
            seed = (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1)
            offset, st[1] = st[1], st[1] + total
        hit = self.__dict__.get("_schedule_dev")
        if hit is None or hit[0] != dev:
            hit = self.__dict__["_schedule_dev"] = (dev, self.schedule.to(dev).contiguous())
        y = x.detach().clone().view(B, -1)
        e_valid = False
        if start:                      # the caller wants e_A of the start state: both ends' energy kernels, whose bits the chain kernel carries on
            e_a = particles.pair_energy(plan_a, (y,))[:, 0].contiguous()
            e_b = particles.pair_energy(plan_b, (y,))[:, 0].contiguous()
            self.e_a_start, e_valid = e_a.clone(), True
        else:
            e_a, e_b = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
            self.e_a_start = None
        work = torch.empty(B, dtype=torch.float64, device=dev)
        acc = torch.empty(B, dtype=torch.int32, device=dev)
        cap = max(1, int(ANNEAL_MAX_STEPS_PER_LAUNCH))
        for begin in range(0, total, cap):
            pair_anneal(plan_a, plan_b, y, hit[1], K, begin, min(total, begin + cap), self.noise_std, e_a, e_b, e_valid or begin > 0, work,
                        noise, unif, seed, offset, self.chain_offset, acc, accumulate=begin > 0)
        self.e_a, self.e_b, self.n_accepted, self.n_proposed = e_a, e_b, acc, total
        return y.view(x.shape), work

    # -- the general path
    def _energies(self, x):
        B = x.shape[0]
        return self.energy_a.energy(x).reshape(B), self.energy_b.energy(x).reshape(B)

    def _general_run(self, x):
        B, K, M = x.shape[0], self.n_steps, self.n_stages
        noise, unif = self._take_fed(x, M * K)
        table = self.schedule.tolist()
        e_a, e_b = self._energies(x)
        self.e_a_start = e_a
        work = torch.zeros(B, dtype=torch.float64, device=x.device)
        acc = torch.zeros(B, dtype=torch.int32, device=x.device)
        batch = (B,) + (1,) * (x.dim() - 1)
        s = 0
        for m in range(1, M + 1):
            (c_a, c_b), (p_a, p_b) = table[m], table[m - 1]
            work = work + _reduced(c_a - p_a, c_b - p_b, e_a.to(torch.float64), e_b.to(torch.float64))
            for _ in range(K):
                xi = torch.randn_like(x) if noise is None else noise[s].to(device=x.device, dtype=x.dtype).reshape(x.shape)
                xp = x + self.noise_std * xi
                q_a, q_b = self._energies(xp)
                u, up = _reduced(c_a, c_b, e_a, e_b), _reduced(c_a, c_b, q_a, q_b)
                r = torch.rand_like(u) if unif is None else unif[s].to(device=u.device, dtype=u.dtype)
                accept = -(up - u) >= r.log()                       # false for a NaN on either side
                x = torch.where(accept.reshape(batch), xp, x)
                e_a, e_b = torch.where(accept, q_a, e_a), torch.where(accept, q_b, e_b)
                acc = acc + accept.to(torch.int32)
                s += 1
        self.e_a, self.e_b, self.n_accepted, self.n_proposed = e_a, e_b, acc, M * K
        return x, work

    def _run(self, x, start=False):
        """``forward``; with ``start`` the raw e_A of the start state is kept as ``e_a_start`` on either path"""
        setup = self._fused_setup(x)
        if setup is not None:
            return self._fused_run(x, setup, start)
        return self._general_run(x)

    def forward(self, x):
        return self._run(x)


def annealed_importance_sampling(prior, target, n_samples_or_x0, lambdas, n_steps=1, noise_std=0.1, temperature_prior=1.0,
                                 temperature_target=1.0, fused=True):
    """Annealed importance sampling from ``prior`` (energy A) to ``target`` (energy B): ``(x, log_weights)`` with ``log_weights = -work`` of
    the forward protocol (f64 [B]).  ``n_samples_or_x0``: a number of chains, drawn with ``prior.sample``, or the start states themselves.
    The mean of exp(log_weights) estimates Z_B / Z_A (``jarzynski_free_energy(-log_weights)`` its negative logarithm)."""
    x0 = n_samples_or_x0 if torch.is_tensor(n_samples_or_x0) else prior.sample(int(n_samples_or_x0))
    switching = AnnealedSwitching(prior, target, lambdas, n_steps=n_steps, noise_std=noise_std, temperature_a=temperature_prior,
                                  temperature_b=temperature_target)
    switching.fused = fused
    x, work = switching(x0)
    return x, -work


def jarzynski_free_energy(work):
    """the Jarzynski estimate of the reduced free-energy difference f_B - f_A = -log mean exp(-W) = -logsumexp(-W) + log N from the work
    values of a forward protocol (any shape; computed in f64)"""
    w = work.reshape(-1).to(torch.float64)
    return -torch.logsumexp(-w, dim=0) + math.log(w.numel())
