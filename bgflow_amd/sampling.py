"""Iterative samplers: ``SamplerState`` / ``SamplerStep`` / ``IterativeSampler`` (bgflow/distribution/sampling/iterative.py,
_iterative_helpers.py) and Metropolis Monte Carlo -- ``GaussianProposal``, ``LatentProposal``, ``MCMCStep``, ``GaussianMCMCSampler``,
``metropolis_accept`` (sampling/mcmc.py) -- with the reference's constructor signatures, defaults and state bookkeeping.

The general path is the reference's step in torch ops over ``energy.energy(...)``: any ``Energy``, any proposal, any device and dtype.

The fused path (csrc/bgk_mcmc.hip, entries bgk_pair_mcmc / bgk_box_mcmc) runs whole chains in one launch: a particle-system target with a
``PairPlan`` (2..64 particles in 1..3 dimensions) or a ``BoxPlan`` (the particle box: 2..64 particles in 2 dimensions), a plain ``GaussianProposal`` with a numeric ``noise_std``, one contiguous f32 HIP samples tensor
[B, n d] or [B, n, d], no box vectors, the default samples hook, and a positive number or a tensor of B positive values as
``target_temperatures``.  ``MCMCStep.forward`` is then one launch for its ``n_steps``; an ``IterativeSampler`` whose only step is such a
step (and whose ``extract_sample_hook`` is the default) runs ``stride * n_steps`` steps per iteration inside the launch and has the kernel
write every recorded state straight into the ``[n, B, ...]`` result.  ``MCMCStep.fused = False`` forces the general path.

Hamiltonian Monte Carlo (not in the reference outside its OpenMM integrators): ``HamiltonianProposal`` / ``HMCStep`` /
``HamiltonianMCSampler``.  A ``HamiltonianProposal`` on the step's own energy and temperature, with numeric ``step_size`` and ``mass``,
takes the fused path under the same conditions through csrc/bgk_hmc.hip (entries bgk_pair_hmc / bgk_box_hmc): the leapfrog trajectory
and the accept step of every step inside the launch, in launches of at most ``hmc_max_steps_per_launch(n_leapfrog)`` steps.  By
default (``fused = True``) that holds where the kernel was measured faster than the general path -- pair targets of n d <= 79,
``hmc_fused_by_default`` -- and ``fused = "always"`` takes the kernel wherever it accepts the state.

Not in the reference: ``MCMCStep.n_accepted`` (per-chain accepted steps) / ``n_proposed``, ``MCMCStep.feed_noise`` and ``chain_offset``;
``ReplicaExchangeMCMCStep`` / ``ReplicaExchangeSampler`` -- parallel tempering over ladders of temperatures with the exchange rule of the
reference's numpy ``ReplicaExchangeMetropolisGauss`` (_mcmc/metropolis.py:138-188; its numpy port is in umbrella.py), fused as entries
bgk_pair_remc / bgk_box_remc of the same kernel: the exchange is a swap of row index, tile flag and energy between two lanes.

Chains that switch from one target to another and record the nonequilibrium work -- ``AnnealedSwitching``, annealed importance
sampling -- are in annealing.py (csrc/bgk_anneal.hip: the same tile walk and Philox layout with two targets per lane).
"""
import dataclasses
import math
import warnings
from typing import Sequence

import torch

from .distributions import BoxPlan, PairPlan, Sampler, _FusedSampling, _kernel_plan
from .particles import _check_tensors, _target_args
from .utils import pack_tensor_in_list, pack_tensor_in_tuple, unpack_tensor_tuple

__all__ = ["AbstractSamplerState", "SamplerState", "SamplerStep", "IterativeSampler", "GaussianProposal", "LatentProposal", "MCMCStep",
           "GaussianMCMCSampler", "metropolis_accept", "default_set_samples_hook", "default_extract_sample_hook",
           "ReplicaExchangeMCMCStep", "ReplicaExchangeSampler", "exchange_permutation", "mcmc_tile_rows",
           "HamiltonianProposal", "HMCStep", "HamiltonianMCSampler", "hmc_tile_rows"]

# The most Metropolis steps one launch of bgk_pair_mcmc runs; longer runs are split (bitwise the same chain: the random stream and the
# carried f32 energies do not depend on the split), so that no single launch holds a shared GPU for long.  Measured on an MI355X
# (tools/mcmc_time.py, its last line): the widest shape of the envelope -- Lennard-Jones, n = 64, d = 3, 2^16 chains -- takes 70.46 ms
# for one launch of 64 steps (70.29 .. 70.74 over three rounds), 1.10 ms per step, so 224 steps are 0.247 s.  The replica-exchange
# launches (bgk_pair_remc) reuse it: tools/remc_time.py measured 1.07 ms per step at that shape with an exchange after every step.
# The HMC launches (bgk_pair_hmc) scale it, ``hmc_max_steps_per_launch``: tools/hmc_time.py measured, at that shape, 6.50 ms per step of
# 1 leapfrog step (52.03 ms for a launch of 8 steps, 51.87 .. 52.16) and 33.88 ms per step of 10 (271.03 ms, 269.95 .. 271.18) next to
# 1.062 ms per Metropolis step (67.98 ms for 64 steps) -- 16 rows per tile instead of 41 -- so a step of L leapfrog steps counts as
# 2.86 L + 3.26 Metropolis steps: 7 steps per launch at L = 10 are 0.237 s.
MCMC_MAX_STEPS_PER_LAUNCH = 224

# The tile height from which an ``MCMCStep`` takes the HMC kernel by default on a pair target (``hmc_fused_by_default``): the lowest
# at which it was measured faster than the general path.  Five LDS tiles per chain bound the chains in flight per CU, so the kernel
# loses ground as rows grow wider.  tools/hmc_time.py on an MI355X, Lennard-Jones, 2^16 chains, 10 leapfrog steps, ms per step fused
# (kernel forced) / general: n = 16 (64 rows) 0.637 / 3.629; n = 20 (51 rows) 1.329 / 3.686; n = 26 (40 rows) 2.668 / 3.722; n = 40
# (26 rows) 7.283 / 6.067; n = 64 (16 rows) 33.70 / 18.56.  The particle box of 38 (41 rows) took 3.502 / 2.03: its general path is
# cheaper, and no box was measured faster, so box targets take the kernel only with ``fused = "always"``.
HMC_FUSED_MIN_ROWS = 40


# ---- state ---------------------------------------------------------------------------------------------------------------------
class AbstractSamplerState:
    """Interface of the internal state of iterative samplers (_iterative_helpers.py:9-71)."""

    def as_dict(self):
        raise NotImplementedError()

    def _replace(self, **kwargs):
        raise NotImplementedError()

    def evaluate_energy_force(self, energy_model, evaluate_energies=True, evaluate_forces=True):
        """a new state with up-to-date energies / forces"""
        state = self.as_dict()
        evaluate_energies = evaluate_energies and not state["energies_up_to_date"]
        energies = energy_model.energy(*state["samples"])[..., 0] if evaluate_energies else state["energies"]
        evaluate_forces = evaluate_forces and not state["forces_up_to_date"]
        forces = energy_model.force(*state["samples"]) if evaluate_forces else state["forces"]
        return self.replace(energies=energies, forces=forces)

    def replace(self, **kwargs):
        """a new state with updated fields: setting energies / forces marks them up to date, setting samples alone marks them
        stale; samples are mapped to the primary cell of the box vectors"""
        state_dict = self.as_dict()
        if "energies" in kwargs:
            kwargs = {**kwargs, "energies_up_to_date": True}
        elif "samples" in kwargs:
            kwargs = {**kwargs, "energies_up_to_date": False}
        if "forces" in kwargs:
            kwargs = {**kwargs, "forces_up_to_date": True}
        elif "samples" in kwargs:
            kwargs = {**kwargs, "forces_up_to_date": False}
        box_vectors = None
        if "box_vectors" in kwargs:
            box_vectors = kwargs["box_vectors"]
        elif "box_vectors" in state_dict:
            box_vectors = state_dict["box_vectors"]
        if "samples" in kwargs and box_vectors is not None:
            kwargs = {**kwargs, "samples": tuple(_map_to_primary_cell(x, cell) for x, cell in zip(kwargs["samples"], box_vectors))}
        return self._replace(**kwargs)


def default_set_samples_hook(x):
    """by default, use samples as is"""
    return x


def default_extract_sample_hook(state):
    """the samples of a state"""
    return state.as_dict()["samples"]


def _bmv(m, bv):
    return torch.einsum("ij,...j->...i", m, bv)


def _map_to_primary_cell(x, cell):
    """coordinates x [..., n] mapped into the primary cell of the lattice vectors ``cell`` (column-wise, upper triangular)"""
    if cell is None:
        return x
    n = torch.floor(_bmv(torch.inverse(cell), x))
    return x - _bmv(cell, n)


@dataclasses.dataclass(frozen=True)
class _SamplerStateData:
    samples: Sequence[torch.Tensor]
    velocities: Sequence[torch.Tensor] = None
    energies: torch.Tensor = None
    forces: Sequence[torch.Tensor] = None
    box_vectors: Sequence[torch.Tensor] = None
    energies_up_to_date: bool = False
    forces_up_to_date: bool = False


class SamplerState(AbstractSamplerState):
    """A minibatch of samples with optional velocities, energies, forces and box vectors (iterative.py:49-118); samples, velocities,
    forces and box vectors are stored as tuples of tensors."""
    _tuple_kwargs = ["samples", "velocities", "forces", "box_vectors"]

    def __init__(self, dataclass=_SamplerStateData, set_samples_hook=default_set_samples_hook, **kwargs):
        self._dataclass = dataclass
        self.set_samples_hook = set_samples_hook
        kwargs_with_tuples = dict()
        for key, value in kwargs.items():
            if key in self._tuple_kwargs:
                value = pack_tensor_in_tuple(value)
            kwargs_with_tuples[key] = value
        self._data = dataclass(**kwargs_with_tuples)

    def __getattr__(self, field):
        try:
            return getattr(self.__dict__["_data"], field)
        except (AttributeError, KeyError) as e:
            raise AttributeError(f"SamplerState has no attribute '{field}'; {str(e)}")

    def __str__(self):
        return str(self._data)

    def as_dict(self):
        return dataclasses.asdict(self._data)

    def _replace(self, **kwargs):
        data = {**self.as_dict(), **kwargs}
        if "samples" in kwargs:
            data["samples"] = self.set_samples_hook(data["samples"])
        return SamplerState(dataclass=self._dataclass, set_samples_hook=self.set_samples_hook, **data)


# ---- the kernel launch ------------------------------------------------------------------------------------------------------------
def _chain_launch_checks(fn, plan, x, temperature, noise, uniforms, n_rows, n_accepted, tensors=(), noun="target"):
    """What ``pair_mcmc``, ``pair_hmc`` and ``annealing.pair_anneal`` check first: the columns of x [B, n d] against the plan, noise with
    uniforms (``n_rows`` rows each), and the tensors every chain launch has next to the caller's f32 ``tensors``, (tensor or None, shape)
    pairs.  Returns the tensor [B] of temperatures, or None for a number."""
    B, nd = x.shape
    if nd != plan.n_particles * plan.n_dims:
        raise ValueError(f"{fn}: x has {nd} columns, the {noun} {plan.n_particles} x {plan.n_dims}")
    if (noise is None) != (uniforms is None):
        raise ValueError(f"{fn}: noise and uniforms go together")
    temps = temperature if torch.is_tensor(temperature) else None
    _check_tensors(fn, x, [(x, (B, nd)), (temps, (B,)), (noise, (n_rows, B, nd)), (uniforms, (n_rows, B)), *tensors])
    _check_tensors(fn, x, [(n_accepted, (B,))], dtype=torch.int32)
    return temps


def pair_mcmc(plan, x, e, e_valid, temperature, noise_std, n_steps, noise=None, uniforms=None, seed=0, offset=0, row0=0,
              traj=None, traj_e=None, traj_every=0, n_accepted=None, accumulate=False, n_replicas=0, exchange_every=1,
              exchange_phase=0, exchange_parity=0, exchange_uniforms=None, n_exchanged=None, walkers=None):
    """One launch of bgk_pair_mcmc (bgk_box_mcmc for a ``BoxPlan``): ``n_steps`` Metropolis steps of the chains x [B, n d] (f32,
    contiguous, HIP; updated IN PLACE) on the target of the plan.  e [B]: raw energies (temperature 1), read if ``e_valid``, written for the final state.
    ``temperature``: a positive number or an f32 tensor [B].  noise [n_steps, B, n d] and uniforms [n_steps, B], or neither (Philox
    numbers of (seed, offset + step, chain row0 + b)).  traj [n_steps // traj_every, B, n d] / traj_e [n_steps // traj_every, B]: the
    state / energy after every ``traj_every``-th step.  n_accepted [B] (int32): written, or added to with ``accumulate``.

    With ``n_replicas`` K >= 2 the launch is bgk_pair_remc / bgk_box_remc: the chains are B / K ladders of K temperatures, ladder-major,
    ``temperature`` is the tensor [B], and after every step that completes an epoch of ``exchange_every`` steps (``exchange_phase`` of
    which were taken before the launch) the pairs of slots (k, k + 1), k = parity (mod 2), try an exchange; ``exchange_parity`` is the
    first attempt's.  exchange_uniforms [(exchange_phase + n_steps) // exchange_every, B]: with noise / uniforms, all or none.
    n_exchanged [B] (int32): accepted exchanges at the pair's lower slot, like n_accepted; walkers [B] (int32, in / out)."""
    from . import _lib
    B, nd = x.shape
    n_frames = n_steps // traj_every if traj is not None else 0
    temps = _chain_launch_checks("pair_mcmc", plan, x, temperature, noise, uniforms, n_steps, n_accepted,
                                 [(e, (B,)), (traj, (n_frames, B, nd)), (traj_e, (n_frames, B))])
    if traj is not None and traj_every < 1:
        raise ValueError("pair_mcmc: traj_every must be at least 1")
    name = "bgk_box_" if isinstance(plan, BoxPlan) else "bgk_pair_"
    more = ()
    if n_replicas:
        if temps is None:
            raise ValueError("pair_mcmc: replica exchange needs a tensor of B temperatures")
        if exchange_every < 1 or not 0 <= exchange_phase < exchange_every:
            raise ValueError("pair_mcmc: exchange_every must be at least 1 and 0 <= exchange_phase < exchange_every")
        n_exchanges = (exchange_phase + n_steps) // exchange_every
        if n_exchanges == 0:
            exchange_uniforms = None
        elif (noise is None) != (exchange_uniforms is None):
            raise ValueError("pair_mcmc: noise, uniforms and exchange_uniforms go together")
        _check_tensors("pair_mcmc", x, [(exchange_uniforms, (n_exchanges, B))])
        _check_tensors("pair_mcmc", x, [(n_exchanged, (B,)), (walkers, (B,))], dtype=torch.int32)
        more = (int(n_replicas), int(exchange_every), int(exchange_phase), int(exchange_parity), _lib.ptr(exchange_uniforms),
                _lib.ptr(n_exchanged), _lib.ptr(walkers))
    elif exchange_uniforms is not None or n_exchanged is not None or walkers is not None:
        raise ValueError("pair_mcmc: exchange arguments without n_replicas")
    name += "remc" if n_replicas else "mcmc"
    with torch.cuda.device(x.device):
        st = getattr(_lib.lib(), name)(_lib.ptr(x), B, *_target_args(plan), _lib.ptr(e), int(bool(e_valid)),
                                       1.0 if temps is not None else float(temperature),
                                       _lib.ptr(temps), float(noise_std), int(n_steps), _lib.ptr(noise), _lib.ptr(uniforms),
                                       int(seed) & (2 ** 64 - 1), int(offset) & 0xffffffff, int(row0), _lib.ptr(traj), _lib.ptr(traj_e),
                                       int(traj_every), _lib.ptr(n_accepted), int(bool(accumulate)), _lib.stream_ptr(x.device), *more)
    _lib.check(st, name)


def pair_hmc(plan, x, e, e_valid, temperature, step_size, n_leapfrog, mass, n_steps, noise=None, uniforms=None, seed=0, offset=0, row0=0,
             traj=None, traj_e=None, traj_every=0, n_accepted=None, accumulate=False):
    """One launch of bgk_pair_hmc (bgk_box_hmc for a ``BoxPlan``): ``n_steps`` Hamiltonian Monte Carlo steps of ``n_leapfrog`` leapfrog
    steps of size ``step_size`` at ``mass`` on the chains x [B, n d] (f32, contiguous, HIP; updated IN PLACE).  Every other argument is
    ``pair_mcmc``'s; noise [n_steps, B, n d] holds the standard normals of the momenta."""
    from . import _lib
    B, nd = x.shape
    n_frames = n_steps // traj_every if traj is not None else 0
    temps = _chain_launch_checks("pair_hmc", plan, x, temperature, noise, uniforms, n_steps, n_accepted,
                                 [(e, (B,)), (traj, (n_frames, B, nd)), (traj_e, (n_frames, B))])
    if traj is not None and traj_every < 1:
        raise ValueError("pair_hmc: traj_every must be at least 1")
    name = "bgk_box_hmc" if isinstance(plan, BoxPlan) else "bgk_pair_hmc"
    with torch.cuda.device(x.device):
        st = getattr(_lib.lib(), name)(_lib.ptr(x), B, *_target_args(plan), _lib.ptr(e), int(bool(e_valid)),
                                       1.0 if temps is not None else float(temperature), _lib.ptr(temps),
                                       float(step_size), int(n_leapfrog), float(mass), int(n_steps), _lib.ptr(noise), _lib.ptr(uniforms),
                                       int(seed) & (2 ** 64 - 1), int(offset) & 0xffffffff, int(row0), _lib.ptr(traj), _lib.ptr(traj_e),
                                       int(traj_every), _lib.ptr(n_accepted), int(bool(accumulate)), _lib.stream_ptr(x.device))
    _lib.check(st, name)


def hmc_max_steps_per_launch(n_leapfrog):
    """The most HMC steps of ``n_leapfrog`` leapfrog steps one launch of bgk_pair_hmc runs, so that a launch holds the device no longer
    than ``MCMC_MAX_STEPS_PER_LAUNCH`` Metropolis steps do: the measured cost of an HMC step in Metropolis steps (the comment of
    ``MCMC_MAX_STEPS_PER_LAUNCH``), rounded up.  Results do not depend on the split."""
    return max(1, MCMC_MAX_STEPS_PER_LAUNCH // math.ceil(2.86 * int(n_leapfrog) + 3.26))


def hmc_fused_by_default(plan):
    """whether an ``MCMCStep`` with ``fused = True`` runs a ``HamiltonianProposal`` on the target of ``plan`` inside the kernel: a pair
    target (kinds 0 .. 2) whose tile has at least ``HMC_FUSED_MIN_ROWS`` rows, i.e. n d <= 79.  ``fused = "always"`` takes the kernel wherever it
    accepts the state."""
    return isinstance(plan, PairPlan) and hmc_tile_rows(plan.n_particles * plan.n_dims) >= HMC_FUSED_MIN_ROWS


def _chain_tile_rows(nd, first, second):
    """rows of a tile of a chain kernel whose lanes keep ``first`` + ``second`` LDS tiles of rows of ``nd`` floats (csrc/bgk_chain.h,
    ``chain_layout``): the most, at most 64, whose tiles (odd row stride, the second side starting at a multiple of 32 words) fit
    63,488 bytes"""
    S = nd | 1
    rows = min(64, 63488 // (4 * (first + second) * S))
    while (((first * rows * S + 31) & ~31) + second * rows * S) * 4 > 63488:
        rows -= 1
    return rows


def hmc_tile_rows(nd):
    """rows of a tile of the HMC kernel for rows of ``nd`` floats (csrc/bgk_hmc.hip, ``hmc_run``): the most, at most 64, whose five LDS
    tiles (odd row stride, the second (position, gradient) pair starting at a multiple of 32 words) fit 63,488 bytes"""
    return _chain_tile_rows(nd, 3, 2)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _launch_plan(unit, count, cap):
    """[(steps, traj_every, frames)] of the launches that run ``count`` units of ``unit`` steps and record the state after every unit,
    no launch longer than ``cap`` steps (traj_every = 0: a piece of a unit longer than the cap, nothing recorded)"""
    cap = max(1, int(cap))
    out = []
    if unit <= cap:
        per = cap // unit
        done = 0
        while done < count:
            k = min(per, count - done)
            out.append((k * unit, unit, k))
            done += k
    else:
        for _ in range(count):
            left = unit
            while left > cap:
                out.append((cap, 0, 0))
                left -= cap
            out.append((left, left, 1))
    return out


# ---- steps ----------------------------------------------------------------------------------------------------------------------
class SamplerStep(torch.nn.Module):
    """Base class of sampler steps: ``_step`` maps a state to a state; ``forward`` applies it ``n_steps`` times (iterative.py:195-214)."""

    def __init__(self, n_steps=1):
        super().__init__()
        self._n_steps = n_steps

    def _step(self, state):
        raise NotImplementedError()

    def forward(self, state):
        for _ in range(self._n_steps):
            state = self._step(state)
        return state


class GaussianProposal(torch.nn.Module):
    """Normal distributed displacement of the samples by ``noise_std`` (mcmc.py:29-46)."""

    def __init__(self, noise_std=0.1):
        super().__init__()
        self._noise_std = noise_std

    def forward(self, state):
        delta_log_prob = 0.0  # symmetric density
        proposed_state = state.replace(samples=tuple(x + torch.randn_like(x) * self._noise_std for x in state.as_dict()["samples"]))
        return proposed_state, delta_log_prob


class LatentProposal(torch.nn.Module):
    """Proposal in the latent space of a flow whose forward direction is latent-to-target (mcmc.py:49-83):
    delta_log_prob = base delta - (logdet of the forward map at the proposal + logdet of the inverse map at the state)."""

    def __init__(self, flow, base_proposal=GaussianProposal(noise_std=0.1), flow_kwargs=dict()):
        super().__init__()
        self.flow = flow
        self.base_proposal = base_proposal
        self.flow_kwargs = flow_kwargs

    def forward(self, state):
        *z, logdet_inverse = self.flow.forward(*state.as_dict()["samples"], inverse=True, **self.flow_kwargs)
        proposed_latent, delta_log_prob = self.base_proposal.forward(state.replace(samples=z))
        *proposed_samples, logdet_forward = self.flow.forward(*proposed_latent.as_dict()["samples"])
        delta_log_prob = delta_log_prob - (logdet_forward + logdet_inverse)
        return proposed_latent.replace(samples=proposed_samples), delta_log_prob[:, 0]


class HamiltonianProposal(torch.nn.Module):
    """Hamiltonian Monte Carlo proposal: fresh momenta, ``n_leapfrog`` leapfrog steps of size ``step_size`` in the potential
    ``energy`` / ``temperature``, and the change of the kinetic energy as ``delta_log_prob`` -- the proposal protocol of ``MCMCStep``,
    ``forward(state) -> (proposed_state, delta_log_prob)``.  With h = step_size, m = mass (a positive number), T = temperature (a positive
    number or a tensor of one value per chain), f(x) = -grad E(x) / T (E at temperature 1) and xi standard normal, shaped like the samples:

        p0 = sqrt(m) xi;  p = p0 + (h / 2) f(x);  n_leapfrog times:  x = x + (h / m) p,  p = p + c f(x)  (c = h; h / 2 after the last drift)
        delta_log_prob = K(p) - K(p0), [B],  K(p) = |p|^2 / (2 m)

    so that ``metropolis_accept`` decides on -(E' / T - E / T) - delta_log_prob = -(change of the Hamiltonian).  The momenta are
    refreshed in full at every step; ``n_leapfrog = 1`` is the Metropolis-adjusted Langevin algorithm.  The forces come from
    ``energy.force`` on a detached copy (no graph reaches the state); the state holds exactly one samples tensor; its ``velocities``
    and ``forces`` are ignored.

    The chain stays exact when ``temperature`` differs from the step's ``target_temperatures``: leapfrog is reversible and
    volume-preserving whatever potential drives it, so the accept step corrects for it and only the acceptance rate suffers.

    Inside a plain ``MCMCStep`` on the same energy and temperature, with numeric ``step_size`` and ``mass``, whole chains run in one
    launch of csrc/bgk_hmc.hip (module docstring).  Inside a ``ReplicaExchangeMCMCStep`` the general path runs: exchanges between HMC
    chains inside the kernel are not built."""

    def __init__(self, energy, step_size, n_leapfrog=10, mass=1.0, temperature=1.0):
        super().__init__()
        if not (_is_number(mass) and mass > 0):
            raise ValueError("HamiltonianProposal: mass must be a positive number")
        if not (isinstance(n_leapfrog, int) and not isinstance(n_leapfrog, bool) and n_leapfrog >= 1):
            raise ValueError("HamiltonianProposal: n_leapfrog must be an integer, at least 1")
        self.energy = energy
        self.step_size = step_size
        self.n_leapfrog = n_leapfrog
        self.mass = mass
        self.temperature = temperature

    def _force(self, x):
        """f(x) = -grad E(x) / T, detached"""
        f = self.energy.force(x.detach().clone()).detach()
        t = self.temperature
        if torch.is_tensor(t):
            t = t.to(device=x.device, dtype=x.dtype).reshape((-1,) + (1,) * (x.dim() - 1))
        return f / t

    def forward(self, state):
        samples = state.as_dict()["samples"]
        if len(samples) != 1 or not torch.is_tensor(samples[0]):
            raise ValueError("HamiltonianProposal takes a state with exactly one samples tensor")
        x = samples[0].detach()
        h, m = self.step_size, self.mass
        p0 = math.sqrt(m) * torch.randn_like(x)
        p = p0 + (h / 2) * self._force(x)
        for k in range(self.n_leapfrog):
            x = x + (h / m) * p
            p = p + (h if k + 1 < self.n_leapfrog else h / 2) * self._force(x)
        batch = x.shape[0]
        kinetic = [(q * q).reshape(batch, -1).sum(dim=-1) / (2 * m) for q in (p, p0)]
        return state.replace(samples=(x,)), kinetic[0] - kinetic[1]


def metropolis_accept(current_energies, proposed_energies, proposal_delta_log_prob):
    """Metropolis criterion (mcmc.py:192-222): True where min(0, -(u' - u) - delta_log_prob) >= log r, r ~ U(0, 1); a NaN or +inf
    proposed energy is never accepted (the comparison is False)."""
    log_prob = -(proposed_energies - current_energies) - proposal_delta_log_prob
    log_acceptance_ratio = torch.min(torch.zeros_like(proposed_energies), log_prob)
    log_random = torch.rand_like(log_acceptance_ratio).log()
    return log_acceptance_ratio >= log_random


class MCMCStep(SamplerStep, _FusedSampling):
    """Metropolis Monte Carlo on ``target_energy`` with ``proposal`` at ``target_temperatures`` (a number or a tensor broadcast along the
    batch), ``n_steps`` steps per ``forward`` (mcmc.py:86-122).

    Where the fused path applies (module docstring) ``forward`` is one launch of bgk_pair_mcmc on a copy of the samples.  Its random
    numbers come from the Philox stream of this object (``_FusedSampling``: key from ``torch.initial_seed()``, rank and stream id, the
    per-object counter is the index of the next step, both travel in ``state_dict``), unless ``feed_noise`` has handed it explicit ones.
    ``n_accepted`` (int32 [B]) counts the accepted steps per chain and ``n_proposed`` the steps taken, on either path."""
    fused = True                       # False: the general path; "always": the HMC kernel also where it is not the default

    def __init__(self, target_energy, proposal=GaussianProposal(), target_temperatures=1.0, n_steps=1):
        super().__init__(n_steps=n_steps)
        self.target_energy = target_energy
        self.target_temperatures = target_temperatures
        self.proposal = proposal
        self.n_accepted = None
        self.n_proposed = 0
        self.chain_offset = 0          # global index of this state's first chain: chains sharded over processes draw the numbers of the whole
        self._fed = None

    # -- the general path: the reference's step
    def _step(self, state):
        state = state.evaluate_energy_force(self.target_energy, evaluate_forces=False)
        proposed_state, delta_log_prob = self.proposal.forward(state)
        proposed_state = proposed_state.evaluate_energy_force(self.target_energy, evaluate_forces=False)
        new_dict = proposed_state.as_dict()
        old_dict = state.as_dict()
        accept = metropolis_accept(
            current_energies=old_dict["energies"] / self.target_temperatures,
            proposed_energies=new_dict["energies"] / self.target_temperatures,
            proposal_delta_log_prob=delta_log_prob
        )
        counts = accept.to(torch.int32)
        if self.n_accepted is None or self.n_accepted.shape != counts.shape or self.n_accepted.device != counts.device:
            self.n_accepted, self.n_proposed = counts, 0
        else:
            self.n_accepted = self.n_accepted + counts
        self.n_proposed += 1
        return state.replace(
            samples=tuple(torch.where(accept[..., None], new, old) for new, old in zip(new_dict["samples"], old_dict["samples"])),
            energies=torch.where(accept, new_dict["energies"], old_dict["energies"])
        )

    # -- the fused path
    def feed_noise(self, noise, uniforms):
        """explicit random numbers for the next fused steps instead of the Philox stream: noise [S, B, n d] standard normals and
        uniforms [S, B] (f32, on the samples' device); each fused step consumes one row of either, ``feed_noise(None, None)``
        returns to the Philox stream"""
        if noise is None and uniforms is None:
            self._fed = None
            return self
        if noise.dim() != 3 or uniforms.dim() != 2 or uniforms.shape != noise.shape[:2]:
            raise ValueError("feed_noise: noise [S, B, n d] and uniforms [S, B]")
        self._fed = [noise.contiguous(), uniforms.contiguous(), 0]
        return self

    def _temperatures(self, B, device):
        """the kernel's temperature argument -- a float, or an f32 tensor [B] on the device -- or None; a tensor's host check is made
        once per state of the tensor"""
        t = self.target_temperatures
        if isinstance(t, (int, float)) and not isinstance(t, bool):
            return float(t) if t > 0 else None
        if not torch.is_tensor(t) or t.numel() != B or t.dim() > 1 or not t.dtype.is_floating_point:
            return None
        key = (t.data_ptr(), t._version, t.device, t.dtype, device)
        hit = self.__dict__.get("_temp_cache")
        if hit is None or hit[0] != key:
            ok = bool((t > 0).all()) and bool(torch.isfinite(t).all())
            dev_t = t.detach().reshape(B).to(device=device, dtype=torch.float32).contiguous() if ok else None
            hit = self.__dict__["_temp_cache"] = (key, dev_t)
        return hit[1]

    def _chain_launch(self):
        """the launch of the proposal's chain kernel, ``pair_mcmc`` / ``pair_hmc`` without the proposal's own arguments --
        f(plan, x, e, e_valid, temperature, n_steps, noise, uniforms, ...) -- or None if no kernel takes the proposal"""
        proposal = self.proposal
        if type(proposal) is GaussianProposal:
            std = proposal._noise_std
            if not (_is_number(std) and std >= 0):
                return None
            return lambda plan, x, e, e_valid, temps, steps, *args, **kwargs: pair_mcmc(plan, x, e, e_valid, temps, std, steps, *args, **kwargs)
        if type(proposal) is HamiltonianProposal:
            h, L, m, t = proposal.step_size, proposal.n_leapfrog, proposal.mass, proposal.temperature
            if proposal.energy is not self.target_energy or not (_is_number(h) and h > 0 and _is_number(m) and m > 0):
                return None
            if not (isinstance(L, int) and not isinstance(L, bool) and L >= 1):
                return None
            mine = self.target_temperatures
            if not (t is mine if torch.is_tensor(t) or torch.is_tensor(mine) else _is_number(t) and _is_number(mine) and t == mine):
                return None
            return lambda plan, x, e, e_valid, temps, steps, *args, **kwargs: pair_hmc(plan, x, e, e_valid, temps, h, L, m, steps, *args, **kwargs)
        return None

    def _launch_cap(self):
        """the most steps of one launch of ``_chain_launch``"""
        if type(self.proposal) is HamiltonianProposal:
            return hmc_max_steps_per_launch(self.proposal.n_leapfrog)
        return MCMC_MAX_STEPS_PER_LAUNCH

    def _fused_setup(self, state):
        """(plan, B, temperature argument) if the kernel takes this state, else None"""
        if not self.fused or self._chain_launch() is None:
            return None
        if not isinstance(state, SamplerState) or state.set_samples_hook is not default_set_samples_hook:
            return None
        data = state.__dict__["_data"]
        samples = data.samples
        if getattr(data, "box_vectors", None) is not None or len(samples) != 1 or not torch.is_tensor(samples[0]):
            return None
        plan = _kernel_plan(self.target_energy, 1.0)
        if not isinstance(plan, (PairPlan, BoxPlan)):
            return None
        if type(self.proposal) is HamiltonianProposal and self.fused != "always" and not hmc_fused_by_default(plan):
            return None                # measured slower than the general path, or not measured (HMC_FUSED_MIN_ROWS)
        x, nd = samples[0], plan.n_particles * plan.n_dims
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (2, 3) and x.shape[0] > 0):
            return None
        if tuple(x.shape[1:]) not in ((nd,), (plan.n_particles, plan.n_dims)):
            return None
        temps = self._temperatures(x.shape[0], x.device)
        if temps is None:
            return None
        return plan, x.shape[0], temps

    def _carried_energies(self, state, B):
        """the state's energies as the kernel's f32 [B], if they are up to date (a copy: the launch overwrites them)"""
        data = state.__dict__["_data"]
        e = data.energies
        if not data.energies_up_to_date or not torch.is_tensor(e) or e.numel() != B or e.device != data.samples[0].device:
            return None
        return e.detach().reshape(B).to(torch.float32).clone()

    def _run_chains(self, setup, x2, e, e_valid, launches, traj=None, traj_e=None, tick=None):
        """the launches of ``_launch_plan`` on the chains x2 [B, n d] / e [B] in place; frames go to traj / traj_e in order;
        ``tick(steps enqueued so far)`` is called after every launch"""
        plan, B, temps = setup
        total = sum(steps for steps, _, _ in launches)
        if total == 0:
            return
        if self.n_accepted is None or self.n_accepted.shape != (B,) or self.n_accepted.device != x2.device or self.n_accepted.dtype != torch.int32:
            self.n_accepted, self.n_proposed, fresh = torch.empty(B, dtype=torch.int32, device=x2.device), 0, True
        else:
            fresh = False
        fed = self._fed
        if fed is not None:
            if fed[0].shape[0] - fed[2] < total or fed[0].shape[1:] != x2.shape or fed[0].device != x2.device:
                raise ValueError(f"MCMCStep: {total} steps of {tuple(x2.shape)} chains need as many rows of fed noise; "
                                 f"{fed[0].shape[0] - fed[2]} rows of {tuple(fed[0].shape[1:])} are left")
            seed = offset = 0
        else:
            from . import dp
            st = self._philox_ids()
            seed = (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1)
            offset, st[1] = st[1], st[1] + total
        launch = self._chain_launch()
        frame = 0
        done = 0
        for steps, every, frames in launches:
            noise = uniforms = None
            if fed is not None:
                noise, uniforms = fed[0][fed[2]:fed[2] + steps], fed[1][fed[2]:fed[2] + steps]
                fed[2] += steps
            launch(plan, x2, e, e_valid, temps, steps, noise, uniforms, seed, offset, self.chain_offset,
                   None if not frames else traj[frame:frame + frames].view(frames, B, -1),
                   None if not frames or traj_e is None else traj_e[frame:frame + frames], every, self.n_accepted, not fresh,
                   **self._begin_launch(steps, x2, fresh))
            e_valid, fresh = True, False
            offset += steps
            frame += frames
            done += steps
            if tick is not None:
                tick(done)
        self.n_proposed += total

    def _begin_launch(self, steps, x2, fresh):
        """called before every launch of ``steps`` steps; returns further keywords of ``pair_mcmc`` (a subclass advances its own
        schedule here: the replica exchange)"""
        return {}

    def _hand_out(self, state, x2, e):
        """called with the state a fused run hands out and the working chains it came from (a subclass may keep them)"""

    def _working_copy(self, state, B):
        """(x [B, n d], e [B], e_valid): the chains of a state as the launches advance them in place -- a copy of the samples and, if
        they are up to date, of the energies"""
        x = state.__dict__["_data"].samples[0]
        e = self._carried_energies(state, B)
        e_valid = e is not None
        if e is None:
            e = torch.empty(B, dtype=torch.float32, device=x.device)
        return x.detach().clone().view(B, -1), e, e_valid

    def _fused_forward(self, state, setup, n_steps):
        plan, B, _ = setup
        y, e, e_valid = self._working_copy(state, B)
        self._run_chains(setup, y, e, e_valid, [(k, 0, 0) for k in _split(n_steps, self._launch_cap())])
        out = _advanced_state(state, y.view(state.__dict__["_data"].samples[0].shape), e)
        self._hand_out(out, y, e)
        return out

    def forward(self, state):
        setup = self._fused_setup(state)
        if setup is None:
            return super().forward(state)
        return self._fused_forward(state, setup, self._n_steps)


def _split(total, cap):
    cap = max(1, int(cap))
    return [min(cap, total - s) for s in range(0, total, cap)]


class HMCStep(MCMCStep):
    """Hamiltonian Monte Carlo on ``target_energy`` at ``target_temperatures``: an ``MCMCStep`` whose proposal is a
    ``HamiltonianProposal`` on the same energy and the same temperatures"""

    def __init__(self, target_energy, step_size, n_leapfrog=10, mass=1.0, target_temperatures=1.0, n_steps=1):
        proposal = HamiltonianProposal(target_energy, step_size, n_leapfrog=n_leapfrog, mass=mass, temperature=target_temperatures)
        super().__init__(target_energy, proposal=proposal, target_temperatures=target_temperatures, n_steps=n_steps)


# ---- replica exchange --------------------------------------------------------------------------------------------------------------
def mcmc_tile_rows(nd):
    """rows of a tile of the chain kernel for rows of ``nd`` floats (csrc/bgk_mcmc.hip, ``mcmc_run``): the most, at most 64, whose two
    LDS tiles (odd row stride, the second one starting at a multiple of 32 words) fit 63,488 bytes"""
    return _chain_tile_rows(nd, 1, 1)


def exchange_permutation(energies, temperatures, r, n_replicas, parity):
    """The exchange rule of ``ReplicaExchangeMetropolisGauss.run`` (_mcmc/metropolis.py:172-188) for L ladders at once: energies,
    temperatures, r [B = L K], ladder-major.  For every pair of slots (k, k + 1) with k = parity (mod 2) and k + 1 < K
    c = -(e[k+1] - e[k]) (1 / T[k+1] - 1 / T[k]), and the pair exchanges iff -log r > c, r the entry of its lower slot (a NaN never
    exchanges).  Returns (perm [B]: the chain that sits in each slot afterwards, lower [P]: the pairs' lower slots, swap [P])."""
    B, K = energies.shape[0], int(n_replicas)
    dev = energies.device
    lower = (torch.arange(0, B, K, device=dev)[:, None] + torch.arange(parity, K - 1, 2, device=dev)[None, :]).reshape(-1)
    upper = lower + 1
    beta = 1.0 / temperatures
    c = -(energies[upper] - energies[lower]) * (beta[upper] - beta[lower])
    swap = -torch.log(r[lower]) > c
    perm = torch.arange(B, device=dev)
    perm[lower] = torch.where(swap, upper, lower)
    perm[upper] = torch.where(swap, lower, upper)
    return perm, lower, swap


class ReplicaExchangeMCMCStep(MCMCStep):
    """Parallel tempering: Metropolis Monte Carlo of L ladders of K = len(temperatures) replicas -- the state's B = L K chains,
    ladder-major: chain b is slot b % K of ladder b / K and runs at ``temperatures[b % K]`` -- with an exchange attempt between
    neighbouring slots after every ``exchange_every``-th step (``exchange_permutation``: the rule of the reference's numpy
    ``ReplicaExchangeMetropolisGauss``, pairs (0, 1), (2, 3), ... and (1, 2), (3, 4), ... in turn).  An exchange swaps configuration and
    energy of two slots; temperatures and counters belong to the slot.

    The schedule follows ``steps_done`` (an int, assignable; not the Philox counter): an exchange follows every step that makes it a
    multiple of ``exchange_every``, with parity ``(steps_done // exchange_every - 1) & 1``.  The exchange FOLLOWS the frame of its step:
    the state ``forward`` returns (and an ``IterativeSampler`` records) after such a step is the one before the exchange, which is
    applied when the chains continue -- ``apply_pending_exchange(state)`` applies it at the end of a run.

    ``n_exchanged`` (int32 [B]) counts the accepted exchanges of pair (k, k + 1) at its lower slot, ``n_exchange_attempts`` the exchange
    steps, ``walkers`` (int32 [B]) says which walker (0..K-1 of its ladder, by its start slot) sits in each slot.

    General path (any energy with energies [B], proposal, device, dtype): ``MCMCStep._step`` and the exchange in torch ops; every
    exchange makes exactly one ``torch.rand_like(energies)`` call and uses the entry at each pair's lower slot.  A
    ``HamiltonianProposal`` always runs this path: exchanges between HMC chains inside the kernel are not built.  Fused path
    (bgk_pair_remc / bgk_box_remc, the exchange by wave shuffles inside the chain kernel): under the conditions of ``MCMCStep``'s, K within
    the kernel's tile height (``mcmc_tile_rows``) and ``chain_offset`` a multiple of K.  There the due exchange of a run's last step has
    already happened in the working chains the step keeps for the state it handed out (``_HandedOut``; ``forward`` and
    ``IterativeSampler`` both register their runs), and in ``walkers`` / ``n_exchanged`` / ``n_exchange_attempts``.  Continuing from that
    state, or ``apply_pending_exchange`` of it, uses those chains.  A state from elsewhere gets the exchange in torch ops instead, and the
    kernel's exchange is taken out of ``walkers`` and the counters again, so that they describe the chains that go on."""

    def __init__(self, target_energy, temperatures, proposal=GaussianProposal(), n_steps=1, exchange_every=1):
        ladder = temperatures.detach().reshape(-1) if torch.is_tensor(temperatures) else torch.as_tensor(temperatures, dtype=torch.float64).reshape(-1)
        if ladder.numel() < 2 or not ladder.dtype.is_floating_point or not bool((ladder > 0).all()) or not bool(torch.isfinite(ladder).all()):
            raise ValueError("ReplicaExchangeMCMCStep: temperatures must be at least two positive numbers")
        if not isinstance(exchange_every, int) or exchange_every < 1:
            raise ValueError("ReplicaExchangeMCMCStep: exchange_every must be a positive integer")
        super().__init__(target_energy, proposal=proposal, target_temperatures=ladder, n_steps=n_steps)
        self.temperatures = ladder
        self.n_replicas = ladder.numel()
        self.exchange_every = exchange_every
        self.steps_done = 0
        self.n_exchanged = None
        self.n_exchange_attempts = 0
        self.walkers = None
        self._applied_at = 0           # the value of ``steps_done`` whose exchange the states handed out have (``_exchange_due``)
        self._handed = None            # _HandedOut: the fused path's working chains of the state handed out last
        self._run = None               # inside ``_run_chains``: [steps left, counters before the run's last launch]
        self._before_last = None       # those counters, from the end of a run that ended with an exchange until ``_hand_out``
        self._tiled = None

    def _exchange_due(self):
        """the exchange after step ``steps_done`` is due and the state handed out does not have it -- also true for an object that was
        assigned a ``steps_done`` at the end of an epoch: it continues a run whose last state is the one before that exchange"""
        return self.steps_done > 0 and self.steps_done % self.exchange_every == 0 and self._applied_at != self.steps_done

    # -- bookkeeping
    def _tile(self, x):
        """the ladder tiled over the batch of x, in x's dtype on x's device (kept while these do not change)"""
        B, K = x.shape[0], self.n_replicas
        if B % K != 0:
            raise ValueError(f"ReplicaExchangeMCMCStep: {B} chains are not a whole number of ladders of {K} temperatures")
        dtype = x.dtype if x.dtype.is_floating_point else torch.get_default_dtype()
        key = (B, x.device, dtype)
        if self._tiled is None or self._tiled[0] != key:
            self._tiled = (key, self.temperatures.to(device=x.device, dtype=dtype).repeat(B // K))
        return self._tiled[1]

    def _book(self, B, device, reset=False):
        if reset or self.n_exchanged is None or self.n_exchanged.shape != (B,) or self.n_exchanged.device != device:
            self.n_exchanged = torch.zeros(B, dtype=torch.int32, device=device)
        if self.walkers is None or self.walkers.shape != (B,) or self.walkers.device != device:
            self.walkers = torch.arange(self.n_replicas, dtype=torch.int32, device=device).repeat(B // self.n_replicas)

    @staticmethod
    def _first_samples(state):
        return state.__dict__["_data"].samples[0] if isinstance(state, SamplerState) else state.as_dict()["samples"][0]

    # -- the general path
    def _exchange(self, state):
        """the exchange that is due, in torch ops"""
        self._applied_at = self.steps_done
        state = state.evaluate_energy_force(self.target_energy, evaluate_forces=False)
        data = state.as_dict()
        e = data["energies"]
        if e.dim() != 1:
            raise ValueError("ReplicaExchangeMCMCStep: the energies of the state must be one per chain, [B]")
        temps = self._tile(e)
        parity = (self.steps_done // self.exchange_every - 1) & 1
        r = torch.rand_like(e)
        perm, lower, swap = exchange_permutation(e, temps, r, self.n_replicas, parity)
        self._book(e.shape[0], e.device)
        self.n_exchanged[lower] += swap.to(torch.int32)
        self.walkers = self.walkers[perm]
        self.n_exchange_attempts += 1
        moved = {"samples": tuple(x[perm] for x in data["samples"]), "energies": e[perm]}
        if data.get("velocities") is not None:
            moved["velocities"] = tuple(v[perm] for v in data["velocities"])
        return state.replace(**moved)

    def _step(self, state):
        self.target_temperatures = self._tile(self._first_samples(state))
        state = self.apply_pending_exchange(state)
        self._handed = None
        state = super()._step(state)
        self.steps_done += 1
        return state

    def apply_pending_exchange(self, state):
        """the state with the exchange that is due after the last step, if there is one (``forward`` returns the state before it).  For
        the state the fused path handed out last that is a copy of its working chains, where the kernel has made the exchange; any other
        state is exchanged in torch ops, after the kernel's exchange has been taken out of ``walkers`` and the counters again."""
        if not self._exchange_due():
            return state
        handed = self._handed
        if handed is not None and handed.state is state:
            self._applied_at = self.steps_done
            handed.state = _advanced_state(state, handed.x.clone().view(self._first_samples(state).shape), handed.e.clone())
            return handed.state                        # the working chains now belong to this state: it has the exchange
        self._take_back()
        return self._exchange(state)

    # -- the fused path
    def feed_noise(self, noise, uniforms, exchange_uniforms=None):
        """as ``MCMCStep.feed_noise``, with exchange_uniforms [X, B]: every exchange consumes one row (its entries at the pairs' lower
        slots); all three or none"""
        if noise is None and uniforms is None and exchange_uniforms is None:
            self._fed = None
            return self
        if noise is None or uniforms is None or exchange_uniforms is None:
            raise ValueError("feed_noise: noise, uniforms and exchange_uniforms go together")
        super().feed_noise(noise, uniforms)
        if exchange_uniforms.dim() != 2 or exchange_uniforms.shape[1] != uniforms.shape[1]:
            raise ValueError("feed_noise: exchange_uniforms [X, B]")
        self._fed += [exchange_uniforms.contiguous(), 0]
        return self

    def _fused_setup(self, state):
        if not isinstance(state, SamplerState):
            return None
        samples = state.__dict__["_data"].samples
        if len(samples) != 1 or not torch.is_tensor(samples[0]) or samples[0].dim() < 1:
            return None
        x = samples[0]
        self.target_temperatures = self._tile(x)
        if type(self.proposal) is HamiltonianProposal:      # no exchanges inside the HMC kernel: the general path
            return None
        setup = super()._fused_setup(state)
        if setup is None or self.n_replicas > mcmc_tile_rows(setup[0].n_particles * setup[0].n_dims):
            return None
        if self.chain_offset % self.n_replicas != 0:
            raise ValueError("ReplicaExchangeMCMCStep: chain_offset must be a multiple of the number of temperatures")
        return setup

    def _begin_launch(self, steps, x2, fresh):
        K, E = self.n_replicas, self.exchange_every
        self._book(x2.shape[0], x2.device, reset=fresh)
        run = self._run
        if run is not None:
            run[0] -= steps
            if run[0] == 0:                            # the run's last launch: what it may exchange is what ``_take_back`` undoes
                run[1] = (self.walkers.clone(), self.n_exchanged.clone())
        phase = self.steps_done % E
        n_exchanges = (phase + steps) // E
        parity = (self.steps_done // E) & 1            # of the next exchange: (its steps_done // E - 1) & 1
        rows = None
        fed = self._fed
        if fed is not None and n_exchanges:
            if fed[3].shape[0] - fed[4] < n_exchanges or fed[3].device != x2.device:
                raise ValueError(f"ReplicaExchangeMCMCStep: {n_exchanges} exchanges need as many rows of fed exchange_uniforms; "
                                 f"{fed[3].shape[0] - fed[4]} are left")
            rows = fed[3][fed[4]:fed[4] + n_exchanges]
            fed[4] += n_exchanges
        self.steps_done += steps
        self.n_exchange_attempts += n_exchanges
        return dict(n_replicas=K, exchange_every=E, exchange_phase=phase, exchange_parity=parity, exchange_uniforms=rows,
                    n_exchanged=self.n_exchanged, walkers=self.walkers)

    def _run_chains(self, setup, x2, e, e_valid, launches, traj=None, traj_e=None, tick=None):
        """x2 / e are working chains: every exchange so far is in them.  A run that ends with an exchange makes its last step a launch
        of its own, so that the counters before that exchange can be kept (``_take_back``)"""
        self._handed, self._before_last, self._applied_at = None, None, self.steps_done
        total = sum(steps for steps, _, _ in launches)
        ends = total > 0 and (self.steps_done + total) % self.exchange_every == 0
        if ends:
            launches = list(launches[:-1]) + _last_step_apart(launches[-1])
        self._run = [total, None]
        try:
            super()._run_chains(setup, x2, e, e_valid, launches, traj, traj_e, tick)
            self._before_last = self._run[1] if ends else None
        finally:
            self._run = None

    def _hand_out(self, state, x2, e):
        before, self._before_last = self._before_last, None
        self._handed = _HandedOut(state, x2, e, *before) if before is not None and self._exchange_due() else None

    def _take_back(self):
        """forget the working chains of the state handed out last; the exchange the kernel made in them after the run's last step, if
        it is still due for that state, leaves ``walkers``, ``n_exchanged`` and ``n_exchange_attempts`` with them"""
        handed, self._handed = self._handed, None
        if handed is not None and self._exchange_due():
            self.walkers, self.n_exchanged = handed.walkers, handed.n_exchanged
            self.n_exchange_attempts -= 1

    def _working_copy(self, state, B):
        handed = self._handed
        if handed is not None and handed.state is state:       # the state handed out last: its working chains have the due exchange
            self._handed, self._applied_at = None, self.steps_done
            return handed.x, handed.e, True
        state = self.apply_pending_exchange(state)
        self._handed = None
        return super()._working_copy(state, B)

    def _fused_forward(self, state, setup, n_steps):
        if n_steps <= 0 or (self.steps_done + n_steps) % self.exchange_every != 0:
            return super()._fused_forward(state, setup, n_steps)
        # the run ends with an exchange: the kernel records the last step's frame before it, and that frame is the state handed out
        plan, B, _ = setup
        x = state.__dict__["_data"].samples[0]
        y, e, e_valid = self._working_copy(state, B)
        pieces = _split(n_steps, MCMC_MAX_STEPS_PER_LAUNCH)
        frame = torch.empty((1,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        frame_e = torch.empty((1, B), dtype=torch.float32, device=x.device)
        self._run_chains(setup, y, e, e_valid, [(k, 0, 0) for k in pieces[:-1]] + [(pieces[-1], pieces[-1], 1)], frame, frame_e)
        out = _advanced_state(state, frame[0], frame_e[0])
        self._hand_out(out, y, e)
        return out


@dataclasses.dataclass
class _HandedOut:
    """What ``ReplicaExchangeMCMCStep`` keeps after a fused run that ended with an exchange: the state it handed out (the frame before
    that exchange), the working chains x [B, n d] / e [B] in which the kernel has made it, and ``walkers`` / ``n_exchanged`` as they were
    before it.  ``IterativeSampler`` and ``forward`` both register their runs here (``_hand_out``)."""
    state: object
    x: torch.Tensor
    e: torch.Tensor
    walkers: torch.Tensor
    n_exchanged: torch.Tensor


def _last_step_apart(launch):
    """the launch (steps, traj_every, frames) of ``_launch_plan`` as launches that record the same frames, the last of one step"""
    steps, every, frames = launch
    if not frames:
        return ([(steps - 1, 0, 0)] if steps > 1 else []) + [(1, 0, 0)]
    return (([((frames - 1) * every, every, frames - 1)] if frames > 1 else []) + ([(every - 1, 0, 0)] if every > 1 else [])
            + [(1, 1, 1)])


def _advanced_state(state, samples, energies):
    """``state.replace(samples=(samples,), energies=energies)`` for a state the fused path takes (default samples hook, no box vectors),
    without the deep copy of every field that ``as_dict`` makes"""
    data = dataclasses.replace(state.__dict__["_data"], samples=(samples,), energies=energies, energies_up_to_date=True, forces_up_to_date=False)
    new = SamplerState.__new__(SamplerState)
    new._dataclass, new.set_samples_hook, new._data = state._dataclass, state.set_samples_hook, data
    return new


# ---- the driver -----------------------------------------------------------------------------------------------------------------
class IterativeSampler(Sampler, torch.utils.data.Dataset):
    """Drives ``sampler_steps`` over a ``SamplerState`` (iterative.py:121-192): an iteration applies every step ``stride`` times;
    ``sample(n)`` returns the samples after each of n iterations, [n, B, ...]; ``n_burnin`` iterations run at construction;
    ``max_iterations`` bounds the iterations (``StopIteration`` beyond).  Also an iterable-style torch dataset.  ``return_hook``
    (keyword, as of the reference's ``Sampler``) post-processes the list of sampled tensors.

    With one fusable ``MCMCStep`` and the default ``extract_sample_hook`` an iteration is one launch of ``stride * n_steps`` steps and
    ``sample(n)`` has the kernel write the n states into the result (launches of at most ``MCMC_MAX_STEPS_PER_LAUNCH`` steps); the
    state's samples are then the last recorded frame.  The same holds for one fusable ``ReplicaExchangeMCMCStep``: the exchanges happen
    inside the launches, each after the frame of its step."""

    def __init__(
            self,
            sampler_state,
            sampler_steps,
            stride=1,
            n_burnin=0,
            max_iterations=None,
            extract_sample_hook=default_extract_sample_hook,
            progress_bar=lambda x: x,
            **kwargs
    ):
        return_hook = kwargs.pop("return_hook", lambda x: x)
        super().__init__(**kwargs)
        self.return_hook = return_hook
        if isinstance(sampler_state, torch.Tensor):
            sampler_state = SamplerState(samples=sampler_state)
        self.state = sampler_state
        self.sampler_steps = sampler_steps
        self.extract_sample_hook = extract_sample_hook
        self.progress_bar = progress_bar
        self.stride = stride
        self.max_iterations = max_iterations
        self.i = 0
        self._chains = None            # (state handed out last, x [B, n d], e [B]): the fused path's working buffers
        fused = self._fused_setup() if n_burnin > 0 else None
        if fused is not None:
            self._fused_iterations(n_burnin, False, fused)
        else:
            for _ in self.progress_bar(range(n_burnin)):
                self.state = next(self)

    def _fused_setup(self):
        """(step, setup) if the iterations run inside the kernel, else None"""
        steps = self.sampler_steps
        if self.extract_sample_hook is not default_extract_sample_hook or not isinstance(steps, (list, tuple)) or len(steps) != 1:
            return None
        step = steps[0]
        base = ReplicaExchangeMCMCStep if isinstance(step, ReplicaExchangeMCMCStep) else MCMCStep
        if not isinstance(step, MCMCStep) or type(step).forward is not base.forward or type(step)._step is not base._step:
            return None
        if not (isinstance(self.stride, int) and self.stride >= 1 and isinstance(step._n_steps, int) and step._n_steps >= 1):
            return None
        setup = step._fused_setup(self.state)
        return None if setup is None else (step, setup)

    def _fused_iterations(self, n, record, fused, show=True):
        """n iterations inside the kernel (fused = ``_fused_setup()``); returns the [n, B, ...] frames if ``record``, else only
        advances the state.  ``show``: ``progress_bar`` is handed ``range(n)`` as on the general path and advanced, after every launch,
        by the iterations that launch completed (the launches are asynchronous: the bar shows what is enqueued)"""
        step, setup = fused
        n_ok = n if self.max_iterations is None else max(0, min(n, self.max_iterations - self.i))
        x = self.state.__dict__["_data"].samples[0]
        B, dev = x.shape[0], x.device
        frames = None
        if n_ok > 0:
            chains = self._chains
            if chains is None or chains[0] is not self.state:          # a state from outside: take a working copy of it
                chains = [None, *step._working_copy(self.state, B)]
            else:
                chains = [None, chains[1], chains[2], True]
            unit = self.stride * step._n_steps
            cap = step._launch_cap()
            launches = _launch_plan(unit, n_ok, cap) if record else _launch_plan(unit * n_ok, 1, cap)
            n_frames = n_ok if record else 1
            frames = torch.empty((n_frames,) + tuple(x.shape), dtype=torch.float32, device=dev)
            frames_e = torch.empty((n_frames, B), dtype=torch.float32, device=dev)
            bar, shown = (iter(self.progress_bar(range(n_ok))) if show else None), [0]

            def tick(steps_done):
                while bar is not None and shown[0] < steps_done // unit:
                    next(bar, None)
                    shown[0] += 1

            step._run_chains(setup, chains[1], chains[2], chains[3], launches, frames, frames_e, tick)
            for _ in (bar or ()):                                       # let the bar finish
                pass
            self.state = _advanced_state(self.state, frames[-1], frames_e[-1])
            self._chains = (self.state, chains[1], chains[2])
            step._hand_out(self.state, chains[1], chains[2])
            self.i += n_ok
        if n_ok < n:
            raise StopIteration
        return frames

    def _sample(self, n_samples, *args, **kwargs):
        fused = self._fused_setup() if n_samples > 0 else None
        if fused is not None:
            return [self._fused_iterations(n_samples, True, fused)]
        samples = None
        for _ in self.progress_bar(range(n_samples)):
            self.state = next(self)
            new_samples = self.extract_sample_hook(self.state)
            if samples is None:
                samples = [x[None, ...].clone() for x in new_samples]     # add the batch dimension
            else:
                for i, (x, new) in enumerate(zip(samples, new_samples)):
                    samples[i] = torch.cat((x, new[None, ...]), dim=0)
        return samples

    def sample(self, n_samples, temperature=1.0, *args, **kwargs):
        samples = pack_tensor_in_list(super().sample(n_samples, temperature, *args, **kwargs))
        return unpack_tensor_tuple(self.return_hook(samples))

    def __iter__(self):
        return self

    def __next__(self):
        if self.max_iterations is not None and self.i >= self.max_iterations:
            raise StopIteration
        fused = self._fused_setup()
        if fused is not None:
            self._fused_iterations(1, False, fused, show=False)
            return self.state
        for _ in range(self.stride):
            for sampler_step in self.sampler_steps:
                self.state = sampler_step.forward(self.state)
        self.i += 1
        return self.state


class GaussianMCMCSampler(IterativeSampler):
    """Shortcut for a Gaussian Metropolis sampler (mcmc.py:125-189): ``box_constraint`` is applied whenever samples are set, the default
    ``return_hook`` combines the sample and batch dimensions, ``n_stride`` is the deprecated spelling of ``stride``."""

    def __init__(
            self,
            energy,
            init_state,
            temperature=1.,
            noise_std=.1,
            stride=1,
            n_burnin=0,
            box_constraint=None,
            return_hook=None,
            **kwargs
    ):
        set_samples_hook = default_set_samples_hook
        if box_constraint is not None:
            set_samples_hook = lambda samples: [box_constraint(x) for x in samples]     # noqa: E731
        if not isinstance(init_state, SamplerState):
            init_state = SamplerState(samples=init_state, set_samples_hook=set_samples_hook)
        if return_hook is None:
            return_hook = lambda samples: [x.reshape(-1, *shape) for x, shape in zip(samples, energy.event_shapes)]     # noqa: E731
        if "n_stride" in kwargs:
            warnings.warn("keyword n_stride is deprecated, use stride instead", DeprecationWarning)
            stride = kwargs["n_stride"]
        super().__init__(
            init_state,
            sampler_steps=[MCMCStep(energy, proposal=GaussianProposal(noise_std=noise_std), target_temperatures=temperature)],
            stride=stride,
            n_burnin=n_burnin,
            return_hook=return_hook
        )


class HamiltonianMCSampler(IterativeSampler):
    """Shortcut for a Hamiltonian Monte Carlo sampler in the manner of ``GaussianMCMCSampler``: one ``HMCStep``; ``box_constraint`` is
    applied whenever samples are set, the default ``return_hook`` combines the sample and batch dimensions.  Further keywords are
    ``IterativeSampler``'s."""

    def __init__(
            self,
            energy,
            init_state,
            temperature=1.,
            step_size=.01,
            n_leapfrog=10,
            mass=1.,
            stride=1,
            n_burnin=0,
            box_constraint=None,
            return_hook=None,
            **kwargs
    ):
        set_samples_hook = default_set_samples_hook
        if box_constraint is not None:
            set_samples_hook = lambda samples: [box_constraint(x) for x in samples]     # noqa: E731
        if not isinstance(init_state, SamplerState):
            init_state = SamplerState(samples=init_state, set_samples_hook=set_samples_hook)
        if return_hook is None:
            return_hook = lambda samples: [x.reshape(-1, *shape) for x, shape in zip(samples, energy.event_shapes)]     # noqa: E731
        super().__init__(
            init_state,
            sampler_steps=[HMCStep(energy, step_size, n_leapfrog=n_leapfrog, mass=mass, target_temperatures=temperature)],
            stride=stride,
            n_burnin=n_burnin,
            return_hook=return_hook,
            **kwargs
        )


class ReplicaExchangeSampler(IterativeSampler):
    """Shortcut for a parallel-tempering sampler in the manner of ``GaussianMCMCSampler``: ``init_state`` holds B = L K chains,
    ladder-major, K = len(temperatures); one ``ReplicaExchangeMCMCStep`` with a ``GaussianProposal(noise_std)`` and an exchange attempt
    after every ``exchange_every``-th step.  Further keywords are ``IterativeSampler``'s."""

    def __init__(self, energy, init_state, temperatures, noise_std=.1, stride=1, n_burnin=0, exchange_every=1, **kwargs):
        if not isinstance(init_state, SamplerState):
            init_state = SamplerState(samples=init_state)
        step = ReplicaExchangeMCMCStep(energy, temperatures, proposal=GaussianProposal(noise_std=noise_std), exchange_every=exchange_every)
        super().__init__(init_state, sampler_steps=[step], stride=stride, n_burnin=n_burnin, **kwargs)
