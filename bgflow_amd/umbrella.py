"""Umbrella sampling along one reaction coordinate and its binless WHAM / MBAR estimate (distribution/sampling/_mcmc/umbrella_sampling.py,
with ``MetropolisGauss`` of distribution/sampling/_mcmc/metropolis.py as the sampler its loop expects).

``UmbrellaModel`` / ``UmbrellaSampling`` keep the reference's constructors, attributes and loop.  ``mbar_solve`` is the estimator the
reference takes from pyemma (not a dependency of this package): the self-consistent iteration for the window free energies f [K] over K
harmonic windows b_k(r) = kappa_k (r - m_k)^2, kappa_k = k_k / temperature (DESIGN.md "Umbrella sampling and MBAR"):

    D_n  = log sum_l N_l exp(f_l - b_l(r_n))        W_nk = N_k exp(f_k - b_k(r_n) - D_n)        S_k = sum_n W_nk
    f_k <- f_k - (log S_k - log N_k), then every f_k minus the new f_0;   err = max_k |f_k_new - f_k_old|

until err <= tolerance (status ``CONVERGED``), ``maximum_iterations`` (``BUDGET``: the last iterate is returned) or a NaN err
(``NOT_A_NUMBER``: a NaN or infinite sample gets there).  -D_n are the log weights that take every sample to the unbiased ensemble.  Two
paths run this ONE iteration:

* kernel (csrc/bgk_mbar.hip): a list of contiguous 1-d f32 / f64 tensors of one dtype on one HIP device, K <= ``MAX_WINDOWS``.  An
  iteration is two launches (block partials of the S_k, then merge + update of f on the device); the host enqueues ``MBAR_CHUNK``
  iterations per call and reads the 8-double record back once per chunk.
* torch: the same steps as f64 torch ops over slices of ``TORCH_CHUNK_ELEMENTS / K`` samples (neither path ever holds [K, N]), err read
  back every iteration: numpy arrays, CPU tensors, other dtypes, more windows.

``UmbrellaSampling.for_box`` is the on-device route for the particle box: a harmonic umbrella on the dimer distance is the box energy with
other dimer coefficients (``biased_system``), so every umbrella runs on the unchanged fused chain kernel through ``GaussianMCMCSampler``.

Deviations from the reference:

* ``UmbrellaModel`` is callable (``model(x)`` = ``model.energy(x)``): the reference's loop assigns the model itself to
  ``sampler.energy_function``, which its ``MetropolisGauss`` then calls -- a TypeError there.
* ``umbrella_free_energies`` takes ``bar`` from ``bgflow_amd.analysis``; the reference imports it from ``deep_boltzmann``, which does not
  exist.  ``save`` / ``load`` use ``numpy.savez`` for the same reason.
* ``mbar`` needs no pyemma; its ``F`` is -log of the normalised unbiased weight of every ``np.digitize`` state, empty states +inf.
* ``MetropolisGauss`` keeps the reference's single uniform number per step, shared by ALL walkers (metropolis.py:85): the walkers of one
  step accept or reject against the same threshold.  Kept, so that ``np.random.seed`` reproduces the reference's trajectories; the
  fused chain kernel (sampling.py) draws one per walker.  ``ReplicaExchangeMetropolisGauss`` (metropolis.py:138-188) is the numpy class
  with the reference's calls in the reference's order; the sampler for particle targets on the GPU is
  ``sampling.ReplicaExchangeMCMCStep``.  ``SystemWrapper`` is not ported."""
from collections import namedtuple

import numpy as np
import torch

from . import _driver, _lib
from ._driver import BUDGET, CONVERGED, NOT_A_NUMBER, R_STATUS      # NO_ROOT cannot happen here
from ._driver import DTYPE_CODES as _DTYPE_CODES
from .analysis import bar
from .particles import HarmonicParticles, RepulsiveParticles
from .sampling import GaussianMCMCSampler

__all__ = ["UmbrellaModel", "UmbrellaSampling", "MetropolisGauss", "ReplicaExchangeMetropolisGauss", "mbar_solve", "MBARResult",
           "biased_system"]

MBARResult = namedtuple("MBARResult", ["f", "log_weights", "status", "iterations", "err"])

MBAR_CHUNK = 32                # iterations enqueued per host read-back of the record (kernel path)
MAX_WINDOWS = 256              # the kernel's envelope (one stage-2 thread per window); more windows take the torch path
MAX_BLOCKS = 512               # stage-1 blocks (2 per CU)
SAMPLES_PER_BLOCK = 1024       # one LDS tile of the kernel
TORCH_CHUNK_ELEMENTS = 1 << 22  # elements of the [samples, K] slices of the torch path

# the device record (f64), csrc/bgk_mbar.hip / include/bgflow_amd.h
RECORD_DOUBLES = 8
R_N_ITER, R_ERR, R_K, R_N = range(2, 6)      # after R_PHASE, R_STATUS
PHASE_DONE = 1


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------
def _log_denominators(rc, c, kappa, m, sums=None):
    """D_n [N] (f64) for the pooled samples ``rc`` at c_l = log N_l + f_l, slice by slice; ``sums`` [K]: S_k is added to it"""
    K, N = c.numel(), rc.numel()
    step = max(1, TORCH_CHUNK_ELEMENTS // K)
    D = torch.empty(N, dtype=torch.float64, device=rc.device)
    for s in range(0, N, step):
        r = rc[s:s + step].to(torch.float64)
        a = c[None, :] - kappa[None, :] * (r[:, None] - m[None, :]) ** 2
        D[s:s + step] = torch.logsumexp(a, 1)
        if sums is not None:
            sums += torch.exp(a - D[s:s + step, None]).sum(0)
    return D


def _mbar_torch(rc, table, maximum_iterations, tolerance):
    """the iteration of csrc/bgk_mbar.hip in torch ops; rc: the pooled samples [N], table [K, 3] f64 = {m, kappa, log N} on rc's device"""
    m, kappa, logN = table[:, 0], table[:, 1], table[:, 2]
    f = torch.zeros_like(m)
    iterations = 0
    with torch.no_grad():
        while True:
            S = torch.zeros_like(m)
            _log_denominators(rc, logN + f, kappa, m, sums=S)
            f_new = f - (torch.log(S) - logN)
            f_new = f_new - f_new[0]
            err = float((f_new - f).abs().max())
            f = f_new
            iterations += 1
            if err != err:
                status = NOT_A_NUMBER
            elif err <= tolerance:
                status = CONVERGED
            elif iterations >= maximum_iterations:
                status = BUDGET
            else:
                continue
            break
        return MBARResult(f, -_log_denominators(rc, logN + f, kappa, m), status, iterations, err)


def _blocks(n):
    return max(1, min(MAX_BLOCKS, -(-n // SAMPLES_PER_BLOCK)))


def _mbar_kernel(rc, table, maximum_iterations, tolerance, f0=None, n_blocks=None, chunk=None):
    """the kernel path; rc: the pooled samples, a contiguous 1-d f32 / f64 HIP tensor, table [K, 3] f64 on its device"""
    chunk = MBAR_CHUNK if chunk is None else int(chunk)
    dev, n, K = rc.device, rc.numel(), table.shape[0]
    nb = _blocks(n) if n_blocks is None else int(n_blocks)
    table = table.contiguous()
    f = torch.zeros(K, dtype=torch.float64, device=dev) if f0 is None else f0.to(device=dev, dtype=torch.float64).clone()
    partial = torch.empty(nb * K, dtype=torch.float64, device=dev)
    code = _DTYPE_CODES[rc.dtype]

    def enqueue(record, n_steps):
        return _lib.lib().bgk_mbar_solve_steps(_lib.ptr(rc), n, code, _lib.ptr(table), K, nb, _lib.ptr(partial), _lib.ptr(f),
                                               _lib.ptr(record), maximum_iterations, tolerance, n_steps, _lib.stream_ptr(dev))

    _, host, _ = _driver.solve_record(enqueue, RECORD_DOUBLES, PHASE_DONE, maximum_iterations, chunk, dev, "bgk_mbar_solve_steps",
                                      unit="iterations")
    log_weights = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_mbar_log_weights(_lib.ptr(rc), n, code, _lib.ptr(table), K, _lib.ptr(f), _lib.ptr(log_weights), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_mbar_log_weights")
    return MBARResult(f, log_weights, int(host[R_STATUS]), int(host[R_N_ITER]), float(host[R_ERR]))


def _kernel_eligible(trajs):
    return len(trajs) <= MAX_WINDOWS and all(_driver.kernel_takes(t) for t in trajs) and _driver.same_kind(trajs)


def _window_table(counts, centers, force_constants, temperature, device):
    """[K, 3] f64 = {m_k, k_k / temperature, log N_k}"""
    table = np.stack([np.asarray(centers, np.float64), np.asarray(force_constants, np.float64) / float(temperature),
                      np.log(np.asarray(counts, np.float64))], axis=1)
    return torch.from_numpy(np.ascontiguousarray(table)).to(device)


def mbar_solve(rc_trajs, centers, force_constants, temperature=1.0, maximum_iterations=10000, tolerance=1e-10, path=None):
    """Window free energies and sample weights of K harmonic umbrella windows by binless WHAM / MBAR.

    rc_trajs: a list of K 1-d arrays or tensors, the reaction coordinate of window k's samples; centers [K]: m_k; force_constants: k_k
    (a scalar or [K]) of the bias k_k (r - m_k)^2, the reference's ``bias_energy``; temperature: the bias enters as k_k / temperature.
    Returns an ``MBARResult``: ``f`` [K] (f64, f[0] = 0), ``log_weights`` [N] (f64, -D_n for the samples in the order of
    ``concatenate(rc_trajs)``; softmax of them are the normalised unbiased weights), host numbers ``status`` (``CONVERGED``, ``BUDGET``:
    the last iterate, ``NOT_A_NUMBER``), ``iterations``, ``err``.  Tensors in, tensors on their device out; numpy in, numpy out.

    ``path``: None picks the kernel for contiguous 1-d f32 / f64 tensors of one dtype on one HIP device and K <= 256, the torch ops
    otherwise; "kernel" / "torch" force one ("kernel" raises ValueError for inputs it does not take)."""
    trajs = list(rc_trajs)
    K = len(trajs)
    centers = np.asarray(centers, np.float64).reshape(-1)
    force_constants = np.broadcast_to(np.asarray(force_constants, np.float64), (centers.size,)) if np.ndim(force_constants) == 0 \
        else np.asarray(force_constants, np.float64).reshape(-1)
    if K == 0 or centers.size != K or force_constants.size != K:
        raise ValueError(f"mbar_solve: {K} trajectories, {centers.size} centers, {force_constants.size} force constants")
    counts = [int(t.numel()) if isinstance(t, torch.Tensor) else int(np.size(t)) for t in trajs]
    if any(c == 0 for c in counts):
        raise ValueError(f"mbar_solve: window {counts.index(0)} has no samples")
    if not (np.all(np.isfinite(centers)) and np.all(np.isfinite(force_constants)) and float(temperature) > 0):
        raise ValueError("mbar_solve: centers and force constants must be finite, the temperature positive")
    maximum_iterations = int(maximum_iterations)
    if maximum_iterations <= 0:
        raise ValueError("mbar_solve: maximum_iterations must be positive")
    if not float(tolerance) >= 0:
        raise ValueError("mbar_solve: the tolerance must be a number >= 0")
    kernel = _driver.use_kernel(path, _kernel_eligible(trajs), "mbar_solve",
                                f"contiguous 1-d f32 or f64 tensors of one dtype on one HIP device, at most {MAX_WINDOWS} windows")
    tensors = isinstance(trajs[0], torch.Tensor)
    if tensors:
        if any(not isinstance(t, torch.Tensor) or t.device != trajs[0].device for t in trajs):
            raise ValueError("mbar_solve: the trajectories must be tensors on one device (or all numpy arrays)")
        rc = trajs[0].reshape(-1) if K == 1 else torch.cat([t.detach().reshape(-1) for t in trajs])
    else:
        rc = torch.from_numpy(np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in trajs]))
    table = _window_table(counts, centers, force_constants, temperature, rc.device)
    if kernel:
        return _mbar_kernel(rc.detach(), table, maximum_iterations, float(tolerance))
    r = _mbar_torch(rc.detach(), table, maximum_iterations, float(tolerance))
    return r if tensors else r._replace(f=r.f.numpy(), log_weights=r.log_weights.numpy())


# ---- the reference's classes -----------------------------------------------------------------------------------------------------------
class UmbrellaModel(object):
    """u(x) + k_umbrella (rc(x) - m_umbrella)^2 (umbrella_sampling.py:6-49); works on numpy arrays and on tensors alike, whatever the
    two callables take.  ``model(x)`` is ``model.energy(x)``."""

    def __init__(self, energy_function, rc_function, k_umbrella, m_umbrella):
        self.energy_function = energy_function
        self.rc_function = rc_function
        self.k_umbrella = k_umbrella
        self.m_umbrella = m_umbrella

    @classmethod
    def from_dict(cls, D):
        model = cls(None, None, D["k_umbrella"], D["m_umbrella"])
        if "rc_traj" in D:
            model.rc_traj = D["rc_traj"]
        return model

    def to_dict(self):
        D = {"k_umbrella": self.k_umbrella, "m_umbrella": self.m_umbrella}
        if hasattr(self, "rc_traj"):
            D["rc_traj"] = self.rc_traj
        return D

    def bias_energy(self, rc):
        return self.k_umbrella * (rc - self.m_umbrella) ** 2

    def energy(self, x):
        return self.energy_function(x) + self.bias_energy(self.rc_function(x))

    __call__ = energy


def biased_system(system, k, m):
    """A copy of a ``RepulsiveParticles`` / ``HarmonicParticles`` whose energy is the system's plus the harmonic umbrella
    k (d - m)^2 - k (dimer_dmid - m)^2 on the dimer distance d.  With t = 2 (d - dimer_dmid) the umbrella is k t^2 / 4 + k (dimer_dmid - m) t
    + const, so it is the same energy with ``dimer_slope + k (dimer_dmid - m)`` and ``dimer_a - k / 4``: the kernels of the box (energy,
    gradient, Metropolis chains) run it unchanged.  The copy has its own params dict; the original is not touched."""
    if not isinstance(system, RepulsiveParticles):
        raise TypeError(f"biased_system: a RepulsiveParticles or HarmonicParticles is expected, got {type(system).__name__}")
    params = dict(system.params)
    params["dimer_slope"] = params["dimer_slope"] + k * (params["dimer_dmid"] - m)
    params["dimer_a"] = params["dimer_a"] - k / 4
    if isinstance(system, HarmonicParticles):
        return type(system)(spring_constant=system.spring_constant, params=params)
    return type(system)(params)


class UmbrellaSampling(object):
    """A chain of harmonic umbrellas along a reaction coordinate (umbrella_sampling.py:52-228): ``n_umbrella`` windows with force constant
    ``k`` at equally spaced centres from ``m_min`` to ``m_max``, then back again if ``forward_backward``; every window is sampled from the
    last configuration of the one before.  ``sampler``: any object with ``reset(x0)``, ``run(nsteps=...)`` and ``traj`` whose
    ``energy_function`` attribute is called on configurations, e.g. ``MetropolisGauss``.  ``temperature`` (an attribute, 1.0 unless
    ``for_box`` sets it) divides the bias in ``mbar``."""

    def __init__(self, energy_function, sampler, rc_function, x0, n_umbrella, k, m_min, m_max, forward_backward=True):
        self.energy_function = energy_function
        self.sampler = sampler
        self.rc_function = rc_function
        self.x0 = x0
        self.forward_backward = forward_backward
        self.temperature = 1.0
        self._box = None
        self._solved = None
        d = (m_max - m_min) / (n_umbrella - 1)
        positions = [m_min + i * d for i in range(n_umbrella)]
        if forward_backward:
            positions += positions[::-1]
        self.umbrellas = [UmbrellaModel(energy_function, rc_function, k, m) for m in positions]

    @classmethod
    def for_box(cls, system, x0, n_umbrella, k, m_min, m_max, forward_backward=True, noise_std=0.1, temperature=1.0):
        """Umbrella sampling of a particle box along its dimer distance on the samples' device: ``system`` a ``RepulsiveParticles`` /
        ``HarmonicParticles``, ``x0`` [B, dim] one walker per row.  ``run`` drives one ``GaussianMCMCSampler`` per umbrella on
        ``biased_system(system, k, m)`` -- for contiguous f32 HIP samples the fused chain kernel."""
        if not isinstance(system, RepulsiveParticles):
            raise TypeError(f"for_box: a RepulsiveParticles or HarmonicParticles is expected, got {type(system).__name__}")
        if not (torch.is_tensor(x0) and x0.dim() == 2 and x0.shape[1] == system.dim):
            raise ValueError(f"for_box: x0 must be a [B, {system.dim}] tensor")
        us = cls(system, None, system.dimer_distance, x0, n_umbrella, k, m_min, m_max, forward_backward=forward_backward)
        us.temperature = temperature
        us._box = {"system": system, "noise_std": noise_std}
        return us

    def _run_box(self, nsteps, verbose, stride, burnin):
        system, x = self._box["system"], self.x0.detach()
        B = x.shape[0]
        for i, umbrella in enumerate(self.umbrellas):
            if verbose:
                print("Umbrella", i + 1, "/", len(self.umbrellas))
            target = biased_system(system, umbrella.k_umbrella, umbrella.m_umbrella)
            sampler = GaussianMCMCSampler(target, x.clone(), temperature=self.temperature, noise_std=self._box["noise_std"], stride=stride,
                                          n_burnin=burnin)
            with torch.no_grad():
                frames = sampler.sample(nsteps)                         # [nsteps * B, dim], frame-major
                umbrella.rc_traj = system.dimer_distance(frames)
            x = frames[-B:]

    def run(self, nsteps=10000, verbose=True, stride=1, burnin=0):
        """Sample every umbrella in turn.  With a sampler object (the reference's loop, :127-140): ``nsteps`` sampler steps per umbrella;
        ``stride`` and ``burnin`` are the sampler's own and must be left at their defaults here.  ``for_box``: ``nsteps`` recorded frames
        per walker and umbrella, ``stride`` chain steps apart, after ``burnin`` unrecorded iterations; ``rc_traj`` [nsteps * B] is a
        tensor on the samples' device."""
        self._solved = None
        if self._box is not None:
            return self._run_box(nsteps, verbose, stride, burnin)
        if stride != 1 or burnin != 0:
            raise ValueError("UmbrellaSampling.run: stride and burnin belong to the sampler object")
        xstart = self.x0
        for i, umbrella in enumerate(self.umbrellas):
            if verbose:
                print("Umbrella", i + 1, "/", len(self.umbrellas))
            self.sampler.energy_function = umbrella
            self.sampler.reset(xstart)
            self.sampler.run(nsteps=nsteps)
            traj = self.sampler.traj
            umbrella.rc_traj = self.rc_function(traj)
            xstart = np.array([traj[-1]])

    @property
    def rc_trajs(self):
        return [u.rc_traj for u in self.umbrellas]

    @property
    def bias_energies(self):
        return [u.bias_energy(u.rc_traj) for u in self.umbrellas]

    @property
    def umbrella_positions(self):
        return np.array([u.m_umbrella for u in self.umbrellas])

    def umbrella_free_energies(self):
        """the running sum of two-sample ``bar`` estimates between neighbouring umbrellas (:154-180), window i's force constant on both
        sides as in the reference"""
        free_energies = [0]
        for a, b in zip(self.umbrellas[:-1], self.umbrellas[1:]):
            k = a.k_umbrella
            a_ua, a_ub = k * (a.rc_traj - a.m_umbrella) ** 2, k * (a.rc_traj - b.m_umbrella) ** 2
            b_ua, b_ub = k * (b.rc_traj - a.m_umbrella) ** 2, k * (b.rc_traj - b.m_umbrella) ** 2
            free_energies.append(free_energies[-1] + bar(a_ub - a_ua, b_ua - b_ub))
        if any(torch.is_tensor(v) for v in free_energies):
            return torch.stack([torch.as_tensor(v, dtype=free_energies[-1].dtype, device=free_energies[-1].device) for v in free_energies])
        return np.array(free_energies)

    # -- MBAR
    def _solve(self):
        if self._solved is None:
            self._solved = mbar_solve(self.rc_trajs, self.umbrella_positions, [u.k_umbrella for u in self.umbrellas],
                                      temperature=self.temperature)
        return self._solved

    def _pooled(self):
        trajs = self.rc_trajs
        if torch.is_tensor(trajs[0]):
            return torch.cat([t.detach().reshape(-1) for t in trajs])
        return np.concatenate([np.asarray(t).reshape(-1) for t in trajs])

    def mbar(self, rc_min=None, rc_max=None, rc_bins=50):
        """Free energy along the reaction coordinate by binless WHAM / MBAR (:182-228).  rc_min, rc_max: the first and last grid point
        (None: the smallest and largest sample); rc_bins: the number of grid points.  The states are ``np.digitize``'s on
        ``np.linspace(rc_min, rc_max, rc_bins)``: 0 (below the grid) .. rc_bins (at or above its last point).  Returns numpy arrays
        ``(xgrid_mean, F)`` of rc_bins + 1 values: the states' positions (grid points shifted down by half a spacing, one appended) and
        -log of the normalised unbiased weight of each state, +inf for a state without samples; also kept as ``rc_discretization`` and
        ``rc_free_energies``.  The weights come from ``mbar_solve`` on the samples' device."""
        rc = self._pooled()
        if rc_min is None:
            rc_min = float(rc.min())
        if rc_max is None:
            rc_max = float(rc.max())
        xgrid = np.linspace(rc_min, rc_max, rc_bins)
        log_w = self._solve().log_weights
        if torch.is_tensor(rc):
            grid = torch.from_numpy(xgrid).to(rc.device)
            states = torch.bucketize(rc.to(torch.float64), grid, right=True)         # np.digitize(x, bins): bins[i - 1] <= x < bins[i]
            p = torch.zeros(rc_bins + 1, dtype=torch.float64, device=rc.device).index_add_(0, states, torch.softmax(log_w, 0))
            F = (-torch.log(p)).cpu().numpy()
        else:
            states = np.digitize(rc, xgrid)
            w = np.exp(log_w - log_w.max())
            p = np.bincount(states, weights=w / w.sum(), minlength=rc_bins + 1)
            with np.errstate(divide="ignore"):
                F = -np.log(p)
        xgrid_mean = np.concatenate([xgrid, [2 * xgrid[-1] - xgrid[-2]]])
        xgrid_mean -= 0.5 * (xgrid[1] - xgrid[0])
        self.rc_discretization = xgrid_mean
        self.rc_free_energies = F
        return xgrid_mean, F

    def mbar_weights(self):
        """The normalised unbiased weights of all samples (they sum to 1 over all windows) as a list with one entry per umbrella, shaped
        and typed like ``rc_trajs``: ``free_energy_bootstrap(rc_trajs, l, r, n, weights=mbar_weights())`` is the unbiased profile with
        error bars (bootstrap by trajectory; concatenate both lists to bootstrap by sample)."""
        trajs = self.rc_trajs
        log_w = self._solve().log_weights
        if torch.is_tensor(log_w):
            w = torch.softmax(log_w, 0).to(trajs[0].dtype)
            return list(torch.split(w, [t.numel() for t in trajs]))
        w = np.exp(log_w - log_w.max())
        w = (w / w.sum()).astype(np.asarray(trajs[0]).dtype)
        return np.split(w, np.cumsum([np.size(t) for t in trajs])[:-1])

    # -- files
    def save(self, filename):
        """the umbrellas (force constants, centres, recorded ``rc_traj``), ``forward_backward``, the temperature and the last ``mbar``
        profile as one ``numpy.savez`` archive"""
        arrays = {"k_umbrella": np.array([u.k_umbrella for u in self.umbrellas], np.float64), "m_umbrella": self.umbrella_positions,
                  "forward_backward": np.array(bool(self.forward_backward)), "temperature": np.array(float(self.temperature))}
        for i, u in enumerate(self.umbrellas):
            if hasattr(u, "rc_traj"):
                arrays[f"rc_traj_{i}"] = u.rc_traj.detach().cpu().numpy() if torch.is_tensor(u.rc_traj) else np.asarray(u.rc_traj)
        if hasattr(self, "rc_discretization"):
            arrays["rc_discretization"], arrays["rc_free_energies"] = self.rc_discretization, self.rc_free_energies
        np.savez(filename, **arrays)

    @classmethod
    def load(cls, filename):
        """what ``save`` wrote, as a data container (no energy function, sampler or start configuration); trajectories are numpy arrays"""
        name = str(filename)
        with np.load(name if name.endswith(".npz") else name + ".npz") as D:
            us = cls.__new__(cls)
            us.energy_function = us.sampler = us.rc_function = us.x0 = us._box = us._solved = None
            us.forward_backward = bool(D["forward_backward"])
            us.temperature = float(D["temperature"])
            us.umbrellas = []
            for i, (k, m) in enumerate(zip(D["k_umbrella"], D["m_umbrella"])):
                record = {"k_umbrella": float(k), "m_umbrella": float(m)}
                if f"rc_traj_{i}" in D:
                    record["rc_traj"] = D[f"rc_traj_{i}"]
                us.umbrellas.append(UmbrellaModel.from_dict(record))
            if "rc_discretization" in D:
                us.rc_discretization, us.rc_free_energies = D["rc_discretization"], D["rc_free_energies"]
        return us


class MetropolisGauss(object):
    """Metropolis Monte Carlo with Gaussian proposals on numpy arrays (metropolis.py:28-135): ``nwalkers`` copies of ``x0`` [1, dim]
    advance together; ``energy_function`` maps [nwalkers, dim] to [nwalkers]; ``mapper`` (optional) is applied to every proposal and to
    the start; a frame is kept whenever ``step > burnin`` and ``step % stride == 0``, and the start itself if ``burnin == 0``.
    ``temperature``: a number, or one per walker.

    The random calls are the reference's in the reference's order -- per step one ``np.random.randn(nwalkers, dim)``, then ONE
    ``np.random.rand()`` whose -log is the acceptance threshold of every walker of that step (module docstring) -- so ``np.random.seed``
    reproduces its trajectories."""

    def __init__(self, energy_function, x0, temperature=1.0, noise=0.1, burnin=0, stride=1, nwalkers=1, mapper=None):
        self.energy_function = energy_function
        self.noise = noise
        self.temperature = temperature
        self.burnin = burnin
        self.stride = stride
        self.nwalkers = nwalkers
        self.mapper = mapper
        self.reset(x0)

    def reset(self, x0):
        self.step = 0
        self.traj_, self.etraj_ = [], []
        self.x = np.tile(x0, (self.nwalkers, 1))
        if self.mapper is not None:
            self.x = self.mapper(self.x)
        self.E = self.energy_function(self.x)
        if self.burnin == 0:
            self._keep()

    def _keep(self):
        self.traj_.append(self.x)
        self.etraj_.append(self.E)

    def _proposal_step(self):
        self.x_prop = self.x + self.noise * np.random.randn(self.x.shape[0], self.x.shape[1])
        if self.mapper is not None:
            self.x_prop = self.mapper(self.x_prop)
        self.E_prop = self.energy_function(self.x_prop)

    def _acceptance_step(self):
        accept = -np.log(np.random.rand()) > (self.E_prop - self.E) / self.temperature
        self.x = np.where(accept[:, None], self.x_prop, self.x)
        self.E = np.where(accept, self.E_prop, self.E)

    def run(self, nsteps=1, verbose=0):
        for i in range(nsteps):
            self._proposal_step()
            self._acceptance_step()
            self.step += 1
            if verbose > 0 and i % verbose == 0:
                print("Step", i, "/", nsteps)
            if self.step > self.burnin and self.step % self.stride == 0:
                self._keep()

    @property
    def trajs(self):
        """one float32 trajectory [frames, dim] per walker"""
        T = np.array(self.traj_).astype(np.float32)
        return [T[:, i, :] for i in range(T.shape[1])]

    @property
    def traj(self):
        return self.trajs[0]

    @property
    def etrajs(self):
        """one energy trajectory [frames] per walker"""
        E = np.array(self.etraj_)
        return [E[:, i] for i in range(E.shape[1])]

    @property
    def etraj(self):
        return self.etrajs[0]


class ReplicaExchangeMetropolisGauss(object):
    """Parallel tempering on numpy arrays (metropolis.py:138-188): one ``MetropolisGauss`` walker per temperature (an ODD number of
    temperatures, as the reference demands; ``temperatures`` a numpy array), all started at ``x0``.  ``run`` makes ``nepochs`` epochs of
    ``nsteps_per_epoch`` Metropolis steps, each followed by an exchange attempt between the neighbours (k, k + 1), k = toggle, toggle + 2,
    ...: with c = -(E[k+1] - E[k]) (1 / T[k+1] - 1 / T[k]) the two swap configuration and energy iff -log(np.random.rand()) > c; then
    ``toggle`` flips.  One ``np.random.rand()`` per pair, in ascending k, after the epoch's steps: the reference's calls in its order."""

    def __init__(self, energy_function, x0, temperatures, noise=0.1, burnin=0, stride=1, mapper=None):
        if temperatures.size % 2 == 0:
            raise ValueError("Please use an odd number of temperatures.")
        self.temperatures = temperatures
        self.sampler = MetropolisGauss(energy_function, x0, temperature=temperatures, noise=noise, burnin=burnin, stride=stride,
                                       nwalkers=temperatures.size, mapper=mapper)
        self.toggle = 0

    @property
    def trajs(self):
        return self.sampler.trajs

    @property
    def etrajs(self):
        return self.sampler.etrajs

    def run(self, nepochs=1, nsteps_per_epoch=1, verbose=0):
        s, T = self.sampler, self.temperatures
        for _ in range(nepochs):
            s.run(nsteps=nsteps_per_epoch)
            for k in range(self.toggle, T.size - 1, 2):
                c = -(s.E[k + 1] - s.E[k]) * (1.0 / T[k + 1] - 1.0 / T[k])
                if -np.log(np.random.rand()) > c:
                    s.x[[k, k + 1]] = s.x[[k + 1, k]]
                    s.E[[k, k + 1]] = s.E[[k + 1, k]]
            self.toggle = 1 - self.toggle
