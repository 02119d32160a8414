"""Free-energy profiles along a reaction coordinate with bootstrap error bars (distribution/sampling/_mcmc/analysis.py).

``free_energy_bootstrap`` keeps the reference's signature (plus the keyword-only ``seed`` and ``indices``); ``bootstrap_histogram`` returns
the raw per-replicate weighted histograms and serves other observables.  Four paths (DESIGN.md "Bootstrap histogram"):

* numpy arrays (or a list of them) in: the reference's method on the host -- per replicate one ``np.random.choice`` and one
  density-normalised ``np.histogram`` -- numpy arrays out; ``np.random.seed`` reproduces the reference's numbers exactly.
* contiguous 1-d f32 / f64 tensors on one HIP device (``weights`` of the same dtype and device or None, nothing requires grad): the
  kernel (csrc/bgk_hist.hip).  One pass turns every sample into a {bin, weight} record, one launch draws the indices of every replicate
  with Philox and gathers the records into f64 histograms in LDS.  Replicates run in batches that keep the kernel's workspace below
  ``PARTIAL_BYTES``; the replicate number is part of the random counter, so the batching does not show in the result.
* a list / tuple of such tensors: bootstrap by trajectory as the reference does for a list -- one launch gives the per-trajectory
  histograms [T, nb], a replicate is the sum of T resampled rows; ``indices`` is then [sample, T].
* any other tensor input (CPU, other dtypes, non-contiguous, requiring grad): the same steps in torch ops in f64 (``bucketize`` on the f64
  edges with the closed last bin, ``index_add_``), with the same rules for dropped samples.

``seed=None`` draws a 64-bit seed from torch's global CPU generator (``torch.manual_seed`` reproduces a run).  Seeds are NOT portable
between the torch path and the kernel path (another generator); ``indices`` is.  Samples whose weight is NaN, infinite or negative are
dropped with one warning per call.

Deviations from the reference:

* ``n`` is the number of EDGES: the reference's docstring says bins, its code (``np.linspace(l, r, n)``) gives n - 1 bins; kept.
* ``std_finite(x, axis=None)`` returns the standard deviation; the reference returns the mean (it calls ``mean_finite_``).
* the ``axis`` variants of ``mean_finite`` / ``std_finite`` pass ``min_finite`` on; the reference drops it (same result at the default).
* a NaN weight drops its sample (tensor paths); numpy carries it into every later bin through its cumulative sum.
* a tuple of arrays or tensors is bootstrapped by trajectory like a list; the reference takes a list only.
* the tensor paths emit no divide-by-zero warning for empty bins, which are +inf as in numpy.
* ``free_energy_bootstrap_2BGs`` and the latent samplers are not part of this package; ``UmbrellaSampling`` and
  ``MetropolisGauss`` live in ``bgflow_amd/umbrella.py``, whose ``mbar_weights`` are ``weights`` for the functions here."""
import warnings

import numpy as np
import torch

from . import _driver, _lib
from ._driver import DTYPE_CODES as _DTYPE_CODES

__all__ = ["mean_finite_", "std_finite_", "mean_finite", "std_finite", "metropolis_function", "bar", "free_energy_bootstrap",
           "bootstrap_histogram"]

PARTIAL_BYTES = 64 << 20       # the kernel's partial[replicates, n_chunks, nb] workspace (f64) stays below this; replicates are batched
N_CHUNKS = None                # blocks per replicate; None: from (n, sample) by _n_chunks (tests set it)
MAX_BINS = 4096                # the kernel's envelope (LDS histogram); more bins take the torch path
MAX_CHUNKS = 512
MIN_DRAWS_PER_CHUNK = 4096     # 16 draws per thread
TARGET_BLOCKS = 2048           # 8 blocks per CU
TORCH_BATCH_ELEMENTS = 1 << 24  # gathered elements per batch of the torch path


# ---- statistics over finite values ---------------------------------------------------------------------------------------------------
def _finite_statistic(x, min_finite, numpy_fn, torch_fn):
    """a statistic of the finite entries of an array or tensor; NaN unless MORE than ``min_finite`` entries are finite"""
    tensor = isinstance(x, torch.Tensor)
    keep = torch.isfinite(x) if tensor else np.isfinite(x)
    if int(keep.sum()) <= min_finite:
        return x.new_tensor(float("nan")) if tensor else np.nan
    return (torch_fn if tensor else numpy_fn)(x[keep])


def mean_finite_(x, min_finite=1):
    """mean over the finite values"""
    return _finite_statistic(x, min_finite, np.mean, torch.mean)


def std_finite_(x, min_finite=2):
    """standard deviation over the finite values, population form (as np.std)"""
    return _finite_statistic(x, min_finite, np.std, lambda v: v.std(unbiased=False))


def _along(fn, x, axis, min_finite):
    if axis is None:
        return fn(x, min_finite)
    if axis == 0 or axis == 1:
        vals = [fn(x[:, i] if axis == 0 else x[i], min_finite) for i in range(x.shape[axis - 1])]
        if isinstance(x, torch.Tensor):
            return torch.stack([torch.as_tensor(v, dtype=torch.float64, device=x.device) for v in vals]) if vals else x.new_zeros(0)
        return np.array(vals, dtype=np.float64).reshape(len(vals))
    raise NotImplementedError("axis value not implemented:", axis)


def mean_finite(x, axis=None, min_finite=1):
    return _along(mean_finite_, x, axis, min_finite)


def std_finite(x, axis=None, min_finite=2):
    return _along(std_finite_, x, axis, min_finite)


def metropolis_function(x):
    if isinstance(x, torch.Tensor):
        return torch.clamp(torch.exp(-x), max=1.0)
    return np.minimum(np.exp(-x), 1)


def bar(sampled_a_uab, sampled_b_uba):
    """-log of the ratio of mean Metropolis acceptances: ``sampled_a_uab`` = Ub - Ua on samples of A, ``sampled_b_uba`` = Ua - Ub on
    samples of B (the reference's two-line estimator; ``bennett_acceptance_ratio`` is the self-consistent one)"""
    R = metropolis_function(sampled_a_uab).mean() / metropolis_function(sampled_b_uba).mean()
    return -torch.log(R) if isinstance(R, torch.Tensor) else -np.log(R)


# ---- histograms ----------------------------------------------------------------------------------------------------------------------
def _draw_seed():
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & (2 ** 64 - 1)


def _host_generator(seed):
    return torch.Generator().manual_seed(int(seed) & (2 ** 64 - 1))


def _kernel_eligible(D, W):
    def one(t):
        return _driver.kernel_takes(t) and t.numel() >= 1
    if not (all(one(d) for d in D) and _driver.same_kind(D)):
        return False
    return W is None or all(one(w) and _driver.same_kind((d, w)) and w.shape == d.shape for d, w in zip(D, W))


def _n_chunks(n, sample):
    if N_CHUNKS is not None:
        return int(N_CHUNKS)
    want = -(-TARGET_BLOCKS // max(1, sample))
    return max(1, min(MAX_CHUNKS, want, -(-n // MIN_DRAWS_PER_CHUNK)))


def _as_indices(indices, rows, cols, device):
    idx = torch.as_tensor(indices, device=device).to(torch.int64).contiguous()
    if idx.shape != (rows, cols):
        raise ValueError(f"indices has shape {tuple(idx.shape)}, expected ({rows}, {cols})")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= cols):
        raise ValueError(f"indices outside [0, {cols})")
    return idx


def _hist_kernel(d, w, edges, sample, seed, indices=None, segments=None):
    """the kernel path: [sample, nb] f64 sums and the two drop counts (int64 [2]) on d's device; ``segments``: offsets [sample + 1] into
    d, one plain histogram per segment"""
    dev, n, nb = d.device, d.numel(), edges.size - 1
    edges_t = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(dev)
    records = torch.empty(2 * n, dtype=d.dtype, device=dev)
    out = torch.empty((sample, nb), dtype=torch.float64, device=dev)
    n_ignored = torch.empty(2, dtype=torch.int64, device=dev)          # zeroed by the call
    if sample == 0:
        return out, n_ignored.zero_()
    n_chunks = _n_chunks(n if segments is None else max(1, n // max(1, sample)), sample)
    per_call = max(1, min(int(PARTIAL_BYTES) // (n_chunks * nb * 8), (2 ** 31 - 1) // n_chunks))
    partial = torch.empty(min(per_call, max(sample, 1)) * n_chunks * nb, dtype=torch.float64, device=dev)
    seg_t = None if segments is None else torch.as_tensor(segments, dtype=torch.int64).to(dev)
    fn = _lib.lib().bgk_bootstrap_histogram
    for r0 in range(0, sample, per_call):
        reps = min(per_call, sample - r0)
        idx = None if indices is None else indices[r0:r0 + reps]
        seg = None if seg_t is None else seg_t[r0:r0 + reps + 1]
        with torch.cuda.device(dev):
            st = fn(_lib.ptr(d), _lib.ptr(w), n, _DTYPE_CODES[d.dtype], _lib.ptr(edges_t), nb, reps, r0, _lib.ptr(idx), _lib.ptr(seg),
                    0 if seed is None else int(seed), 0, n_chunks, _lib.ptr(records), _lib.ptr(partial), _lib.ptr(out[r0:r0 + reps]), _lib.ptr(n_ignored),
                    _lib.stream_ptr(dev))
        _lib.check(st, "bgk_bootstrap_histogram")
    return out, n_ignored


def _digitize_torch(d, w, edges_t):
    """(bin [n] int64 with dropped samples at 0, weight [n] f64 with dropped samples at 0, drop counts int64 [2])"""
    nb = edges_t.numel() - 1
    d = d.detach().reshape(-1).to(torch.float64)
    valid = (d >= edges_t[0]) & (d <= edges_t[-1])                    # (a NaN: False)
    bins = torch.bucketize(d, edges_t, right=True) - 1                 # e[i] <= x < e[i + 1] -> i;  x == e[nb] -> nb
    bins = bins.clamp(0, nb - 1)
    wt = torch.ones_like(d) if w is None else w.detach().reshape(-1).to(torch.float64)
    if wt.shape != d.shape:
        raise ValueError(f"weights of {wt.numel()} values for {d.numel()} samples")
    bad_w = valid & ~(torch.isfinite(wt) & (wt >= 0))
    keep = valid & ~bad_w
    zero_w, zero_b = torch.zeros_like(wt), torch.zeros_like(bins)
    return torch.where(keep, bins, zero_b), torch.where(keep, wt, zero_w), torch.stack([(~valid).sum(), bad_w.sum()])


def _hist_torch(d, w, edges, sample, seed, indices=None, segments=None):
    """the torch-op path of _hist_kernel, f64 on d's device"""
    dev = d.device
    edges_t = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(dev)
    nb = edges_t.numel() - 1
    bins, wt, n_ignored = _digitize_torch(d, w, edges_t)
    n = bins.numel()
    out = torch.zeros(sample * nb, dtype=torch.float64, device=dev)
    if segments is not None:
        lengths = torch.as_tensor(np.diff(np.asarray(segments, dtype=np.int64)), device=dev)
        row = torch.repeat_interleave(torch.arange(sample, device=dev), lengths)
        out.index_add_(0, row * nb + bins, wt)
        return out.reshape(sample, nb), n_ignored
    gen = None if indices is not None else torch.Generator(device=dev).manual_seed(int(seed) & (2 ** 64 - 1))      # torch's generator of d's device
    per = max(1, TORCH_BATCH_ELEMENTS // max(n, 1))
    for r0 in range(0, sample, per):
        reps = min(per, sample - r0)
        idx = indices[r0:r0 + reps] if indices is not None else torch.randint(n, (reps, n), generator=gen, device=dev)
        row = torch.arange(r0, r0 + reps, device=dev)[:, None] * nb
        out.index_add_(0, (row + bins[idx]).reshape(-1), wt[idx].reshape(-1))
    return out.reshape(sample, nb), n_ignored


def _check_edges(edges):
    edges = np.asarray(edges.detach().cpu() if isinstance(edges, torch.Tensor) else edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("bin edges: a 1-d array of at least 2 values")
    if not (np.all(np.isfinite(edges)) and np.all(np.diff(edges) >= 0) and edges[-1] > edges[0]):
        raise ValueError("bin edges must be finite and increase monotonically")
    return edges


def _histograms(D, edges, sample, weights, seed, indices):
    """raw sums [sample, nb] (f64 tensor on D's device) and the drop counts (int64 [2] tensor) for tensor input"""
    edges = _check_edges(edges)
    sample = int(sample)
    if sample < 0:
        raise ValueError("sample must not be negative")
    by_traj = isinstance(D, (list, tuple))
    Ds = list(D) if by_traj else [D]
    Ws = None if weights is None else (list(weights) if by_traj else [weights])
    if not Ds or any(not isinstance(t, torch.Tensor) for t in Ds + (Ws or [])):
        raise TypeError("tensor input expected (a tensor or a list of tensors, weights alike)")
    if Ws is not None and (len(Ws) != len(Ds) or any(w.numel() != d.numel() for d, w in zip(Ds, Ws))):
        raise ValueError("weights do not match D")
    if any(d.numel() == 0 for d in Ds):
        raise ValueError("empty sample array")
    if seed is None and indices is None:
        seed = _draw_seed()
    kernel = _kernel_eligible(Ds, Ws) and edges.size - 1 <= MAX_BINS
    hist = _hist_kernel if kernel else _hist_torch
    dev = Ds[0].device
    if not by_traj:
        d, w = Ds[0], None if Ws is None else Ws[0]
        if not kernel:
            d, w = d.reshape(-1), None if w is None else w.reshape(-1)
        idx = None if indices is None else _as_indices(indices, sample, d.numel(), dev)
        return hist(d, w, edges, sample, seed, indices=idx)
    # by trajectory: per-trajectory histograms, then sums of resampled rows
    T = len(Ds)
    d = torch.cat([t.reshape(-1) for t in Ds])
    w = None if Ws is None else torch.cat([t.reshape(-1) for t in Ws])
    segments = np.concatenate([[0], np.cumsum([t.numel() for t in Ds])]).astype(np.int64)
    H, n_ignored = hist(d, w, edges, T, 0, segments=segments)
    idx = _as_indices(indices, sample, T, dev) if indices is not None else torch.randint(T, (sample, T), generator=_host_generator(seed)).to(dev)
    return H[idx].sum(1), n_ignored


def _warn_dropped(n_ignored, what):
    dropped = int(n_ignored.tolist()[1])
    if dropped:
        warnings.warn(f"{what}: {dropped} samples have a NaN, infinite or negative weight; they are dropped", stacklevel=3)


def bootstrap_histogram(D, edges, sample, weights=None, *, seed=None, indices=None, return_ignored=False):
    """``sample`` bootstrap replicates of the weighted histogram of ``D`` over the bin ``edges`` (np.histogram's bins: half-open, the last
    one closed): raw sums [sample, len(edges) - 1] as an f64 tensor on ``D``'s device.  ``D``: a tensor, or a list / tuple of tensors
    (bootstrap by trajectory); ``indices``: the replicates' source indices [sample, len(D)] instead of random draws; ``return_ignored``:
    also return the int64 pair (samples dropped for their value -- outside the edges, NaN, infinite --, samples dropped for their
    weight)."""
    sums, n_ignored = _histograms(D, edges, sample, weights, seed, indices)
    _warn_dropped(n_ignored, "bootstrap_histogram")
    return (sums, n_ignored) if return_ignored else sums


def _finish_profiles(profiles, centres, bias, temperature):
    """-log densities [sample, nb] (numpy or torch, in place) -> free energies: zero at the lowest replicate-mean, the bias taken off"""
    profiles -= profiles.mean(0).min()
    if bias is not None:
        profiles -= bias(centres) / temperature
    return centres, profiles


def _resample(values, picks, by_trajectory):
    return np.concatenate([values[i] for i in picks]) if by_trajectory else values[picks]


def _free_energy_bootstrap_numpy(D, l, r, n, sample, weights, bias, temperature, seed, indices):
    """numpy in, numpy out, on the host.  Per replicate: ``len(D)`` picks among the samples (or trajectories), one density-normalised
    ``np.histogram`` of what they select, ``-log``.  The picks are ``np.random.choice(arange(len(D)), size=len(D), replace=True)`` on
    numpy's global state when neither ``seed`` nor ``indices`` is given -- the reference's one random call per replicate, so
    ``np.random.seed`` reproduces its numbers; histogram and normalisation are numpy's in either implementation."""
    edges = np.linspace(l, r, n)
    by_trajectory = isinstance(D, (list, tuple))
    population = np.arange(len(D))
    choice = np.random.choice if seed is None else np.random.RandomState(int(seed) % 2 ** 32).choice
    profiles = np.empty((sample, n - 1))
    for s in range(sample):
        picks = np.asarray(indices[s]) if indices is not None else choice(population, size=len(D), replace=True)
        w = None if weights is None else _resample(weights, picks, by_trajectory)
        density, _ = np.histogram(_resample(D, picks, by_trajectory), bins=edges, weights=w, density=True)
        profiles[s] = -np.log(density)
    return _finish_profiles(profiles, 0.5 * (edges[:-1] + edges[1:]), bias, temperature)


def free_energy_bootstrap(D, l, r, n, sample=100, weights=None, bias=None, temperature=1.0, *, seed=None, indices=None):
    """Bootstrapped free-energy profile -log p along a coordinate (analysis.py:73-132).

    D: samples of the coordinate -- one array / tensor (bootstrap by sample) or a list of them (bootstrap by trajectory);
    l, r: leftmost and rightmost bin boundary; n: number of bin EDGES (``np.linspace(l, r, n)``: n - 1 bins, as the reference's code);
    sample: number of bootstrap replicates; weights: None or sample weights matching D; bias: callable of the bin centres whose value /
    temperature is subtracted; seed: 64-bit seed of the resampling (None: from torch's global CPU generator; numpy input with None uses
    ``np.random`` as the reference does); indices: the replicates' source indices [sample, len(D)] instead of random draws.

    Returns ``(bin_means [n - 1], Es [sample, n - 1])``: the bin centres and, per replicate, the free energies of the bins, shifted so
    that the lowest replicate-mean is zero; empty bins are +inf.  numpy in, numpy out; tensors in, f64 tensors on D's device out (module
    docstring: the paths and the deviations from the reference)."""
    first = D[0] if isinstance(D, (list, tuple)) and len(D) > 0 else D
    if not isinstance(first, torch.Tensor):
        return _free_energy_bootstrap_numpy(D, l, r, n, sample, weights, bias, temperature, seed, indices)
    edges = np.linspace(l, r, n)
    sums, n_ignored = _histograms(D, edges, sample, weights, seed, indices)
    _warn_dropped(n_ignored, "free_energy_bootstrap")
    dev = sums.device
    widths = torch.from_numpy(np.diff(edges)).to(dev)
    density = (sums / widths) / sums.sum(1, keepdim=True)             # numpy's order of operations
    centres = torch.from_numpy(0.5 * (edges[:-1] + edges[1:])).to(dev)
    return _finish_profiles(-torch.log(density), centres, bias, temperature)
