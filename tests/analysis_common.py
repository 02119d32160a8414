"""Shared by test_host_analysis.py and test_gpu_analysis.py: the cases of tests/golden/analysis.npz (written by
tests/golden/make_analysis_goldens.py from the reference), the bounds, the kernel's index stream restated with
``oracle.philox.philox4x32_10`` and an exact (``math.fsum``) histogram.

Bounds, and where they come from:

* raw unweighted sums: sums of 1.0 in f64 are exact -- ``np.array_equal`` with the counts.
* raw weighted sums: |got - exact| <= m 2^-52 exact per bin, m the draws that landed in it.  A sum of m positive f64 terms in any order
  is within (m - 1) 2^-53 (relative); the factor 2 covers the chunk merge and the bound's second-order term.
* ``Es`` against the fixture on finite entries: atol = 4 N 2^-52 + 64 2^-52 max|Es|.  Numerator and denominator of the density each
  carry the sum bound (N draws at most), the shift by mean.min() carries it once more, the remainder is the torch-against-numpy rounding
  of the few f64 operations: 3.7e-12 at N = 4096, where a single misplaced unit-weight sample moves a bin by more than 1e-4.  For the
  trajectory case N is the largest number of draws a replicate can have (trajectories x the longest one).
* inf and nan positions identical; ``bin_means`` equal to 1 ulp."""
import json
import math

import numpy as np

from oracle.philox import philox4x32_10

EPS64 = 2.0 ** -52


def bias(x):
    return 3.0 * (x - 1.5) ** 2


def cases(G):
    return json.loads(str(G["cases"]))


CASE_NAMES = ["weighted", "unweighted", "bias", "f64", "offgrid", "empty", "trajs", "f32"]
NUMPY_CASE_NAMES = CASE_NAMES + ["f32w"]      # f32w: the reference's own f32 weight sums, for the numpy path alone (no f64 bound applies)


def case(G, name):
    """(D, W, idx [sample, len(D)] int64, spec) of a case: numpy arrays as stored (lists of arrays for ``trajs``), W None when unweighted"""
    spec = cases(G)[name]
    idx = G[f"{spec['idx']}_idx"].astype(np.int64)
    if name == "trajs":
        cuts = np.concatenate([[0], np.cumsum(G["trajs_lengths"])])
        D = [G["weighted_D"][a:z] for a, z in zip(cuts[:-1], cuts[1:])]
        W = [G["weighted_W"][a:z] for a, z in zip(cuts[:-1], cuts[1:])]
        return D, W, idx, spec
    return G[f"{name}_D"], (G[f"{name}_W"] if spec["weights"] else None), idx, spec


def widen(a):
    """the exact f64 widening of a case's stored arrays: what the fixture's reference run saw"""
    if a is None:
        return None
    return [v.astype(np.float64) for v in a] if isinstance(a, list) else a.astype(np.float64)


def case_kwargs(spec):
    kw = {"sample": spec["sample"]}
    if spec["bias"]:
        kw.update(bias=bias, temperature=spec["temperature"])
    return kw


def max_draws(D):
    return len(D) * max(len(d) for d in D) if isinstance(D, list) else len(D)


def sum_bound(m, exact):
    return m * EPS64 * exact


def es_atol(n_draws, Es):
    finite = np.isfinite(Es)
    return 4.0 * n_draws * EPS64 + 64.0 * EPS64 * (np.abs(Es[finite]).max() if finite.any() else 0.0)


def check_profile(G, name, bin_means, Es, n_draws, label=""):
    """(bin_means, Es) as numpy f64 against the fixture; prints the figures first"""
    want_bm, want = G[f"{name}_bin_means"], G[f"{name}_Es"]
    assert Es.shape == want.shape and Es.dtype == np.float64 and bin_means.dtype == np.float64
    finite = np.isfinite(want)
    atol = es_atol(n_draws, want)
    err = np.abs(Es[finite] - want[finite]).max() if finite.any() else 0.0
    print(f"{label}{name}: max |Es - fixture| {err:.3e} (bound {atol:.3e}), {int((~finite).sum())} non-finite entries")
    assert np.array_equal(np.isposinf(Es), np.isposinf(want)) and np.array_equal(np.isneginf(Es), np.isneginf(want))
    assert np.array_equal(np.isnan(Es), np.isnan(want))
    assert err <= atol
    assert np.all(np.abs(bin_means - want_bm) <= np.spacing(np.abs(want_bm)))


def np_bins(x, edges):
    """np.histogram's bin of every value on the f64 edges: half-open bins, the last one closed, -1 outside / NaN / inf"""
    x = np.asarray(x, dtype=np.float64)
    nb = len(edges) - 1
    with np.errstate(invalid="ignore"):
        inside = (x >= edges[0]) & (x <= edges[-1])
    b = np.searchsorted(edges, np.where(inside, x, edges[0]), side="right") - 1
    b = np.minimum(b, nb - 1)
    return np.where(inside, b, -1)


def philox_indices(seed, n, n_replicates, replicate0=0, offset=0):
    """the kernel's index stream [n_replicates, n] (int64): draw j of replicate R comes from call k = j // 2 at counter
    (k low, k high, R, offset), key = seed; words (o0, o1) = (low, high) for the even draw, (o2, o3) for the odd one;
    index = (r * n) >> 64 in exact integer arithmetic"""
    calls = (n + 1) // 2
    k = np.arange(calls, dtype=np.uint64)
    out = np.zeros((n_replicates, 2 * calls), dtype=np.int64)
    for s in range(n_replicates):
        R = replicate0 + s
        assert 0 <= R < 2 ** 32
        o = philox4x32_10([k & np.uint64(0xFFFFFFFF), k >> np.uint64(32), np.full(calls, R, np.uint64), np.full(calls, offset, np.uint64)],
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        for half in range(2):
            r = [(int(hi) << 32) | int(lo) for lo, hi in zip(o[2 * half], o[2 * half + 1])]
            out[s, half::2] = [(v * n) >> 64 for v in r]
    return out[:, :n]


def exact_histogram(bins, weights, idx, nb):
    """per replicate (row of ``idx``: an array, or a list of index arrays of any lengths) the exactly rounded sums (math.fsum) of the
    gathered weights per bin and the number of draws per bin: (sums [R, nb] f64, counts [R, nb] int64); ``weights`` None = 1.0 each;
    bin -1 is dropped"""
    sums = np.zeros((len(idx), nb), np.float64)
    counts = np.zeros((len(idx), nb), np.int64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    for s, row in enumerate(idx):
        b = bins[row]
        for q in range(nb):
            sel = row[b == q]
            counts[s, q] = sel.size
            sums[s, q] = float(sel.size) if w is None else math.fsum(w[sel].tolist())
    return sums, counts


def check_sums(got, exact, counts, weighted, label=""):
    """raw sums [R, nb] against the exact ones: equal when unweighted, within the sum bound otherwise"""
    assert got.shape == exact.shape and got.dtype == np.float64
    if not weighted:
        assert np.array_equal(got, counts.astype(np.float64)), f"{label}: counts differ"
        return
    err, bound = np.abs(got - exact), sum_bound(counts, exact)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{label}: worst |sum - exact| / bound {worst:.3f}")
    assert np.all(err <= bound)
