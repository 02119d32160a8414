#!/usr/bin/env python
"""Generate tests/golden/analysis.npz by IMPORTING the reference (CPU only, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_analysis_goldens.py

What runs: the UNMODIFIED ``bgflow/distribution/sampling/_mcmc/analysis.py``, loaded by path (it needs numpy alone).  The fixture
holds DATA only; it is written with fixed zip time stamps, so the script regenerates it bit for bit.

Data: D = two Gaussians at 1.0 and 2.0 (sigma 0.15, 40 % each) + 20 % uniform on [0.5, 2.5], W = exp(2 g - max), g standard normal, from
``default_rng(20264)``; stored as float32.  The reference is evaluated on the exact f64 widening of the stored arrays (the same numbers):
np.histogram accumulates weights in the weights' own dtype, so on f32 weights the reference's sums would carry f32 rounding -- 3e-5 in
``Es`` -- and the fixture could not serve an f64 bound.  Per case the script calls
``np.random.seed(k)`` and the reference, re-seeds, repeats the reference's ``np.random.choice(I, size=len(D), replace=True)`` calls to
record every replicate's indices, and asserts that ``Es`` recomputed from the recorded indices equals the reference's output exactly.

  weighted    N 4096, (l, r, n) = (0.5, 2.5, 17), sample 8, weights W.  Asserted: 3 samples outside the range, the smallest count of
              any bin over 256 resamplings is 39, Es finite everywhere
  unweighted  the same D, weights None
  bias        ``weighted`` with bias(x) = 3 (x - 1.5)^2 and temperature 2
  f64         ``weighted``'s arrays widened to f64 and perturbed below f32 resolution (relative 2^-30)
  offgrid     N 2048, (0.3, 2.7, 14) -- edges that are not f32 numbers --, sample 6; the first entries of D replaced by float32(edge) of
              every edge, its f32 neighbours one ulp either side, values outside the range, NaN and +-inf; ``offgrid_n_ignored`` counts the
              entries outside [l, r] or non-finite
  empty       N 1024, one interior bin (8: [1.5, 1.625)) holds 3 samples; the first seed for which at least one replicate leaves that
              bin empty (+inf) and at least one does not
  trajs       8 trajectories of lengths 511, 512, 513, 1, 64, 700, 300, 1095 cut from ``weighted``'s D and W, sample 6, indices [6, 8]
  f32         the first 1024 samples, unweighted, sample 4, the reference run on the stored FLOAT32 array itself, as a user passes it
              (``widened`` false in the case table); asserted equal to the run on the f64 widening: counts are exact in any dtype
  f32w        the same with the float32 weights, the reference on the float32 arrays: np.histogram's f32 weight sums (asserted 1e-8 ..
              1e-3 away from the f64 run).  For the numpy path alone, which makes the same numpy calls; no f64 bound applies to it

``weighted``, ``unweighted``, ``bias`` and ``f64`` share seed and size and therefore indices: stored once (``idx`` in the case table names
the owner).  Small vectors with NaN and infinite entries for ``mean_finite`` / ``std_finite`` / ``bar``; ``meta``: JSON -- parameter names and
defaults of the reference's functions.
"""
import importlib.util
import inspect
import io
import json
import os
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20264
LENGTHS = (511, 512, 513, 1, 64, 700, 300, 1095)


def load_reference():
    path = os.path.join(os.environ["BGFLOW_REFERENCE"], "bgflow", "distribution", "sampling", "_mcmc", "analysis.py")
    spec = importlib.util.spec_from_file_location("reference_analysis", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bias(x):
    return 3.0 * (x - 1.5) ** 2


def data(rng, N):
    k = rng.integers(0, 5, N)
    D = np.where(k < 2, 1.0 + 0.15 * rng.standard_normal(N), np.where(k < 4, 2.0 + 0.15 * rng.standard_normal(N), rng.uniform(0.5, 2.5, N)))
    logw = 2.0 * rng.standard_normal(N)
    W = np.exp(logw - logw.max())
    return D.astype(np.float32), W.astype(np.float32)


def widen(a):
    """the exact f64 widening of stored f32 data (lists: per trajectory)"""
    if a is None:
        return None
    return [v.astype(np.float64) for v in a] if isinstance(a, list) else a.astype(np.float64)


def recompute(D, W, idx, l, r, n, bias=None, temperature=1.0):
    """the reference's arithmetic on recorded indices"""
    bins = np.linspace(l, r, n)
    by_traj = isinstance(D, list)
    Es = []
    for Isel in idx:
        Ds = np.concatenate([D[i] for i in Isel]) if by_traj else D[Isel]
        Ws = None if W is None else (np.concatenate([W[i] for i in Isel]) if by_traj else W[Isel])
        P, _ = np.histogram(Ds, bins=bins, weights=Ws, density=True)
        Es.append(-np.log(P))
    Es = np.vstack(Es)
    Es -= Es.mean(axis=0).min()
    if bias is not None:
        Es -= bias(0.5 * (bins[:-1] + bins[1:])) / temperature
    return Es


def run_case(ref, D, W, l, r, n, sample, seed, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # log(0) of an empty bin
        np.random.seed(seed)
        bm, Es = ref.free_energy_bootstrap(D, l, r, n, sample=sample, weights=W, **kw)
        np.random.seed(seed)
        I = np.arange(len(D))          # noqa: E741
        idx = np.stack([np.random.choice(I, size=len(D), replace=True) for _ in range(sample)])
        again = recompute(D, W, idx, l, r, n, **kw)
    assert Es.shape == (sample, n - 1) and np.array_equal(Es, again, equal_nan=True), "the recorded indices do not reproduce the reference"
    return bm, Es, idx


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (a zip archive of .npy members)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = load_reference()
    rng = np.random.default_rng(SEED)
    D, W = data(rng, 4096)
    l, r, n = 0.5, 2.5, 17
    edges = np.linspace(l, r, n)
    assert int(np.sum((D < l) | (D > r))) == 3
    smallest = min(np.histogram(D[rng.integers(0, 4096, 4096)], bins=edges)[0].min() for _ in range(256))
    assert smallest == 39, smallest

    out, cases = {"seed": np.int64(SEED)}, {}

    def store(name, D_, W_, l_, r_, n_, sample, seed, idx_owner=None, widened=True, **kw):
        bm, Es, idx = run_case(ref, widen(D_) if widened else D_, widen(W_) if widened else W_, l_, r_, n_, sample, seed, **kw)
        if not isinstance(D_, list):
            out[f"{name}_D"] = D_
            if W_ is not None:
                out[f"{name}_W"] = W_
        if idx_owner is None:
            assert idx.max() < 2 ** 15
            out[f"{name}_idx"] = idx.astype(np.int16)
        else:
            assert np.array_equal(idx, out[f"{idx_owner}_idx"])
        out[f"{name}_bin_means"], out[f"{name}_Es"] = bm, Es
        cases[name] = {"l": l_, "r": r_, "n": n_, "sample": sample, "seed": seed, "weights": W_ is not None, "idx": idx_owner or name, "widened": widened,
                       "bias": "bias" in kw, "temperature": kw.get("temperature", 1.0)}
        return Es

    Es = store("weighted", D, W, l, r, n, 8, 1)
    assert np.isfinite(Es).all()
    store("unweighted", D, None, l, r, n, 8, 1, idx_owner="weighted")
    store("bias", D, W, l, r, n, 8, 1, idx_owner="weighted", bias=bias, temperature=2.0)
    prng = np.random.default_rng(SEED + 1)
    D64 = D.astype(np.float64) * (1.0 + 2.0 ** -30 * prng.uniform(-1, 1, D.size))
    W64 = W.astype(np.float64) * (1.0 + 2.0 ** -30 * prng.uniform(-1, 1, W.size))
    assert np.array_equal(D64.astype(np.float32), D) and not np.array_equal(D64, D.astype(np.float64))
    store("f64", D64, W64, l, r, n, 8, 1, idx_owner="weighted")

    # offgrid: edges that are not f32 numbers, samples on and next to them
    lo, ro, no = 0.3, 2.7, 14
    eo = np.linspace(lo, ro, no)
    e32 = eo.astype(np.float32)
    special = np.concatenate([e32, np.nextafter(e32, np.float32(-np.inf)), np.nextafter(e32, np.float32(np.inf)),
                              np.array([lo, ro, 0.29, 2.71, -1.0, 5.0, np.nan, np.inf, -np.inf], np.float32)])
    assert special.size <= 64 and special.dtype == np.float32 and not all(float(np.float32(e)) == e for e in eo[1:-1])
    Do, Wo = D[:2048].copy(), W[:2048].copy()
    Do[:special.size] = special
    store("offgrid", Do, Wo, lo, ro, no, 6, 2)
    with np.errstate(invalid="ignore"):
        out["offgrid_n_ignored"] = np.int64(np.sum(~((Do.astype(np.float64) >= eo[0]) & (Do.astype(np.float64) <= eo[-1]))))
    assert out["offgrid_n_ignored"] >= 9

    # empty: bin 8 keeps 3 samples
    b = 8
    inside = (D >= edges[b]) & (D < edges[b + 1])
    De = np.concatenate([D[~inside][:1021], D[inside][:3]])
    We = np.concatenate([W[~inside][:1021], W[inside][:3]])
    assert np.histogram(De, bins=edges)[0][b] == 3
    for seed in range(3, 200):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            np.random.seed(seed)
            _, Ee = ref.free_energy_bootstrap(widen(De), l, r, n, sample=8, weights=widen(We))
        if np.isposinf(Ee[:, b]).any() and np.isfinite(Ee[:, b]).any():
            break
    else:
        raise AssertionError("no seed leaves the bin empty in some replicates only")
    Ee = store("empty", De, We, l, r, n, 8, seed)
    assert np.isposinf(Ee[:, b]).any() and np.isfinite(Ee[:, b]).any() and not np.isnan(Ee).any()

    # trajs: bootstrap by trajectory
    assert sum(LENGTHS) <= D.size
    cuts = np.concatenate([[0], np.cumsum(LENGTHS)])
    Dt = [D[a:z] for a, z in zip(cuts[:-1], cuts[1:])]
    Wt = [W[a:z] for a, z in zip(cuts[:-1], cuts[1:])]
    store("trajs", Dt, Wt, l, r, n, 6, 4)
    out["trajs_lengths"] = np.array(LENGTHS, np.int64)
    assert out["trajs_idx"].shape == (6, 8)

    # the reference on f32 arrays as a user passes them: unweighted counts are exact in any dtype; weighted, np.histogram's f32 sums
    E32 = store("f32", D[:1024], None, l, r, n, 4, 5, widened=False)
    E32w = store("f32w", D[:1024], W[:1024], l, r, n, 4, 5, idx_owner="f32", widened=False)
    assert out["f32_D"].dtype == np.float32 and E32.dtype == np.float64 and np.isfinite(E32).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        in_f64 = recompute(widen(D[:1024]), widen(W[:1024]), out["f32_idx"], l, r, n)
    assert np.array_equal(recompute(widen(D[:1024]), None, out["f32_idx"], l, r, n), E32) and 1e-8 < np.abs(in_f64 - E32w).max() < 1e-3

    # small vectors
    x = np.array([0.5, np.nan, 1.5, np.inf, -2.0, 3.25, -np.inf, 0.125], np.float64)
    x2 = np.array([[1.0, np.nan, 3.0, 4.0], [np.inf, 2.0, -1.0, 0.5], [0.25, 8.0, np.nan, -3.0], [2.0, 1.0, 7.0, np.nan], [5.0, -np.inf, 2.5, 1.5]])
    few = np.array([1.0, np.nan, 2.0, np.inf])
    ua = np.array([0.3, -0.2, 1.5, 2.5, -1.0, 0.0, 4.0])
    ub = np.array([-0.1, 0.7, -2.0, 1.0, 0.2])
    out.update(vec_x=x, vec_x2=x2, vec_few=few, vec_ua=ua, vec_ub=ub,
               vec_mean_=np.float64(ref.mean_finite_(x)), vec_std_=np.float64(ref.std_finite_(x)),
               vec_few_mean_=np.float64(ref.mean_finite_(few)), vec_few_std_=np.float64(ref.std_finite_(few)),
               vec_mean=np.float64(ref.mean_finite(x)), vec_std_axis_none=np.float64(ref.std_finite(x)),
               vec_mean_axis0=ref.mean_finite(x2, axis=0), vec_mean_axis1=ref.mean_finite(x2, axis=1),
               vec_std_axis0=ref.std_finite(x2, axis=0), vec_std_axis1=ref.std_finite(x2, axis=1),
               vec_metropolis=ref.metropolis_function(ua), vec_bar=np.float64(ref.bar(ua, ub)))
    assert np.isnan(out["vec_few_std_"]) and out["vec_std_axis_none"] == out["vec_mean"]        # the reference's std_finite(axis=None)

    names = ("mean_finite_", "std_finite_", "mean_finite", "std_finite", "metropolis_function", "bar", "free_energy_bootstrap")
    out["meta"] = np.array(json.dumps({f: [[p.name, "<required>" if p.default is p.empty else p.default]
                                           for p in inspect.signature(getattr(ref, f)).parameters.values()] for f in names}))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "analysis.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size < 300 * 1024, size
    print(path, size, "bytes;", ", ".join(f"{k} {out[k + '_Es'].shape}" for k in cases))


if __name__ == "__main__":
    main()
