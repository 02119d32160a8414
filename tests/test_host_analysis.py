"""On the CPU: bgflow_amd.analysis against tests/golden/analysis.npz -- the numpy path (the reference's method, bit for bit under
np.random.seed), the torch path with the recorded indices, the raw histograms, the statistics helpers, signatures and import paths, the
entry's prototype and argument checks, and the index stream the GPU tests compare the kernel with.  Bounds: analysis_common.py."""
import ctypes
import inspect
import json
import math
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib, analysis
from bgflow_amd._abi import HEADER, abi_signatures
from bgflow_amd.build import abi_symbols

from analysis_common import CASE_NAMES, NUMPY_CASE_NAMES, case, case_kwargs, cases, check_profile, max_draws, np_bins, philox_indices, widen

p, i32, i64, u32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
WANT = [p, p, i64, i32, p, i32, i64, i64, p, p, u64, u32, i32, p, p, p, p, p]


def tensors(D, W, dtype, device="cpu"):
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)      # noqa: E731
    if isinstance(D, list):
        return [conv(d) for d in D], [conv(w) for w in W]
    return conv(D), None if W is None else conv(W)


def test_fixture_holds_the_cases(golden):
    G = golden("analysis")
    assert list(cases(G)) == NUMPY_CASE_NAMES
    assert G["weighted_D"].dtype == np.float32 and G["f64_D"].dtype == np.float64 and G["offgrid_D"].size == 2048


@pytest.mark.parametrize("name", NUMPY_CASE_NAMES)
def test_numpy_path_is_the_reference_under_its_seed(golden, name):
    G = golden("analysis")
    D, W, idx, spec = case(G, name)
    if spec["widened"]:                                              # the reference ran on the f64 widening of the stored data,
        D, W = widen(D), widen(W)                                    # except for f32 / f32w: on the stored f32 arrays themselves
    else:
        assert D.dtype == np.float32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        np.random.seed(spec["seed"])
        bm, Es = bg.free_energy_bootstrap(D, spec["l"], spec["r"], spec["n"], weights=W, **case_kwargs(spec))
        _, again = bg.free_energy_bootstrap(D, spec["l"], spec["r"], spec["n"], weights=W, indices=idx, **case_kwargs(spec))
    assert isinstance(Es, np.ndarray) and isinstance(bm, np.ndarray)
    assert np.array_equal(bm, G[f"{name}_bin_means"]) and np.array_equal(Es, G[f"{name}_Es"], equal_nan=True)
    assert np.array_equal(again, Es, equal_nan=True)


# (the f64 case rounds to `weighted` in f32: f64 only)
@pytest.mark.parametrize("name,dtype", [(c, t) for c in CASE_NAMES for t in (torch.float32, torch.float64) if (c, t) != ("f64", torch.float32)])
def test_torch_path_with_the_recorded_indices(golden, name, dtype):
    G = golden("analysis")
    D, W, idx, spec = case(G, name)
    Dt, Wt = tensors(D, W, dtype)
    bm, Es = bg.free_energy_bootstrap(Dt, spec["l"], spec["r"], spec["n"], weights=Wt, indices=idx, **case_kwargs(spec))
    assert bm.dtype == torch.float64 and Es.dtype == torch.float64 and Es.device.type == "cpu"
    check_profile(G, name, bm.numpy(), Es.numpy(), max_draws(D), label=f"torch {dtype} ")


def test_raw_histograms_on_offgrid(golden):
    G = golden("analysis")
    D, W, idx, spec = case(G, "offgrid")
    edges = np.linspace(spec["l"], spec["r"], spec["n"])
    sums, ignored = bg.bootstrap_histogram(torch.from_numpy(D), edges, spec["sample"], indices=idx, return_ignored=True)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (spec["sample"], spec["n"] - 1)
    with np.errstate(invalid="ignore"):
        want = np.stack([np.histogram(D[row], bins=edges)[0] for row in idx])
    assert np.array_equal(sums.numpy(), want.astype(np.float64))
    assert ignored.tolist() == [int(G["offgrid_n_ignored"]), 0]
    # the test's own bin rule is np.histogram's too
    bins = np_bins(D, edges)
    assert np.array_equal(np.bincount(bins[bins >= 0], minlength=spec["n"] - 1), np.histogram(D, bins=edges)[0])
    assert int((bins < 0).sum()) == int(G["offgrid_n_ignored"])
    with pytest.raises(TypeError):
        bg.bootstrap_histogram(D, edges, spec["sample"], indices=idx)           # tensors only


def test_bad_weights_drop_their_sample_with_one_warning(golden):
    G = golden("analysis")
    D, W, idx, spec = case(G, "weighted")
    edges = np.linspace(spec["l"], spec["r"], spec["n"])
    Dt, Wt = tensors(D, W, torch.float64)
    planted = Wt.clone()
    inside = np.flatnonzero(np_bins(D, edges) >= 0)[:4]
    planted[inside[0]], planted[inside[1]], planted[inside[2]], planted[inside[3]] = float("nan"), float("inf"), -1.0, float("-inf")
    with pytest.warns(UserWarning, match="4 samples") as rec:
        sums, ignored = bg.bootstrap_histogram(Dt, edges, 3, weights=planted, indices=idx[:3], return_ignored=True)
    assert len(rec) == 1 and ignored.tolist() == [3, 4]
    zeroed = Wt.clone()
    zeroed[torch.from_numpy(inside)] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clean = bg.bootstrap_histogram(Dt, edges, 3, weights=zeroed, indices=idx[:3])
    assert torch.equal(sums, clean) and bool(torch.isfinite(sums).all())


def test_statistics_helpers(golden):
    G = golden("analysis")
    x, x2, few = G["vec_x"], G["vec_x2"], G["vec_few"]
    assert analysis.mean_finite_(x) == G["vec_mean_"] and analysis.std_finite_(x) == G["vec_std_"]
    assert analysis.mean_finite_(few) == G["vec_few_mean_"] and math.isnan(analysis.std_finite_(few)) and math.isnan(G["vec_few_std_"])
    assert analysis.mean_finite(x) == G["vec_mean"]
    for axis in (0, 1):
        assert np.array_equal(analysis.mean_finite(x2, axis=axis), G[f"vec_mean_axis{axis}"], equal_nan=True)
        assert np.array_equal(analysis.std_finite(x2, axis=axis), G[f"vec_std_axis{axis}"], equal_nan=True)
    with pytest.raises(NotImplementedError):
        analysis.mean_finite(x2, axis=2)
    assert np.array_equal(analysis.metropolis_function(G["vec_ua"]), G["vec_metropolis"])
    assert analysis.bar(G["vec_ua"], G["vec_ub"]) == G["vec_bar"]
    # the two documented deviations: std_finite(axis=None) is the standard deviation (the reference returns the mean) ...
    assert G["vec_std_axis_none"] == G["vec_mean"] and analysis.std_finite(x) == G["vec_std_"] != G["vec_mean"]
    # ... and the axis variants pass min_finite on
    assert np.isnan(analysis.mean_finite(x2, axis=0, min_finite=4)).all() and not np.isnan(analysis.mean_finite(x2, axis=0)).any()
    # tensors
    xt = torch.from_numpy(x)
    assert abs(float(analysis.mean_finite_(xt)) - G["vec_mean_"]) <= 1e-15 and abs(float(analysis.std_finite(xt)) - G["vec_std_"]) <= 1e-15
    assert np.allclose(analysis.mean_finite(torch.from_numpy(x2), axis=1).numpy(), G["vec_mean_axis1"], rtol=1e-15, atol=0, equal_nan=True)
    assert abs(float(analysis.bar(torch.from_numpy(G["vec_ua"]), torch.from_numpy(G["vec_ub"]))) - G["vec_bar"]) <= 1e-15


def test_signatures_are_the_references(golden):
    meta = json.loads(str(golden("analysis")["meta"]))
    extra = {"free_energy_bootstrap": ["seed", "indices"]}
    for name, want in meta.items():
        params = list(inspect.signature(getattr(analysis, name)).parameters.values())
        positional = [q for q in params if q.kind is not q.KEYWORD_ONLY]
        assert [[q.name, "<required>" if q.default is q.empty else q.default] for q in positional] == want, name
        assert [q.name for q in params if q.kind is q.KEYWORD_ONLY] == extra.get(name, []), name
    sig = inspect.signature(analysis.bootstrap_histogram)
    assert list(sig.parameters)[:4] == ["D", "edges", "sample", "weights"]
    assert [q.name for q in sig.parameters.values() if q.kind is q.KEYWORD_ONLY] == ["seed", "indices", "return_ignored"]


def test_import_paths():
    import sys

    import bgflow_amd.distribution.sampling._mcmc as package
    import bgflow_amd.distribution.sampling._mcmc.analysis as module
    from bgflow_amd.distribution.sampling._mcmc.analysis import free_energy_bootstrap
    assert free_energy_bootstrap is analysis.free_energy_bootstrap is bg.free_energy_bootstrap is package.free_energy_bootstrap
    assert module.bootstrap_histogram is analysis.bootstrap_histogram is bg.bootstrap_histogram
    assert sys.modules["bgflow_amd.distribution.sampling._mcmc.analysis"] is module and package.analysis is module
    assert package.HungarianMapper is bg.HungarianMapper and module.mean_finite is analysis.mean_finite and bg.analysis is analysis


def test_manual_seed_repeats_a_run(golden):
    G = golden("analysis")
    D, W, _, spec = case(G, "weighted")
    Dt, Wt = tensors(D, W, torch.float32)
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        runs.append(bg.free_energy_bootstrap(Dt, spec["l"], spec["r"], spec["n"], sample=3, weights=Wt)[1])
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    a = bg.free_energy_bootstrap(Dt, spec["l"], spec["r"], spec["n"], sample=3, weights=Wt, seed=11)[1]
    b = bg.free_energy_bootstrap(Dt, spec["l"], spec["r"], spec["n"], sample=3, weights=Wt, seed=11)[1]
    assert torch.equal(a, b)
    # by trajectory
    Dl, Wl = tensors(*case(G, "trajs")[:2], torch.float32)
    torch.manual_seed(5)
    t1 = bg.free_energy_bootstrap(Dl, 0.5, 2.5, 17, sample=4, weights=Wl)[1]
    torch.manual_seed(5)
    assert torch.equal(t1, bg.free_energy_bootstrap(Dl, 0.5, 2.5, 17, sample=4, weights=Wl)[1])


def test_the_prototype_is_declared_parsed_and_exported(hip_lib):
    sigs = abi_signatures()
    assert sigs["bgk_bootstrap_histogram"] == (ctypes.c_int, WANT)
    assert "bgk_bootstrap_histogram" in abi_symbols()
    assert list(hip_lib.bgk_bootstrap_histogram.argtypes) == WANT
    assert ctypes.cast(ctypes.CDLL(_lib.LIB_PATH).bgk_bootstrap_histogram, ctypes.c_void_p).value, "bgk_bootstrap_histogram is not exported"
    with open(HEADER) as f:
        header = f.read()
    assert "#define BGK_HIST_F32 0\n" in header and "#define BGK_HIST_F64 1\n" in header
    assert analysis._DTYPE_CODES == {torch.float32: 0, torch.float64: 1} and analysis.MAX_BINS == 4096 and analysis.MAX_CHUNKS == 512


def test_argument_checks_of_the_entry(hip_lib):
    fake = ctypes.c_void_p(64)              # never dereferenced: every check comes before the first launch

    def call(d=fake, w=None, n=8, dtype=0, edges=fake, nb=4, reps=0, r0=0, indices=None, segments=None, seed=1, offset=0, n_chunks=1,
             records=fake, partial=fake, out=fake, n_ignored=fake):
        return hip_lib.bgk_bootstrap_histogram(d, w, n, dtype, edges, nb, reps, r0, indices, segments, seed, offset, n_chunks, records,
                                               partial, out, n_ignored, None)

    err = hip_lib.bgk_last_error
    assert call() == 0 and call(w=fake, indices=fake) == 0 and call(segments=fake, n_ignored=None) == 0      # no replicates: no launch
    for bad in (dict(d=None), dict(edges=None), dict(records=None), dict(partial=None), dict(out=None)):
        assert call(**bad) == -1 and b"null pointer" in err()
    assert call(n=0) == -1 and b"bad size" in err() and call(n=-5) == -1
    assert call(dtype=2) == -1 and b"dtype" in err() and call(dtype=-1) == -1 and call(dtype=1) == 0
    assert call(nb=0) == -1 and b"bins" in err() and call(nb=-1) == -1 and call(nb=4096) == 0
    assert call(nb=4097) == -2 and b"envelope" in err()
    assert call(n_chunks=0) == -1 and b"n_chunks" in err() and call(n_chunks=513) == -1 and call(n_chunks=512) == 0
    assert call(r0=-1) == -1 and b"replicates" in err() and call(reps=-1) == -1
    assert call(r0=2 ** 32) == 0 and call(r0=2 ** 32 + 1) == -1 and call(r0=2 ** 32 - 3, reps=4) == -1 and b"2^32" in err()
    assert call(indices=fake, segments=fake) == -1 and b"both indices and segments" in err()
    assert call(d=ctypes.c_void_p(68)) == 0 and call(d=ctypes.c_void_p(68), dtype=1) == -1 and b"aligned" in err()
    for name in ("w", "edges", "partial", "out", "indices", "segments", "n_ignored"):
        assert call(**{name: ctypes.c_void_p(66)}) == -1 and b"aligned" in err(), name
    assert call(records=ctypes.c_void_p(68)) == -1 and call(records=ctypes.c_void_p(72)) == 0 and call(records=ctypes.c_void_p(72), dtype=1) == -1


def test_index_stream():
    for n in (1, 2, 3, 4096):
        idx = philox_indices(77, n, 3)
        assert idx.shape == (3, n) and idx.min() >= 0 and idx.max() < n
    assert philox_indices(77, 1, 2).tolist() == [[0], [0]]
    odd = philox_indices(77, 3, 40)                                  # an odd number of draws: the last call serves one draw
    assert odd.min() == 0 and odd.max() == 2
    long, short = philox_indices(9, 4096, 1), philox_indices(9, 4095, 1)
    assert long.shape == (1, 4096) and len(np.unique(long)) > 2400   # 4096 draws from 4096: about 63 % distinct
    assert not np.array_equal(long[0, :4095], short[0])              # n is part of the map, not only of the count
    # the draws depend on the absolute replicate number alone
    whole = philox_indices(123456789012345678, 65, 7)
    assert np.array_equal(philox_indices(123456789012345678, 65, 4, replicate0=3), whole[3:])
    assert not np.array_equal(whole[0], whole[1]) and not np.array_equal(whole, philox_indices(123456789012345679, 65, 7))
    assert not np.array_equal(whole, philox_indices(123456789012345678, 65, 7, offset=1))
    # uniform: 3 values over 120 draws, none rarer than 20
    assert np.bincount(odd.reshape(-1), minlength=3).min() >= 20
