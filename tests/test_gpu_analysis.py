"""On the GPU: the kernel path of bgflow_amd.analysis (csrc/bgk_hist.hip) against tests/golden/analysis.npz, against the index stream
restated on the host (analysis_common.philox_indices) and against exact sums -- explicit indices, the Philox draws at sizes around the
wave and the chunking, the split of replicates over calls, segments, bin counts at the envelope's ends, the dispatch between the kernel
and the torch ops.  Bounds: analysis_common.py."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib, analysis

from analysis_common import (CASE_NAMES, case, case_kwargs, check_profile, check_sums, es_atol, exact_histogram, max_draws, np_bins,
                             philox_indices)
from test_host_analysis import tensors

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15


def edges_of(spec):
    return np.linspace(spec["l"], spec["r"], spec["n"])


def launch(d, w, edges, reps, seed=SEED, replicate0=0, n_chunks=1, indices=None, segments=None):
    """one call of the entry on device tensors: (out [reps, nb], n_ignored [2])"""
    dev, n, nb = d.device, d.numel(), len(edges) - 1
    e = torch.from_numpy(edges).to(dev)
    records = torch.empty(2 * n, dtype=d.dtype, device=dev)
    partial = torch.empty(max(reps, 1) * n_chunks * nb, dtype=torch.float64, device=dev)
    out = torch.full((reps, nb), -1.0, dtype=torch.float64, device=dev)
    ignored = torch.full((2,), -1, dtype=torch.int64, device=dev)
    st = _lib.lib().bgk_bootstrap_histogram(_lib.ptr(d), _lib.ptr(w), n, analysis._DTYPE_CODES[d.dtype], _lib.ptr(e), nb, reps, replicate0,
                                            _lib.ptr(indices), _lib.ptr(segments), seed, 0, n_chunks, _lib.ptr(records), _lib.ptr(partial),
                                            _lib.ptr(out), _lib.ptr(ignored), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_bootstrap_histogram")
    torch.cuda.synchronize()
    return out, ignored


@pytest.mark.parametrize("name", CASE_NAMES)
def test_explicit_indices_meet_the_fixture(golden, dev, name):
    G = golden("analysis")
    D, W, idx, spec = case(G, name)
    dtype = torch.float64 if name == "f64" else torch.float32
    Dt, Wt = tensors(D, W, dtype, dev)
    assert analysis._kernel_eligible(Dt if isinstance(Dt, list) else [Dt], None if Wt is None else (Wt if isinstance(Wt, list) else [Wt]))
    bm, Es = bg.free_energy_bootstrap(Dt, spec["l"], spec["r"], spec["n"], weights=Wt, indices=idx, **case_kwargs(spec))
    assert bm.device == dev and Es.device == dev and Es.dtype == torch.float64
    check_profile(G, name, bm.cpu().numpy(), Es.cpu().numpy(), max_draws(D), label=f"kernel {dtype} ")


@pytest.mark.parametrize("name", ["weighted", "unweighted", "f64", "offgrid", "empty"])
def test_raw_sums_with_explicit_indices(golden, dev, name):
    G = golden("analysis")
    D, W, idx, spec = case(G, name)
    edges = edges_of(spec)
    Dt, Wt = tensors(D, W, torch.float64 if name == "f64" else torch.float32, dev)
    bins = np_bins(D, edges)
    for weights, wt in ((None, None), (W, Wt)) if W is not None else ((None, None),):
        sums, ignored = bg.bootstrap_histogram(Dt, edges, spec["sample"], weights=wt, indices=idx, return_ignored=True)
        exact, counts = exact_histogram(bins, weights, idx, len(edges) - 1)
        check_sums(sums.cpu().numpy(), exact, counts, weights is not None, label=f"{name} indices")
        assert ignored.tolist() == [int((bins < 0).sum()), 0]
    if name == "offgrid":
        assert ignored.tolist()[0] == int(G["offgrid_n_ignored"])
        with np.errstate(invalid="ignore"):
            want = np.stack([np.histogram(D[row], bins=edges)[0] for row in idx])
        unweighted = bg.bootstrap_histogram(Dt, edges, spec["sample"], indices=idx)
        assert np.array_equal(unweighted.cpu().numpy(), want.astype(np.float64))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4099])
def test_philox_draws_equal_the_restated_stream(golden, dev, monkeypatch, n):
    G = golden("analysis")
    D, W, _, spec = case(G, "weighted")
    D, W = np.concatenate([D, D[:3]])[:n], np.concatenate([W, W[:3]])[:n]
    edges = edges_of(spec)
    Dt, Wt = tensors(D, W, torch.float32, dev)
    idx = philox_indices(SEED, n, 5)
    bins = np_bins(D, edges)
    exact_u, counts = exact_histogram(bins, None, idx, len(edges) - 1)
    exact_w, _ = exact_histogram(bins, W, idx, len(edges) - 1)
    first = None
    for n_chunks in (1, 3, 7):
        monkeypatch.setattr(analysis, "N_CHUNKS", n_chunks)
        u = bg.bootstrap_histogram(Dt, edges, 5, seed=SEED).cpu().numpy()
        w = bg.bootstrap_histogram(Dt, edges, 5, weights=Wt, seed=SEED).cpu().numpy()
        check_sums(u, exact_u, counts, False, label=f"n {n} chunks {n_chunks}")
        check_sums(w, exact_w, counts, True, label=f"n {n} chunks {n_chunks} weighted")
        first = u if first is None else first
        assert np.array_equal(u, first)
    assert counts.sum() == 5 * n - int((bins[idx] < 0).sum())


def test_replicates_split_over_calls(golden, dev, monkeypatch):
    G = golden("analysis")
    D, W, _, spec = case(G, "weighted")
    edges = edges_of(spec)
    nb = len(edges) - 1
    Dt, Wt = tensors(D, W, torch.float32, dev)
    bins = np_bins(D, edges)
    idx = philox_indices(SEED, D.size, 7)
    exact_w, counts = exact_histogram(bins, W, idx, nb)
    for wt in (None, Wt):
        whole, _ = launch(Dt, wt, edges, 7, n_chunks=3)
        a, _ = launch(Dt, wt, edges, 3, replicate0=0, n_chunks=2)
        b, _ = launch(Dt, wt, edges, 4, replicate0=3, n_chunks=5)
        parts = torch.cat([a, b])
        if wt is None:
            assert torch.equal(whole, parts) and np.array_equal(whole.cpu().numpy(), counts.astype(np.float64))
        else:
            check_sums(whole.cpu().numpy(), exact_w, counts, True, label="7 in one call")
            check_sums(parts.cpu().numpy(), exact_w, counts, True, label="3 + 4")
    # the Python batching: a byte budget of one replicate's partials per call
    one = bg.bootstrap_histogram(Dt, edges, 7, seed=SEED)
    monkeypatch.setattr(analysis, "PARTIAL_BYTES", analysis._n_chunks(D.size, 7) * nb * 8)
    batched = bg.bootstrap_histogram(Dt, edges, 7, seed=SEED)
    assert torch.equal(one, batched) and np.array_equal(one.cpu().numpy(), counts.astype(np.float64))
    check_sums(bg.bootstrap_histogram(Dt, edges, 7, weights=Wt, seed=SEED).cpu().numpy(), exact_w, counts, True, label="batched by 1")
    # the highest replicate number the counter word holds
    top, _ = launch(Dt, None, edges, 2, replicate0=2 ** 32 - 2)
    want = exact_histogram(bins, None, philox_indices(SEED, D.size, 2, replicate0=2 ** 32 - 2), nb)[1]
    assert np.array_equal(top.cpu().numpy(), want.astype(np.float64))


def test_segments_are_plain_histograms(golden, dev):
    G = golden("analysis")
    D, W, idx, spec = case(G, "trajs")
    edges = edges_of(spec)
    Dt, Wt = tensors(D, W, torch.float32, dev)
    lengths = [len(d) for d in D]
    seg = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    with np.errstate(invalid="ignore"):
        rows = np.stack([np.histogram(d, bins=edges)[0] for d in D])
    for n_chunks in (1, 4):
        H, ignored = launch(torch.cat(Dt), None, edges, len(D), n_chunks=n_chunks, segments=seg)
        assert np.array_equal(H.cpu().numpy(), rows.astype(np.float64))
    flat_bins = np_bins(np.concatenate(D), edges)
    assert ignored.tolist() == [int((flat_bins < 0).sum()), 0]
    Hw, _ = launch(torch.cat(Dt), torch.cat(Wt), edges, len(D), n_chunks=2, segments=seg)
    cuts = np.concatenate([[0], np.cumsum(lengths)])
    own = [np.arange(a, z) for a, z in zip(cuts[:-1], cuts[1:])]       # every trajectory's own samples
    exact, counts = exact_histogram(flat_bins, np.concatenate(W), own, len(edges) - 1)
    check_sums(Hw.cpu().numpy(), exact, counts, True, label="segments weighted")
    # the public function by trajectory, unweighted, against sums of the resampled rows
    sums = bg.bootstrap_histogram(Dt, edges, spec["sample"], indices=idx)
    assert np.array_equal(sums.cpu().numpy(), rows[idx].sum(1).astype(np.float64))


@pytest.mark.parametrize("nb", [1, 13, 4096])
def test_bin_counts(golden, dev, nb):
    G = golden("analysis")
    D, W, idx, spec = case(G, "offgrid")
    edges = np.linspace(spec["l"], spec["r"], nb + 1)
    Dt, Wt = tensors(D, W, torch.float32, dev)
    bins = np_bins(D, edges)
    idx = idx[:2]
    exact, counts = exact_histogram(bins, W, idx, nb)
    sums, ignored = bg.bootstrap_histogram(Dt, edges, 2, indices=idx, return_ignored=True)
    with np.errstate(invalid="ignore"):
        want = np.stack([np.histogram(D[row], bins=edges)[0] for row in idx])
    assert np.array_equal(sums.cpu().numpy(), want.astype(np.float64))
    assert ignored.tolist() == [int((bins < 0).sum()), 0]
    weighted = bg.bootstrap_histogram(Dt, edges, 2, weights=Wt, indices=idx).cpu().numpy()
    check_sums(weighted, exact, counts, True, label=f"nb {nb}")
    philox = bg.bootstrap_histogram(Dt, edges, 2, seed=SEED).cpu().numpy()
    assert np.array_equal(philox.sum(1), (bins[philox_indices(SEED, D.size, 2)] >= 0).sum(1).astype(np.float64))
    # one bin more than the envelope: the torch ops
    if nb == 4096:
        wide = np.linspace(spec["l"], spec["r"], nb + 2)
        assert bg.bootstrap_histogram(Dt, wide, 1, indices=idx[:1]).shape == (1, nb + 1)


def test_dispatch(golden, dev):
    G = golden("analysis")
    D, W, idx, spec = case(G, "weighted")
    Dt, Wt = tensors(D, W, torch.float32, dev)
    args = (spec["l"], spec["r"], spec["n"])
    _, kernel = bg.free_energy_bootstrap(Dt, *args, sample=8, weights=Wt, indices=idx)
    strided = torch.stack([Dt, Dt], dim=1)[:, 0]
    grad = Dt.clone().requires_grad_(True)
    others = {"non-contiguous": (strided, Wt), "grad": (grad, Wt), "cpu": (Dt.cpu(), Wt.cpu()), "f64 weights of f32 samples": (Dt, Wt.double())}
    for label, (d, w) in others.items():
        assert not analysis._kernel_eligible([d], [w]), label
        bm, Es = bg.free_energy_bootstrap(d, *args, sample=8, weights=w, indices=idx)
        assert Es.device == d.device
        check_profile(G, "weighted", bm.cpu().numpy(), Es.detach().cpu().numpy(), D.size, label=f"{label} ")
        assert float((Es.detach().cpu() - kernel.cpu()).abs().max()) <= 2 * es_atol(D.size, G["weighted_Es"])
    # integer samples: the torch path
    ints = torch.arange(0, 40, device=dev) % 4
    assert not analysis._kernel_eligible([ints], None)
    counts = bg.bootstrap_histogram(ints, np.array([0.0, 1.0, 2.0, 3.0]), 1, indices=torch.arange(40)[None])
    assert counts.tolist() == [[10.0, 10.0, 20.0]]
    # repeated kernel calls with one seed: bitwise equal
    a = bg.bootstrap_histogram(Dt, np.linspace(*args), 6, seed=5)
    b = bg.bootstrap_histogram(Dt, np.linspace(*args), 6, seed=5)
    assert torch.equal(a, b) and not torch.equal(a, bg.bootstrap_histogram(Dt, np.linspace(*args), 6, seed=6))
    with pytest.raises(ValueError):
        bg.bootstrap_histogram(Dt, np.linspace(*args), 2, indices=np.full((2, D.size), D.size))


def test_kernel_path_launches_only_its_own_kernels(golden, dev):
    from test_gpu_round6 import _device_kernel_names
    G = golden("analysis")
    D, W, _, spec = case(G, "weighted")
    Dt, Wt = tensors(D, W, torch.float32, dev)
    edges = edges_of(spec)
    names = _device_kernel_names(lambda: bg.bootstrap_histogram(Dt, edges, 8, weights=Wt, seed=3))
    kernels = [k for k in names if not k.lower().startswith(("memcpy", "memset"))]
    print(names)
    assert kernels and all("hist_" in k for k in kernels), names
    assert [sum(stage in k for k in kernels) for stage in ("hist_digitize_kernel", "hist_resample_kernel", "hist_merge_kernel")] == [1, 1, 1]


def test_stream(golden, dev):
    G = golden("analysis")
    D, W, _, spec = case(G, "weighted")
    Dt, Wt = tensors(D, W, torch.float32, dev)
    edges = edges_of(spec)
    main = bg.bootstrap_histogram(Dt, edges, 4, seed=9)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = bg.bootstrap_histogram(Dt, edges, 4, seed=9)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(r, main)


def test_profile_of_a_dimer_distance(golden, dev):
    """end to end, no fixture comparison: 4096 dimer distances, 16 bins; the profile is finite wherever every replicate's bin is occupied.
    The rows are a SUBSTITUTE for chain output, not a physical ensemble: box.npz holds 150 configurations (36 solvent particles), which
    are tiled 28 times with the dimer's second particle moved by seeded noise.  The test checks the plumbing from ``dimer_distance`` to
    the profile (shapes, counts, where inf may stand); the numbers of the profile mean nothing."""
    G = golden("box")
    x = torch.tensor(G["x_36"], device=dev).repeat(28, 1)[:4096].contiguous()
    g = torch.Generator().manual_seed(4)
    x[:, 2:4] += 0.2 * torch.randn(4096, 2, generator=g).to(dev)
    energy = bg.RepulsiveParticles()
    d = energy.dimer_distance(x).contiguous()
    assert d.shape == (4096,) and d.dtype == torch.float32
    lo, hi = float(d.min()), float(d.max())
    edges = np.linspace(lo, hi, 17)
    sums = bg.bootstrap_histogram(d, edges, 20, seed=12)
    bm, Es = bg.free_energy_bootstrap(d, lo, hi, 17, sample=20, seed=12)
    assert bm.shape == (16,) and Es.shape == (20, 16) and sums.sum(1).tolist() == [4096.0] * 20
    occupied = (sums > 0).all(0)
    assert bool(occupied.any()) and bool(torch.isfinite(Es[:, occupied]).all()) and bool(torch.isposinf(Es[sums == 0]).all())
    assert abs(float(Es.mean(0).min())) <= 1e-12
