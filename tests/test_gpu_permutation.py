"""GPU (-m gpu): ``HungarianMapper`` on bgk_assign_particles (csrc/bgk_assign.hip) against tests/golden/permutation.npz -- scipy's
solution of the f64 problem on the same f32 inputs -- under the stable-row rule of permutation_common.py: the exact permutation on rows
whose solution does not change with the f32 rounding of the costs, a valid permutation and status 0 on the others.

cost: against the f64 cost of the kernel's own permutation on the f32 inputs, within the rounding of an f32 sum of m d squared
differences, (m d + 2) 2^-24 cost.  Everything else is bitwise: y against the gather of X by perm, runs against each other, the kernel
path's ``map`` against the general path's on stable rows.  The integration check bounds the energy change under relabelling by the box
kernel's own bound against its f64 formulas (test_gpu_box.py): err_u <= 4 err(reference f32) + 1e-6."""
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg

from box_common import err_u, make
from mcmc_common import N_FRAMES
from permutation_common import case, case_list, check_perm, cost64, gathered, solve_rows
from test_gpu_mcmc import fused_sampler

pytestmark = pytest.mark.gpu


def launch_all(mapper, x):
    """every output of one launch, as numpy: y, perm (int64), cost, status, permuted"""
    y, perm, cost, status, permuted = mapper._launch(x, y=True, perm=True, cost=True, status=True, permuted=True)
    return y.cpu().numpy(), perm.cpu().numpy().astype(np.int64), cost.cpu().numpy(), status.cpu().numpy(), permuted.cpu().numpy()


def check_outputs(mapper, X, out, label):
    """perm, cost, permuted and y of one launch are consistent with one another"""
    y, perm, cost, status, permuted = out
    m, d = len(mapper.identical_particles), mapper.dim
    assert perm.shape == (X.shape[0], m) and np.array_equal(np.sort(perm, axis=1), np.tile(np.arange(m), (X.shape[0], 1))), label
    assert y.tobytes() == gathered(mapper, X, perm).tobytes(), f"{label}: y is not the gather of X by perm"
    assert np.array_equal(permuted, (perm != np.arange(m)).any(axis=1).astype(np.int32)), label
    c64 = cost64(mapper, X, perm)
    err, bound = np.abs(cost.astype(np.float64) - c64), (m * d + 2) * 2.0 ** -24 * c64
    worst = int(np.argmax(err - bound))
    print(f"{label}: cost error {err[worst]:.3g} (bound {bound[worst]:.3g}) at row {worst}")
    assert cost.dtype == np.float32 and np.all(err <= bound), label


@pytest.fixture(scope="module")
def runs(hip_lib, dev, golden):
    """every fixture case through one launch with all outputs, once"""
    G = golden("permutation")
    out = {}
    for c in case_list(G):
        mapper, X, want, stable, meta = case(G, c["name"])
        assert mapper._takes_kernel(torch.tensor(X, device=dev))
        out[c["name"]] = (mapper, X, want, stable, launch_all(mapper, torch.tensor(X, device=dev)))
    return out


def test_kernel_meets_the_fixture(runs):
    for name, (mapper, X, want, stable, out) in runs.items():
        check_perm(out[1], want, stable, name)
        assert not out[3].any(), f"{name}: status"
        check_outputs(mapper, X, out, name)


def test_public_methods_are_the_launch(runs, dev):
    for name in ("m36_d2_b3", "m3_d3_b257", "m64_d3_b1"):
        mapper, X, want, stable, (y, perm, cost, status, permuted) = runs[name]
        x = torch.tensor(X, device=dev)
        got_y, got_p, (got_perm, got_cost) = mapper.map(x), mapper.is_permuted(x), mapper.assignment(x)
        assert got_y.device == x.device and got_y.dtype == torch.float32 and got_y.shape == x.shape
        assert got_p.dtype == torch.bool and got_perm.dtype == torch.int64 and got_cost.dtype == torch.float32
        assert got_y.cpu().numpy().tobytes() == y.tobytes() and np.array_equal(got_p.cpu().numpy(), permuted.astype(bool))
        assert np.array_equal(got_perm.cpu().numpy(), perm) and got_cost.cpu().numpy().tobytes() == cost.tobytes()
        n, d = mapper.n_particles, mapper.dim
        assert mapper.map(x.reshape(-1, n, d)).shape == (X.shape[0], n, d) and mapper.map(x[0]).shape == (n * d,)
        assert torch.equal(mapper.map(x[0]), got_y[0])
    assert mapper.map(x[:0]).shape == (0, n * d)


def test_map_and_is_permuted_are_one_launch_each(runs, dev):
    from test_gpu_round6 import _device_kernel_names
    mapper, X = runs["m36_d2_b3"][:2]
    x = torch.tensor(X, device=dev)
    names = _device_kernel_names(lambda: mapper._launch(x, y=True, status=True))
    assert len(names) == 1 and "assign_kernel" in names[0], names
    names = _device_kernel_names(lambda: mapper._launch(x, permuted=True))
    assert len(names) == 1 and "assign_kernel" in names[0], names


def test_kernel_path_equals_the_general_path_on_stable_rows(runs):
    for name in ("m36_d2_b3", "m33_d1_b257", "m31_d1_b257", "m3_d3_b257", "m63_d3_b3"):
        mapper, X, want, stable, out = runs[name]
        general = mapper.map(X)
        assert general[stable].tobytes() == out[0][stable].tobytes(), name


def test_a_slice_of_a_wider_tensor_on_another_stream(runs, dev):
    for name in ("m36_d2_b3", "m33_d1_b257", "m2_d3_b3"):
        mapper, X, want, stable, out = runs[name]
        wide = torch.full((X.shape[0], X.shape[1] + 6), 7.0, device=dev)
        view = wide[:, 3:3 + X.shape[1]]                     # ldx > n d, 12 bytes off the allocation's alignment
        view.copy_(torch.tensor(X, device=dev))
        assert view.stride(0) > X.shape[1] and view.data_ptr() % 16 != 0
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            got = launch_all(mapper, view)
        stream.synchronize()
        for a, b in zip(got, out):
            assert a.tobytes() == b.tobytes(), name
        assert bool((wide[:, :3] == 7.0).all()) and bool((wide[:, 3 + X.shape[1]:] == 7.0).all())


def test_runs_and_batch_sizes_give_the_same_permutation(runs, dev):
    for name in ("m33_d1_b257", "m31_d1_b257", "m3_d3_b257"):
        mapper, X, want, stable, out = runs[name]
        again = launch_all(mapper, torch.tensor(X, device=dev))
        for a, b in zip(again, out):
            assert a.tobytes() == b.tobytes(), name
        for row in (0, 100, 255, 256):
            alone = launch_all(mapper, torch.tensor(X[row:row + 1], device=dev))
            for a, b in zip(alone, out):
                assert a.tobytes() == b[row:row + 1].tobytes(), (name, row)


def test_idempotence_on_the_device(runs, dev):
    for name in ("m36_d2_b3", "m33_d1_b257", "m64_d2_b3", "m3_d3_b257"):
        mapper, X, want, stable, out = runs[name]
        y = torch.tensor(out[0], device=dev)
        assert mapper.map(y).cpu().numpy().tobytes() == out[0].tobytes(), name
        assert not bool(mapper.is_permuted(y).any()), name


@pytest.mark.parametrize("m,d", [(2, 1), (8, 2), (36, 2), (64, 3)])
def test_exact_ties(hip_lib, dev, m, d):
    """two identical particles at the same position: any optimal permutation will do, its cost is scipy's optimum"""
    rng = np.random.default_rng(100 * m + d)
    n = m + 2
    xref = rng.uniform(-4, 4, (n, d)).astype(np.float32)
    X = np.empty((6, n, d), dtype=np.float32)
    for b in range(6):
        X[b] = xref + rng.standard_normal((n, d)).astype(np.float32)
        X[b, 1:m + 1] = X[b, 1:m + 1][rng.permutation(m)]
        X[b, 1 + (b % m)] = X[b, 1 + ((b + 1) % m)]          # two sample particles coincide
    xref_tied = xref.copy()
    xref_tied[2] = xref_tied[1]                              # ... and, for the second mapper, two reference positions
    X = X.reshape(6, -1)
    for ref in (xref, xref_tied):
        mapper = bg.HungarianMapper(ref.reshape(-1), dim=d, identical_particles=np.arange(1, m + 1))
        out = launch_all(mapper, torch.tensor(X, device=dev))
        check_outputs(mapper, X, out, f"ties m={m} d={d}")
        assert not out[3].any()
        best = np.array([solve_one_cost(mapper, X[b]) for b in range(6)])
        got = cost64(mapper, X, out[1])
        assert np.all(np.abs(got - best) <= (m * d + 2) * 2.0 ** -24 * best), (got, best)


def solve_one_cost(mapper, row):
    from scipy.optimize import linear_sum_assignment
    m, d = len(mapper.identical_particles), mapper.dim
    pts = row[mapper.ip_indices].astype(np.float64).reshape(m, d)
    C = ((np.asarray(mapper._ref_ip)[:, None] - pts[None]) ** 2).sum(-1)
    r, c = linear_sum_assignment(C)
    return C[r, c].sum()


def test_non_finite_rows_keep_their_order_and_leave_their_neighbours_alone(runs, dev):
    for name, rows in (("m33_d1_b257", (0, 3, 4, 130, 256)), ("m3_d3_b257", (1, 17, 18, 19, 255)), ("m36_d2_b3", (1,))):
        mapper, X, want, stable, clean = runs[name]
        X = X.copy()
        for k, b in enumerate(rows):
            X[b, mapper.ip_indices[(5 * k) % len(mapper.ip_indices)]] = (np.nan, np.inf, -np.inf)[k % 3]
        other = np.setdiff1d(np.arange(X.shape[1]), mapper.ip_indices)
        X[2, other[0]] = np.nan                              # not an identical particle's coordinate: an ordinary row
        out = launch_all(mapper, torch.tensor(X, device=dev))
        y, perm, cost, status, permuted = out
        bad = np.zeros(X.shape[0], dtype=bool)
        bad[list(rows)] = True
        assert np.array_equal(status, bad.astype(np.int32)), name
        assert np.array_equal(perm[bad], np.tile(np.arange(perm.shape[1]), (len(rows), 1))) and not permuted[bad].any()
        assert y[bad].tobytes() == X[bad].tobytes()
        assert np.array_equal(perm[~bad], clean[1][~bad]) and cost[~bad].tobytes() == clean[2][~bad].tobytes(), name
        assert y.tobytes() == gathered(mapper, X, perm).tobytes()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            mapped = mapper.map(torch.tensor(X, device=dev))
        assert len(caught) == 1 and f"{len(rows)} of {X.shape[0]}" in str(caught[0].message)
        assert mapped.cpu().numpy().tobytes() == y.tobytes()
    ref = np.array(mapper._ref64, dtype=np.float32)
    ref[mapper.ip_indices[0]] = np.nan
    status = launch_all(bg.HungarianMapper(ref, dim=mapper.dim, identical_particles=mapper.identical_particles), torch.tensor(X, device=dev))[3]
    assert status.all()


def test_fresh_inputs_at_the_packing_thresholds(hip_lib, dev):
    """m = 8, 16, 17 (the sizes either side of a change of lanes per sample) and a batch that ends inside a wavefront, drawn here"""
    for m, d in ((8, 2), (16, 3), (17, 1), (16, 1)):
        rng = np.random.default_rng(7 * m + d)
        n = m + 3
        xref = rng.uniform(-5, 5, (n, d)).astype(np.float32)
        ip = np.arange(2, m + 2)
        X = np.empty((37, n, d), dtype=np.float32)
        for b in range(37):
            X[b] = xref + (0.05, 0.5, 3.0)[b % 3] * rng.standard_normal((n, d)).astype(np.float32)
            X[b, ip] = X[b, ip][rng.permutation(m)]
        X = X.reshape(37, -1)
        mapper = bg.HungarianMapper(xref.reshape(-1), dim=d, identical_particles=ip)
        want, stable, _ = solve_rows(mapper, X)
        out = launch_all(mapper, torch.tensor(X, device=dev))
        check_perm(out[1], want, stable, f"m={m} d={d}")
        check_outputs(mapper, X, out, f"m={m} d={d}")
        assert not out[3].any()


def test_box_samples_mapped_onto_the_chains_start(hip_lib, dev, golden):
    """512 HarmonicParticles samples from the box chain kernel, every second one with its solvent labels shuffled as well, mapped onto the
    chains' initial configuration: relabelling solvent particles does not change the energy, and a mapped row is not permuted."""
    G = golden("box")
    energy = make(G, "harm", 36).to(dev)
    start = torch.tensor(G["x_36"][:1], device=dev)
    sampler, _ = fused_sampler(energy, start.repeat(512, 1).contiguous(), float(G["mc_harm_36_std"]), 1.0, stream=70)
    sampler.sample(N_FRAMES)
    X = sampler.state.as_dict()["samples"][0].clone()
    assert X.shape == (512, 76) and not torch.equal(X[0], X[1])
    gen = torch.Generator().manual_seed(5)
    cube = X.view(512, 38, 2)
    for b in range(1, 512, 2):
        cube[b, 2:] = cube[b, 2:][torch.randperm(36, generator=gen).to(dev)]
    mapper = bg.HungarianMapper(start[0], dim=2, identical_particles=np.arange(2, 38))
    assert mapper._takes_kernel(X)
    Y = mapper.map(X)
    assert bool(mapper.is_permuted(X)[1::2].all()) and not bool(mapper.is_permuted(Y).any())
    assert torch.equal(Y[:, :4], X[:, :4]) and torch.equal(Y.view(512, 38, 2)[:, 2:].sort(dim=1).values, cube[:, 2:].sort(dim=1).values)
    u, v = energy.energy(X)[:, 0].cpu().numpy(), energy.energy(Y)[:, 0].cpu().numpy()
    e, bound = err_u(v, u.astype(np.float64)), 4 * float(G["harm_36_err_u32"]) + 1e-6
    print(f"energy change under relabelling {e:.3g} (bound {bound:.3g})")
    assert e <= bound
