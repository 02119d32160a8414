"""No GPU: bgflow_amd.umbrella on the host -- the reference's classes against tests/golden/umbrella.npz part (a) (written by
tests/golden/make_umbrella_goldens.py from the reference itself), the torch path of ``mbar_solve`` against the BFGS values of part (b) and
an analytic case, the ``mbar`` grid, files, ``biased_system``, import paths, and what csrc/bgk_mbar.hip shows without a device: its
prototypes in the header, in ``abi_signatures`` and in the built library, with the argument checks.  Bounds: umbrella_common.py."""
import ctypes
import inspect
import sys

import numpy as np
import pytest
import torch
from scipy.special import ndtri

import bgflow_amd as bg
from bgflow_amd import _lib, umbrella
from bgflow_amd._abi import HEADER, abi_signatures
from bgflow_amd.build import abi_symbols

import umbrella_common as uc
from box_common import make

f64, i32, i64, p = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
WANT_SOLVE = [p, i64, i32, p, i32, i32, p, p, p, i32, f64, i32, p]
WANT_WEIGHTS = [p, i64, i32, p, i32, p, p, p]


def sampling(forward_backward, sampler=None):
    return bg.UmbrellaSampling(uc.double_well, sampler, uc.first_coordinate, uc.A_X0, uc.A_N_UMBRELLA, uc.A_K, uc.A_M_MIN, uc.A_M_MAX,
                               forward_backward=forward_backward)


@pytest.fixture(scope="module")
def seeded(golden):
    """the seeded run of fixture part (a) with this package's classes, once per value of ``forward_backward``"""
    runs = {}
    for fb in (False, True):
        np.random.seed(uc.A_SEED)
        us = sampling(fb, bg.MetropolisGauss(uc.double_well, uc.A_X0, noise=uc.A_NOISE))
        us.run(nsteps=uc.A_NSTEPS, verbose=False)
        runs[fb] = us
    return runs


# ---- the reference's classes -----------------------------------------------------------------------------------------------------------
def test_signatures_are_the_references():
    names = lambda fn: [q.name for q in inspect.signature(fn).parameters.values()]      # noqa: E731
    assert names(bg.UmbrellaModel.__init__) == ["self", "energy_function", "rc_function", "k_umbrella", "m_umbrella"]
    assert names(bg.UmbrellaSampling.__init__) == ["self", "energy_function", "sampler", "rc_function", "x0", "n_umbrella", "k", "m_min", "m_max",
                                                   "forward_backward"]
    assert inspect.signature(bg.UmbrellaSampling.__init__).parameters["forward_backward"].default is True
    got = [[q.name, q.default] for q in inspect.signature(bg.MetropolisGauss.__init__).parameters.values()][3:]
    assert got == [["temperature", 1.0], ["noise", 0.1], ["burnin", 0], ["stride", 1], ["nwalkers", 1], ["mapper", None]]
    got = [[q.name, q.default] for q in inspect.signature(bg.UmbrellaSampling.mbar).parameters.values()][1:]
    assert got == [["rc_min", None], ["rc_max", None], ["rc_bins", 50]]
    got = [[q.name, q.default] for q in inspect.signature(bg.mbar_solve).parameters.values()][3:]
    assert got == [["temperature", 1.0], ["maximum_iterations", 10000], ["tolerance", 1e-10], ["path", None]]


def test_import_paths():
    import bgflow_amd.distribution.sampling._mcmc.metropolis as metropolis
    import bgflow_amd.distribution.sampling._mcmc.umbrella_sampling as alias
    assert alias.UmbrellaSampling is bg.UmbrellaSampling and alias.UmbrellaModel is bg.UmbrellaModel
    assert metropolis.MetropolisGauss is bg.MetropolisGauss
    assert sys.modules["bgflow_amd.distribution.sampling._mcmc.umbrella_sampling"] is alias
    assert bg.umbrella.mbar_solve is bg.mbar_solve and bg.biased_system is umbrella.biased_system


@pytest.mark.parametrize("fb", [False, True])
def test_positions_and_models(golden, fb):
    G = golden("umbrella")
    key = uc.a_key(fb)
    us = sampling(fb)
    assert np.array_equal(us.umbrella_positions, G[key + "_positions"]) and us.umbrella_positions.dtype == G[key + "_positions"].dtype
    assert len(us.umbrellas) == (8 if fb else 4) and us.forward_backward is fb
    model = us.umbrellas[1]
    assert model.k_umbrella == uc.A_K and model.energy_function is uc.double_well and model.rc_function is uc.first_coordinate
    rc = G[key + "_rc_trajs"][1]
    bias = model.bias_energy(rc)
    assert bias.dtype == G[key + "_bias_energies"].dtype and np.array_equal(bias, G[key + "_bias_energies"][1])
    x = rc[:, None]
    assert np.array_equal(model.energy(x), uc.double_well(x) + bias) and np.array_equal(model(x), model.energy(x))
    xt = torch.from_numpy(x.astype(np.float64))
    assert torch.equal(model.energy(xt), uc.double_well(xt) + uc.A_K * (xt[:, 0] - model.m_umbrella) ** 2)      # tensors work alike
    D = model.to_dict()
    assert D == {"k_umbrella": uc.A_K, "m_umbrella": model.m_umbrella}
    model.rc_traj = rc
    again = bg.UmbrellaModel.from_dict(model.to_dict())
    assert again.k_umbrella == model.k_umbrella and again.m_umbrella == model.m_umbrella and again.rc_traj is rc
    assert again.energy_function is None and again.rc_function is None


@pytest.mark.parametrize("fb", [False, True])
def test_seeded_run_is_the_references(golden, seeded, fb):
    G = golden("umbrella")
    key = uc.a_key(fb)
    us = seeded[fb]
    trajs, bias = np.stack(us.rc_trajs), np.stack(us.bias_energies)
    assert trajs.dtype == G[key + "_rc_trajs"].dtype and np.array_equal(trajs, G[key + "_rc_trajs"])            # bitwise
    assert bias.dtype == G[key + "_bias_energies"].dtype and np.array_equal(bias, G[key + "_bias_energies"])
    F, want = us.umbrella_free_energies(), G[key + "_free_energies"]
    print(f"{key}: free energies {F}, reference {want}, difference {np.abs(F - want).max():.2e} (bound {uc.chain_bound(want):.2e})")
    assert F.dtype == want.dtype and F.shape == want.shape and F[0] == 0
    assert np.abs(F - want).max() <= uc.chain_bound(want)


def test_metropolis_gauss_walkers_burnin_and_stride():
    np.random.seed(3)
    mc = bg.MetropolisGauss(uc.double_well, uc.A_X0, noise=0.3, burnin=4, stride=3, nwalkers=5, temperature=2.0)
    assert mc.traj_ == [] and mc.x.shape == (5, 1)
    mc.run(nsteps=20)
    assert mc.step == 20 and len(mc.trajs) == 5 and mc.traj.shape == (5, 1) and mc.traj.dtype == np.float32      # steps 6, 9, .., 18
    assert len(mc.etrajs) == 5 and mc.etraj.shape == (5,)
    assert np.allclose(mc.etrajs[2], uc.double_well(mc.trajs[2].astype(np.float64)), rtol=1e-5, atol=1e-5)
    after = np.random.rand()
    np.random.seed(3)                       # the calls the reference makes: per step randn(walkers, dim), then ONE rand() for all walkers
    for _ in range(20):
        np.random.randn(5, 1)
        np.random.rand()
    assert np.random.rand() == after


# ---- mbar_solve, torch path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", list(uc.B_CASES))
def test_torch_path_meets_bfgs(golden, case, dtype):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES[case]
    r = bg.mbar_solve(uc.b_tensors(G, case, dtype), centres, k, tolerance=uc.B_TOLERANCE)
    assert torch.is_tensor(r.f) and r.f.device.type == "cpu"
    f = uc.check_case(G, case, r, f"torch {dtype} ")
    if case == "k1":
        assert r.iterations == 1 and np.array_equal(f, [0.0])
        rc = G["k1_rc"].astype(np.float64)
        assert np.allclose(r.log_weights.numpy(), -(np.log(37.0) - k * (rc - centres[0]) ** 2), rtol=0, atol=1e-14)


def test_numpy_input_and_temperature(golden):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES["k5"]
    r = bg.mbar_solve(uc.b_split(G, "k5"), centres, [k] * 5, tolerance=uc.B_TOLERANCE)
    assert isinstance(r.f, np.ndarray) and isinstance(r.log_weights, np.ndarray)
    uc.check_case(G, "k5", r, "numpy ")
    hot = bg.mbar_solve(uc.b_split(G, "k5"), centres, 3.0 * k, temperature=3.0, tolerance=uc.B_TOLERANCE)      # only k / T enters
    assert np.array_equal(hot.f, r.f) and hot.iterations == r.iterations
    forced = bg.mbar_solve(uc.b_tensors(G, "k5", torch.float32), centres, k, tolerance=uc.B_TOLERANCE, path="torch")
    assert np.array_equal(forced.f.numpy(), r.f)                       # f32 in: the exact widening
    small = umbrella.TORCH_CHUNK_ELEMENTS
    try:                                                               # slices of 7 samples: the same sums in another order
        umbrella.TORCH_CHUNK_ELEMENTS = 35
        sliced = bg.mbar_solve(uc.b_split(G, "k5"), centres, k, tolerance=uc.B_TOLERANCE)
    finally:
        umbrella.TORCH_CHUNK_ELEMENTS = small
    assert np.abs(sliced.f - r.f).max() <= uc.path_bound(G, "k5") and np.abs(sliced.log_weights - r.log_weights).max() <= 1e-11


def test_analytic_harmonic_case():
    """u = x^2 / 2 under k (x - m)^2 is a Gaussian of mean k m / (0.5 + k) and variance 0.5 / (0.5 + k), and
    f_k - f_0 = 0.5 k (m_k^2 - m_0^2) / (0.5 + k).  257 samples per window at the quantiles ppf((i + 0.5) / 257): the f64 numpy
    restatement of the iteration converges in 23 iterations at 1e-10 and is 9.2e-4 off the formula -- quadrature error of the
    quantile rule, not noise -- so 5e-3 is asserted."""
    k, m = 1.0, np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    q = ndtri((np.arange(257) + 0.5) / 257)
    trajs = [k * c / (0.5 + k) + np.sqrt(0.5 / (0.5 + k)) * q for c in m]
    r = bg.mbar_solve(trajs, m, k)
    want = 0.5 * k * (m ** 2 - m[0] ** 2) / (0.5 + k)
    print(f"analytic: iterations {r.iterations}, f {r.f}, off the formula by {np.abs(r.f - want).max():.2e}")
    assert r.status == umbrella.CONVERGED and r.iterations == 23
    assert np.abs(r.f - want).max() <= 5e-3
    # the weights undo the bias: the reweighted mean of x^2 is the unbiased ensemble's, 1
    w = np.exp(r.log_weights - r.log_weights.max())
    assert abs(float((w * np.concatenate(trajs) ** 2).sum() / w.sum()) - 1.0) <= 0.05


def test_statuses_and_argument_errors(golden):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES["k5"]
    trajs = uc.b_split(G, "k5")
    short = bg.mbar_solve(trajs, centres, k, maximum_iterations=3, tolerance=uc.B_TOLERANCE)
    assert short.status == umbrella.BUDGET and short.iterations == 3 and short.err > uc.B_TOLERANCE and np.isfinite(short.f).all()
    planted = [t.copy() for t in trajs]
    planted[2][5] = np.nan
    bad = bg.mbar_solve(planted, centres, k)
    assert bad.status == umbrella.NOT_A_NUMBER and bad.iterations == 1 and np.isnan(bad.err) and np.isnan(bad.f).any()
    planted[2][5] = np.inf
    assert bg.mbar_solve(planted, centres, k).status == umbrella.NOT_A_NUMBER
    with pytest.raises(ValueError, match="no samples"):
        bg.mbar_solve(trajs[:2] + [np.zeros(0, np.float32)] + trajs[3:], centres, k)
    with pytest.raises(ValueError):
        bg.mbar_solve(trajs, centres[:4], k)
    with pytest.raises(ValueError):
        bg.mbar_solve(trajs, centres, [k] * 4)
    with pytest.raises(ValueError):
        bg.mbar_solve(trajs, centres, k, maximum_iterations=0)
    with pytest.raises(ValueError):
        bg.mbar_solve(trajs, centres, k, temperature=0.0)
    with pytest.raises(ValueError):
        bg.mbar_solve(trajs, centres, k, path="fast")
    with pytest.raises(ValueError, match="kernel path"):
        bg.mbar_solve(trajs, centres, k, path="kernel")               # numpy arrays: no kernel


# ---- UmbrellaSampling.mbar, files --------------------------------------------------------------------------------------------------
def test_mbar_grid_states_and_weights(seeded):
    us = seeded[True]
    rc = np.concatenate(us.rc_trajs)
    xgrid_mean, F = us.mbar(rc_bins=12)
    grid = np.linspace(float(rc.min()), float(rc.max()), 12)          # the grid is f64 whatever the samples' dtype
    want_grid = np.concatenate([grid, [2 * grid[-1] - grid[-2]]]) - 0.5 * (grid[1] - grid[0])
    assert np.array_equal(xgrid_mean, want_grid) and F.shape == (13,)
    assert us.rc_discretization is xgrid_mean and us.rc_free_energies is F
    states = np.digitize(rc, grid)
    assert states.min() == 1 and states.max() == 12                    # nothing below the first grid point; the maximum alone in state 12
    w = np.concatenate(us.mbar_weights())
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1.0) <= 1e-6 and [v.shape for v in us.mbar_weights()] == [t.shape for t in us.rc_trajs]
    log_w = us._solve().log_weights
    w64 = np.exp(log_w - log_w.max())
    w64 /= w64.sum()
    want = np.array([w64[states == s].sum() for s in range(13)])
    assert np.isposinf(F[0]) and np.isfinite(F[1:]).all()             # state 0 is empty
    assert np.allclose(np.exp(-F), want, rtol=1e-12, atol=0) and abs(np.exp(-F).sum() - 1.0) <= 1e-12
    # a grid wider than the data: empty states on both sides, and the double well's barrier at 0 lies above its minima
    xg, F2 = us.mbar(rc_min=-3.0, rc_max=3.0, rc_bins=25)
    assert np.isposinf(F2[0]) and np.isposinf(F2[-1]) and np.isposinf(F2[1]) and xg.shape == (26,)
    centre, left, right = F2[np.argmin(np.abs(xg))], F2[np.argmin(np.abs(xg + 1.0))], F2[np.argmin(np.abs(xg - 1.0))]
    assert np.isfinite([centre, left, right]).all() and centre > left + 0.5 and centre > right + 0.5
    # the same through tensors on the CPU (the torch ops of the device route)
    ut = sampling(True)
    for u, t in zip(ut.umbrellas, us.rc_trajs):
        u.rc_traj = torch.from_numpy(t)
    xg_t, F_t = ut.mbar(rc_min=-3.0, rc_max=3.0, rc_bins=25)
    assert np.array_equal(xg_t, xg) and np.array_equal(np.isinf(F_t), np.isinf(F2)) and np.allclose(F_t[np.isfinite(F_t)], F2[np.isfinite(F2)], rtol=0, atol=1e-9)
    wt = ut.mbar_weights()
    assert wt[0].dtype == torch.float32 and np.allclose(torch.cat(wt).numpy(), w, rtol=1e-5, atol=0)
    centres, Es = bg.free_energy_bootstrap(torch.cat(ut.rc_trajs), -1.5, 1.5, 7, sample=4, weights=torch.cat(wt), seed=1)
    assert Es.shape == (4, 6) and torch.isfinite(Es).all()


def test_save_and_load(tmp_path, seeded):
    us = seeded[False]
    us.mbar(rc_bins=10)
    us.save(tmp_path / "run")                                          # numpy appends .npz
    back = bg.UmbrellaSampling.load(tmp_path / "run")
    assert back.forward_backward is False and back.temperature == 1.0 and back.sampler is None and back.energy_function is None
    assert np.array_equal(back.umbrella_positions, us.umbrella_positions) and [u.k_umbrella for u in back.umbrellas] == [uc.A_K] * 4
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(back.rc_trajs, us.rc_trajs))
    assert np.array_equal(back.rc_discretization, us.rc_discretization) and np.array_equal(back.rc_free_energies, us.rc_free_energies)
    assert np.array_equal(back.umbrella_free_energies(), us.umbrella_free_energies())
    assert np.array_equal(back.mbar(rc_bins=10)[1], us.rc_free_energies)
    fresh = sampling(True)                                             # nothing sampled yet: positions only
    fresh.save(str(tmp_path / "empty.npz"))
    empty = bg.UmbrellaSampling.load(str(tmp_path / "empty.npz"))
    assert empty.forward_backward is True and len(empty.umbrellas) == 8 and not hasattr(empty.umbrellas[0], "rc_traj") and not hasattr(empty, "rc_discretization")


# ---- the box -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rep", "harm"])
def test_biased_system(golden, kind):
    G = golden("box")
    system = make(G, kind, 2)
    before = dict(system.params)
    k, m = 50.0, 1.2
    biased = bg.biased_system(system, k, m)
    assert type(biased) is type(system) and biased.params is not system.params and system.params == before
    assert biased.params["dimer_slope"] == before["dimer_slope"] + k * (before["dimer_dmid"] - m) and biased.params["dimer_a"] == before["dimer_a"] - k / 4
    assert {key: v for key, v in biased.params.items() if key not in ("dimer_slope", "dimer_a")} == {key: v for key, v in before.items() if key not in ("dimer_slope", "dimer_a")}
    if kind == "harm":
        assert biased.spring_constant == system.spring_constant == float(G["spring_constant"])
    x = torch.tensor(G["x_2"], dtype=torch.float64)
    d = system.dimer_distance(x)
    want = k * (d - m) ** 2 - k * (before["dimer_dmid"] - m) ** 2
    got = (biased.energy(x) - system.energy(x)).reshape(-1)
    scale = 1.0 + float(biased.energy(x).abs().max())
    print(f"{kind}: |difference - umbrella| {float((got - want).abs().max()):.2e} at energies up to {scale:.3g}")
    assert float((got - want).abs().max()) <= 64 * 2.0 ** -52 * scale        # f64 rounding of two energies of that size
    with pytest.raises(TypeError):
        bg.biased_system(bg.DoubleWellEnergy(2), k, m)


def test_for_box_on_the_cpu_torch_path(golden):
    """the settings of the GPU test (test_gpu_umbrella.py) through the same classes on CPU tensors (torch ops, no kernel): the window
    means of the dimer distance are separated by many standard errors"""
    G = golden("box")
    system = make(G, "rep", 2)
    torch.manual_seed(11)
    x0 = torch.tensor(G["x_2"][:1]).repeat(16, 1)
    us = bg.UmbrellaSampling.for_box(system, x0, 3, 50.0, 1.0, 2.0, forward_backward=False)
    us.run(60, verbose=False)
    assert [u.m_umbrella for u in us.umbrellas] == [1.0, 1.5, 2.0] and us.temperature == 1.0
    means = [float(t.mean()) for t in us.rc_trajs]
    sds = [float(t.std()) for t in us.rc_trajs]
    print(f"for_box on the CPU: means {means}, standard deviations {sds}")
    assert all(t.shape == (16 * 60,) and torch.isfinite(t).all() for t in us.rc_trajs)
    assert means[0] < means[1] < means[2]
    xg, F = us.mbar(rc_bins=8)
    assert np.isfinite(F[1:]).sum() >= 4
    with pytest.raises(ValueError):
        sampling(False, bg.MetropolisGauss(uc.double_well, uc.A_X0)).run(5, verbose=False, stride=2)


# ---- the C entries -----------------------------------------------------------------------------------------------------------------
def test_the_prototypes_are_declared_parsed_and_exported(hip_lib):
    sigs = abi_signatures()
    for name, want in (("bgk_mbar_solve_steps", WANT_SOLVE), ("bgk_mbar_log_weights", WANT_WEIGHTS)):
        assert sigs[name] == (ctypes.c_int, want)
        assert name in abi_symbols()
        assert list(getattr(hip_lib, name).argtypes) == want
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), name), ctypes.c_void_p).value, f"{name} is not exported"
    with open(HEADER) as f:
        header = f.read()
    assert f"#define BGK_MBAR_RECORD_DOUBLES {umbrella.RECORD_DOUBLES}\n" in header
    assert "#define BGK_MBAR_F32 0\n" in header and "#define BGK_MBAR_F64 1\n" in header and umbrella._DTYPE_CODES == {torch.float32: 0, torch.float64: 1}


def test_argument_checks_of_the_entries(hip_lib):
    uc.check_entry_arguments(hip_lib)
