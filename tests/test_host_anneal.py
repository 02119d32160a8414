"""Host (no GPU): annealed switching -- the general path of ``AnnealedSwitching`` in f64 against the reference's ``MCMCStep`` driven stage by
stage on recorded numbers (tests/golden/anneal.npz, written by tests/golden/make_anneal_goldens.py), ``reverse()``, the single-energy
schedule, the zero-coefficient rule, ``AnnealedMCFlow`` inside a ``BoltzmannGenerator``, argument validation, the C ABI of
csrc/bgk_anneal.hip as the header declares it, and a statistical check against an analytic free-energy difference."""
import ctypes
import math

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import annealing, sampling
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols

from anneal_common import B, CASES, bar_check, make_end, start_state, switching
from mcmc_common import RecordedProposal, random_numbers, recorded_uniforms


@pytest.mark.parametrize("key", list(CASES))
def test_general_path_reproduces_the_recorded_protocol(golden, key):
    G = golden("anneal")
    sw, x0 = switching(golden, key, dtype=torch.float64)
    start = x0.clone()
    x, work = sw(x0)
    assert torch.equal(x0, start) and x.dtype == torch.float64 and work.dtype == torch.float64 and work.shape == (B,)
    assert sw.n_proposed == 12 and sw.n_accepted.dtype == torch.int32
    assert np.array_equal(sw.n_accepted.numpy(), G[key + "_acc"])
    w64 = G[key + "_work64"]
    assert np.abs(work.numpy() - w64).max() <= 1e-12 * (1 + np.abs(w64).max())
    assert np.abs(x.numpy()[:8] - G[key + "_x64"]).max() <= 1e-12
    for got, want in ((sw.e_a, G[key + "_e_a64"]), (sw.e_b, G[key + "_e_b64"])):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * (1 + np.abs(want).max())
    # the records are the ends' energies of the returned state
    assert torch.equal(sw.e_a, sw.energy_a.energy(x)[:, 0]) and torch.equal(sw.e_b, sw.energy_b.energy(x)[:, 0])


def test_fixture_conditions(golden):
    G = golden("anneal")
    lam = G["lambdas"]
    assert len(lam) == 7 and lam[0] == 0.0 and lam[-1] == 1.0 and len(set(np.diff(lam).round(6))) > 1 and int(G["n_steps"]) == 2
    for key in CASES:
        assert G[key + "_keep"].mean() >= 0.85 and G[key + "_work64"].shape == (B,) and G[key + "_x64"].shape[0] == 8


def test_reverse_mirrors_ends_and_schedule(golden):
    sw, _ = switching(golden, "lj_lj_13_3")
    rv = sw.reverse()
    assert rv.energy_a is sw.energy_b and rv.energy_b is sw.energy_a
    assert rv.temperature_a == sw.temperature_b == 2.0 and rv.temperature_b == sw.temperature_a == 1.0
    assert rv.lambdas == [1.0 - v for v in reversed(sw.lambdas)] and rv.lambdas[0] == 0.0 and rv.lambdas[-1] == 1.0
    assert rv.n_steps == sw.n_steps and rv.noise_std == sw.noise_std and rv._fed is None
    # stage m of the reverse protocol has the coefficients of stage M - m, with the ends' columns swapped
    assert torch.allclose(rv.schedule, sw.schedule.flip(0).flip(1), rtol=1e-6, atol=0)
    assert sw.schedule.dtype == torch.float32 and sw.schedule.shape == (7, 2)
    want = torch.tensor(sw.lambdas, dtype=torch.float64)
    assert torch.equal(sw.schedule, torch.stack([(1 - want) / 1.0, want / 2.0], 1).float())
    sw.fused = "always"
    assert sw.reverse().fused == "always" and bg.AnnealedSwitching.fused is True


def test_a_constant_schedule_is_the_plain_chain_with_zero_work(golden):
    P = golden("particles")
    n, d, steps = 4, 2, 6
    lj, mdw = make_end(P, ("lj", n, d)), make_end(P, ("mdw", n, d))
    x0 = torch.tensor(start_state(golden, ("lj", n, d)))
    noise, unif = (torch.tensor(t) for t in random_numbers(31, n * d, steps, B))
    for lambdas, target in (([0.0, 0.0, 0.0], lj), ([1.0, 1.0, 1.0], mdw)):
        sw = bg.AnnealedSwitching(lj, mdw, lambdas, n_steps=3, noise_std=0.15).feed_noise(noise, unif)
        x, work = sw(x0)
        plain = bg.MCMCStep(target, proposal=RecordedProposal(noise, 0.15), n_steps=steps)
        with recorded_uniforms(unif):
            want = plain(bg.SamplerState(samples=x0)).as_dict()
        assert torch.equal(work, torch.zeros(B, dtype=torch.float64))
        assert torch.equal(x, want["samples"][0]) and torch.equal(sw.n_accepted, plain.n_accepted)
        assert 0 < int(sw.n_accepted.sum()) < steps * B
        assert torch.equal(sw.e_a if target is lj else sw.e_b, want["energies"])


def coincident_box_rows(golden):
    """start states of the box of 2 solvent particles; in row 0 solvent particle 3 sits on solvent particle 2: the repulsive energy is +inf"""
    x0 = torch.tensor(start_state(golden, ("rep", 2)))[:8].clone()
    x0[0, 6:8] = x0[0, 4:6]
    return x0


def test_the_zero_coefficient_rule(golden):
    """A = the harmonic box (finite at coincident particles), B = the repulsive box: e_B = +inf in row 0 at lambda_0 = 0, where its
    coefficient is 0.  The row gets work = +inf, moves on at the first proposal that separates the particles, and no NaN reaches x"""
    P = golden("particles")
    x0 = coincident_box_rows(golden)
    harm, rep = make_end(P, ("harm", 2)), make_end(P, ("rep", 2))
    assert torch.isinf(rep.energy(x0)[0, 0]) and torch.isfinite(harm.energy(x0)).all()
    noise, unif = (torch.tensor(t) for t in random_numbers(37, 8, 4, 8))
    sw = bg.AnnealedSwitching(harm, rep, [0.0, 0.5, 1.0], n_steps=2, noise_std=0.05).feed_noise(noise, unif)
    x, work = sw(x0)
    assert work[0] == float("inf") and torch.isfinite(work[1:]).all()
    assert torch.isfinite(x).all() and int(sw.n_accepted[0]) >= 1 and not torch.equal(x[0], x0[0])
    assert torch.isfinite(sw.e_a).all() and torch.isfinite(sw.e_b).all()
    # the reduced energy of the first stage's start state is finite: the term of the zero coefficient is dropped
    assert torch.isfinite(bg.InterpolatedEnergy(harm, rep, lam=0.0).energy(x0)).all()
    assert torch.isinf(bg.InterpolatedEnergy(harm, rep, lam=0.5).energy(x0)[0, 0])
    # a schedule that never turns B on: its infinite energy never enters, neither the chain nor the work
    sw = bg.AnnealedSwitching(harm, rep, [0.0, 0.0], n_steps=2, noise_std=0.05).feed_noise(noise, unif)
    x, work = sw(x0)
    assert torch.equal(work, torch.zeros(8, dtype=torch.float64)) and torch.isfinite(x).all()
    # NaN noise: every proposal is rejected, the states stay
    sw = bg.AnnealedSwitching(harm, rep, [0.0, 1.0], n_steps=1, noise_std=0.05).feed_noise(torch.full((1, 8, 8), float("nan")), unif[:1])
    x, work = sw(x0)
    assert torch.equal(x, x0) and int(sw.n_accepted.sum()) == 0 and work[0] == float("inf")


def test_interpolated_energy_is_a_target_of_the_samplers(golden):
    P = golden("particles")
    lj, mfn = make_end(P, ("lj", 4, 2)), make_end(P, ("mfn", 4, 2))
    x0 = torch.tensor(start_state(golden, ("lj", 4, 2))).double()
    mix = bg.InterpolatedEnergy(mfn, lj, lam=0.25, temperature_a=1.0, temperature_b=2.0)
    c = annealing.anneal_coefficients([0.25], 1.0, 2.0)[0].tolist()
    assert torch.allclose(mix.energy(x0), c[0] * mfn.energy(x0) + c[1] * lj.energy(x0), rtol=1e-14, atol=0)
    mix.lam = 1.0
    assert torch.equal(mix.energy(x0), 0.5 * lj.energy(x0))
    out = bg.MCMCStep(mix, proposal=bg.GaussianProposal(0.1), n_steps=2)(bg.SamplerState(samples=x0)).as_dict()
    assert out["samples"][0].shape == x0.shape and torch.isfinite(out["energies"]).all()


def test_annealed_mc_flow_inside_a_boltzmann_generator(golden):
    P = golden("particles")
    n, d = 4, 2
    prior, target = make_end(P, ("mfn", n, d)), make_end(P, ("lj", n, d))
    lambdas = [0.0, 0.3, 0.7, 1.0]
    flow = bg.AnnealedMCFlow(prior, target, lambdas, nsteps=2, stepsize=0.1)
    gen = bg.BoltzmannGenerator(prior, flow, target)
    z = torch.tensor(start_state(golden, ("lj", n, d))).double()
    noise, unif = (torch.tensor(t) for t in random_numbers(41, n * d, 6, B))
    flow.switching.feed_noise(noise, unif)
    x, dW = flow(z)
    assert dW.shape == (B, 1) and dW.dtype == torch.float64
    _, work = bg.AnnealedSwitching(prior, target, lambdas, n_steps=2, noise_std=0.1).feed_noise(noise, unif)(z)
    logw = gen.log_weights_given_latent(x, z, dW, normalize=False)
    assert (logw + work).abs().max() <= 1e-10 * (1 + work.abs().max())
    # the inverse runs the mirrored protocol with the mirrored dW
    flow.switching_reverse.feed_noise(noise, unif)
    y, dW_r = flow(z, inverse=True)
    rv = flow.switching.reverse().feed_noise(noise, unif)
    y2, work_r = rv(z)
    want = prior.energy(y2)[:, 0] - target.energy(z)[:, 0] - work_r
    assert torch.equal(y, y2) and (dW_r[:, 0] - want).abs().max() <= 1e-10 * (1 + want.abs().max())
    # A identical to B: MetropolisMCFlow's E - E0
    same = bg.AnnealedMCFlow(target, target, [0.0, 0.5, 1.0], nsteps=3, stepsize=0.1)
    same.switching.feed_noise(noise, unif)
    x, dW = same(z)
    plain = bg.MetropolisMCFlow(target, nsteps=6, stepsize=0.1).feed_noise(noise, unif)
    x2, dW2 = plain(z)
    assert torch.equal(x, x2) and (dW - dW2).abs().max() <= 1e-6 * (1 + dW2.abs().max())
    # an input that requires grad runs the torch path and stays differentiable
    zg = z[:8].clone().requires_grad_(True)
    flow.switching.feed_noise(noise[:, :8].contiguous(), unif[:, :8].contiguous())
    xg, dWg = flow(zg)
    (g,) = torch.autograd.grad(dWg.sum(), zg)
    assert g.shape == zg.shape and torch.isfinite(g).all()


def test_ais_and_jarzynski():
    torch.manual_seed(5)
    prior = bg.MeanFreeNormalDistribution(8, 4, std=1.0, two_event_dims=False)
    target = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False)
    x, logw = bg.annealed_importance_sampling(prior, target, 256, [0.0, 0.5, 1.0], n_steps=2, noise_std=0.3)
    assert x.shape == (256, 8) and logw.shape == (256,) and logw.dtype == torch.float64
    x0 = prior.sample(16)
    torch.manual_seed(6)
    x1, lw1 = bg.annealed_importance_sampling(prior, target, x0, [0.0, 1.0])
    torch.manual_seed(6)
    x2, w2 = bg.AnnealedSwitching(prior, target, [0.0, 1.0])(x0)
    assert torch.equal(x1, x2) and torch.equal(lw1, -w2)
    w = torch.tensor([0.3, -0.2, 1.5, 0.0], dtype=torch.float64)
    assert abs(float(bg.jarzynski_free_energy(w)) - (-math.log(float(torch.exp(-w).mean())))) <= 1e-14
    assert abs(float(bg.jarzynski_free_energy(torch.full((7,), 2.5))) - 2.5) <= 1e-14


def test_argument_validation(golden):
    P = golden("particles")
    lj, mfn = make_end(P, ("lj", 4, 2)), make_end(P, ("mfn", 4, 2))
    for bad in ([0.5], [], [0.0, 1.5], [-0.1, 1.0], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            bg.AnnealedSwitching(mfn, lj, bad)
    for kwargs in (dict(n_steps=0), dict(n_steps=1.5), dict(n_steps=True), dict(temperature_a=0.0), dict(temperature_b=-1.0),
                   dict(temperature_a=torch.tensor(1.0)), dict(noise_std=-0.1)):
        with pytest.raises(ValueError):
            bg.AnnealedSwitching(mfn, lj, [0.0, 1.0], **kwargs)
    with pytest.raises(ValueError):
        bg.InterpolatedEnergy(mfn, make_end(P, ("lj", 13, 3)))
    with pytest.raises(ValueError):
        bg.InterpolatedEnergy(mfn, lj, temperature_a=0.0)
    sw = bg.AnnealedSwitching(mfn, lj, [0.0, 0.5, 1.0], n_steps=2)
    with pytest.raises(ValueError):
        sw.feed_noise(torch.zeros(4, 3, 8), None)
    with pytest.raises(ValueError):
        sw.feed_noise(torch.zeros(4, 3, 8), torch.zeros(4, 2))
    sw.feed_noise(torch.zeros(3, 5, 8), torch.full((3, 5), 0.5))
    with pytest.raises(ValueError, match="4 steps"):
        sw(torch.zeros(5, 8))                      # four steps need four rows
    assert sw.feed_noise(None, None)._fed is None
    # the general path takes any energy: a fused setup is never claimed on the host
    assert sw._fused_setup(torch.zeros(5, 8)) is None
    assert annealing.ANNEAL_MAX_STEPS_PER_LAUNCH >= 1 and "AnnealedSwitching" in sampling.__doc__
    for name in ("InterpolatedEnergy", "AnnealedSwitching", "annealed_importance_sampling", "jarzynski_free_energy", "AnnealedMCFlow"):
        assert hasattr(bg, name)
    assert bg.annealing is annealing and bg.AnnealedMCFlow is bg.stochastic.AnnealedMCFlow


def test_the_default_takes_the_kernel_where_it_was_measured_faster(golden):
    """``fused = True``: tiles of the full 64 rows (n d <= 123), the shapes tools/anneal_time.py measured faster than the general path"""
    from bgflow_amd.distributions import _kernel_plan
    P = golden("particles")

    def plan(end):
        return _kernel_plan(make_end(P, end), 1.0)

    assert annealing.ANNEAL_FUSED_MIN_ROWS == 64 and annealing.ANNEAL_MAX_STEPS_PER_LAUNCH == sampling.MCMC_MAX_STEPS_PER_LAUNCH // 2
    assert annealing.anneal_fused_by_default(plan(("mfn", 13, 3)), plan(("lj", 13, 3)))
    assert annealing.anneal_fused_by_default(plan(("lj", 4, 2)), plan(("mdw", 4, 2)))
    assert not annealing.anneal_fused_by_default(plan(("mfn", 64, 3)), plan(("lj", 64, 3)))          # 41 rows: measured slower
    assert annealing.anneal_fused_by_default(plan(("rep", 36)), plan(("biased", 36)))                 # the box of 38: 64 rows
    assert not annealing.anneal_fused_by_default(plan(("rep", 62)), plan(("harm", 62)))               # the box of 64: 61 rows
    assert [sampling.mcmc_tile_rows(3 * n) for n in (41, 42)] == [64, 62]                             # 63,488 // (8 * 127) = 62


def test_c_abi_and_argument_checks(hip_lib):
    """the header-derived signatures of both entries, and the argument checks, which return before any device work"""
    sigs = abi_signatures()
    i32, i64, u32, u64, f64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p
    tail = [p, i32, i32, i32, i32, f64, p, p, u64, u32, i64, p, p, i32, p, p, i32, p]
    end = [i32, f64, f64, f64, f64, f64]
    want = {"bgk_pair_anneal": [p, i64, i32, i32] + end + end + tail, "bgk_box_anneal": [p, i64, i32] + [i32, p, i32] * 2 + tail}
    for name, args in want.items():
        assert name in abi_symbols() and sigs[name] == (ctypes.c_int, args)
        assert list(getattr(hip_lib, name).argtypes) == args
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def pair(batch=0, n=13, d=3, ka=2, kb=0, M=6, K=2, begin=0, end=12, std=0.1, noise=None, unif=None):
        return hip_lib.bgk_pair_anneal(fake, batch, n, d, ka, 0.0, 0.0, 0.0, 0.0, 1.0, kb, 1.0, 1.0, 0.0, 0.0, 0.5, fake, M, K, begin, end,
                                       std, noise, unif, 1, 0, 0, fake, fake, 0, fake, None, 0, None)

    prm = (ctypes.c_float * 12)(0.7, 1.21, 0.9, 0.81, 150.0, -1.0, 25.0, 10.0, 1.5, 20.0, 3.0, 100.0)

    def box(batch=0, n=38, ka=3, kb=4, M=6, K=2, begin=0, end=12, std=0.1, noise=None, unif=None, n_params=12):
        return hip_lib.bgk_box_anneal(fake, batch, n, ka, prm, 12, kb, prm, n_params, fake, M, K, begin, end, std, noise, unif, 1, 0, 0,
                                      fake, fake, 0, fake, None, 0, None)

    for entry in (pair, box):
        assert entry() == 0                                                        # an empty batch: nothing to do
        for bad in (dict(M=0), dict(K=0), dict(begin=-1), dict(begin=5, end=4), dict(end=13), dict(std=-0.1), dict(std=float("nan")),
                    dict(noise=fake), dict(unif=fake), dict(batch=-1)):
            assert entry(**bad) == -1, bad
        assert entry(noise=fake, unif=fake) == 0 and entry(begin=5, end=7) == 0 and entry(batch=8, begin=3, end=3) == 0
        assert entry(n=65) == -2 and b"envelope" in hip_lib.bgk_last_error()
        assert entry(n=1) == -2 and b"envelope" in hip_lib.bgk_last_error()
    assert pair(d=4) == -2 and pair(ka=3) == -1 and pair(kb=4) == -1 and box(ka=2) == -1 and box(kb=0) == -1 and box(n_params=11) == -1
    for ka in (0, 1, 2):
        for kb in (0, 1, 2):
            for d in (1, 2, 3):
                assert pair(ka=ka, kb=kb, d=d) == 0
    # the tile heights are the chain kernel's
    assert [sampling.mcmc_tile_rows(nd) for nd in (192, 39, 76, 128)] == [41, 64, 64, 61]


def test_bar_of_forward_and_reverse_work_against_the_analytic_answer():
    """mean-free normals of 4 particles in 2 dimensions, sigma_A = 1.0 -> sigma_B = 0.8: the reduced free-energy difference is
    -(n - 1) d ln(sigma_B / sigma_A) = -6 ln 0.8 = 1.3389.  A numpy run of this protocol gave BAR 1.3344 +- 0.0054; the forward Jarzynski
    standard error was 0.007."""
    torch.manual_seed(2026)
    prior = bg.MeanFreeNormalDistribution(8, 4, std=1.0, two_event_dims=False)
    target = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False)
    df, ddf, exact, sw, rv = bar_check(prior, target, prior.sample(4096), target.sample(4096), fused=True)
    jar = float(bg.jarzynski_free_energy(sw(prior.sample(4096))[1]))
    print(f"BAR {df:.4f} +- {ddf:.4f}, Jarzynski {jar:.4f}, exact {exact:.4f}")
    assert abs(df - exact) <= 5 * ddf
    assert ddf <= 0.02
    assert abs(jar - exact) <= 0.05
