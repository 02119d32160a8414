"""Host: Hamiltonian Monte Carlo in bgflow_amd.sampling -- the general path of ``HamiltonianProposal`` / ``HMCStep`` (torch ops over
``energy.force``) against the recorded f64 chains of tests/golden/hmc.npz (written by tests/golden/make_hmc_goldens.py), the leapfrog
rule on a linear force, the shortcut classes, the guards of the fused path and the C ABI of csrc/bgk_hmc.hip as the header declares it."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols

from hmc_common import B, CASES, IDS, N_FRAMES, N_STEPS, case_numbers, case_settings, key_of, make, recorded_normals, run_general


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_general_path_reproduces_the_recorded_chains(golden, case):
    """f64 on the CPU, the fixture's random numbers -- the same arithmetic in the same order: the same decisions, and states to 1e-10,
    on EVERY chain"""
    G, key = golden("hmc"), key_of(case)
    energy, x0 = make(golden, case)
    noise, unif = case_numbers(golden, case, x0.shape[1])
    frames, sampler, step = run_general(energy, torch.from_numpy(x0).double(), torch.from_numpy(noise), torch.from_numpy(unif),
                                        case_settings(G, key, torch.float64, "cpu"))
    assert frames.shape == (N_FRAMES, B, x0.shape[1]) and frames.dtype == torch.float64
    assert np.array_equal(step.n_accepted.numpy(), G[key + "acc"]) and step.n_proposed == N_STEPS
    state = sampler.state.as_dict()
    assert state["energies_up_to_date"]
    x = state["samples"][0].numpy()
    assert np.abs(x[G[key + "rows"]] - G[key + "x64"]).max() <= 1e-10
    e64 = G[key + "e64"]
    assert np.max(np.abs(state["energies"].numpy() - e64) / (1 + np.abs(e64))) <= 1e-10
    assert np.abs(frames[:, :8].numpy() - G[key + "frames64"]).max() <= 1e-10
    assert np.array_equal(frames[-1].numpy(), x)


def test_fixture_conditions(golden):
    G = golden("hmc")
    for case in CASES:
        key = key_of(case)
        rate = G[key + "acc"].mean() / N_STEPS
        assert G[key + "keep"].mean() >= 0.85 and 0.3 <= rate <= 0.95, (case, rate)
        assert int(G[key + "n_leapfrog"]) == (1 if case[1:] == (2, 1) else 5)
    assert float(G["mfn_13_3_mass"]) == 2.5 and G["mdw_13_3_temps"].shape == (B,)


def test_leapfrog_on_a_linear_force_is_reversible():
    """a unit normal (f = -x / T) at T = 2: delta_log_prob is [B], the state carries no graph, and the trajectory run again from the end
    point with the final momentum reversed returns to the start to f64 round-off"""
    torch.manual_seed(0)
    energy = bg.NormalDistribution(5)
    h, L, m, T = 0.3, 7, 1.7, 2.0
    proposal = bg.HamiltonianProposal(energy, h, n_leapfrog=L, mass=m, temperature=T)
    x0 = torch.randn(9, 5, dtype=torch.float64, requires_grad=True)
    xi = torch.randn(1, 9, 5, dtype=torch.float64)
    with recorded_normals(xi):
        new, dlp = proposal(bg.SamplerState(samples=x0))
    x1 = new.as_dict()["samples"][0]
    assert dlp.shape == (9,) and dlp.dtype == torch.float64 and not x1.requires_grad and not dlp.requires_grad
    assert not new.as_dict()["energies_up_to_date"]
    # the same rule by hand: the momentum at the end
    x, p = x0.detach(), m ** 0.5 * xi[0] + (h / 2) * (-x0.detach() / T)
    for k in range(L):
        x = x + (h / m) * p
        p = p + (h if k + 1 < L else h / 2) * (-x / T)
    assert torch.allclose(x, x1, rtol=0, atol=1e-14)
    k0 = (m * xi[0] ** 2).sum(-1) / (2 * m)
    assert torch.allclose(dlp, (p * p).sum(-1) / (2 * m) - k0, rtol=0, atol=1e-13)
    # the change of the Hamiltonian is small and not zero
    dh = (energy.energy(x1)[:, 0] - energy.energy(x0.detach())[:, 0]) / T + dlp
    assert 0 < float(dh.abs().max()) < 0.5
    # back: momenta -p / sqrt(m) as the normals
    with recorded_normals((-p / m ** 0.5)[None]):
        back, dlp_back = proposal(bg.SamplerState(samples=x1))
    assert torch.allclose(back.as_dict()["samples"][0], x0.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(dlp_back, -dlp, rtol=0, atol=1e-13)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_signatures_passthrough_and_import_paths():
    E = inspect.Parameter.empty
    assert _params(bg.HamiltonianProposal.__init__) == [("energy", E), ("step_size", E), ("n_leapfrog", 10), ("mass", 1.0), ("temperature", 1.0)]
    assert _params(bg.HMCStep.__init__) == [("target_energy", E), ("step_size", E), ("n_leapfrog", 10), ("mass", 1.0),
                                            ("target_temperatures", 1.0), ("n_steps", 1)]
    assert _params(bg.HamiltonianMCSampler.__init__)[:-1] == [
        ("energy", E), ("init_state", E), ("temperature", 1.), ("step_size", .01), ("n_leapfrog", 10), ("mass", 1.), ("stride", 1),
        ("n_burnin", 0), ("box_constraint", None), ("return_hook", None)]
    assert [n for n, _ in _params(sampling.pair_hmc)][:9] == ["plan", "x", "e", "e_valid", "temperature", "step_size", "n_leapfrog", "mass", "n_steps"]
    assert _params(sampling.pair_hmc)[9:] == _params(sampling.pair_mcmc)[7:17]
    for path in ("distribution.sampling", "distribution.sampling.mcmc", "distribution"):
        mod = importlib.import_module("bgflow_amd." + path)
        for name in ("HamiltonianProposal", "HMCStep", "HamiltonianMCSampler"):
            assert getattr(mod, name) is getattr(bg, name), (path, name)
    energy = bg.DoubleWellEnergy(2)
    temps = torch.linspace(1.0, 2.0, 7)
    step = bg.HMCStep(energy, 0.2, n_leapfrog=3, mass=1.5, target_temperatures=temps, n_steps=4)
    p = step.proposal
    assert isinstance(step, bg.MCMCStep) and type(p) is bg.HamiltonianProposal and p.energy is energy and step.target_energy is energy
    assert (p.step_size, p.n_leapfrog, p.mass) == (0.2, 3, 1.5) and p.temperature is temps and step.target_temperatures is temps
    assert step._n_steps == 4
    # the shortcut class: arguments passed through, the default return hook combines [n, B], a box constraint is applied
    torch.manual_seed(3)
    x0 = torch.randn(7, 2)
    sampler = bg.HamiltonianMCSampler(energy, x0, temperature=temps, step_size=0.2, n_leapfrog=3, mass=1.5, stride=2, n_burnin=5)
    out = sampler.sample(4)
    assert out.shape == (28, 2) and torch.isfinite(out).all()
    step = sampler.sampler_steps[0]
    assert type(step) is bg.HMCStep and (step.proposal.step_size, step.proposal.n_leapfrog, step.proposal.mass) == (0.2, 3, 1.5)
    assert step.target_temperatures is temps and sampler.stride == 2
    assert step.n_proposed == (5 + 4) * 2 and step.n_accepted.shape == (7,) and 0 < int(step.n_accepted.sum())
    assert bg.HamiltonianMCSampler(energy, x0, step_size=0.2, return_hook=lambda xs: xs).sample(3).shape == (3, 7, 2)
    boxed = bg.HamiltonianMCSampler(energy, x0, step_size=0.5, box_constraint=lambda t: t.clamp(-0.5, 0.5))
    assert float(boxed.sample(5).abs().max()) <= 0.5
    given = bg.SamplerState(samples=x0, energies=energy.energy(x0)[:, 0])
    assert bg.HamiltonianMCSampler(energy, given).state is given
    seen = []
    bg.HamiltonianMCSampler(energy, x0, step_size=0.2, progress_bar=lambda it: seen.append(len(it)) or it, max_iterations=3).sample(3)
    assert seen == [0, 3]


def test_guards():
    energy = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    other = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    x = torch.randn(6, 8)
    proposal = bg.HamiltonianProposal(energy, 0.1)
    with pytest.raises(ValueError, match="exactly one"):
        proposal(bg.SamplerState(samples=(x, x)))
    for bad in (dict(mass=0.0), dict(mass=-1.0), dict(mass=torch.ones(1)), dict(n_leapfrog=0), dict(n_leapfrog=2.0)):
        with pytest.raises(ValueError):
            bg.HamiltonianProposal(energy, 0.1, **bad)
    # velocities and forces of the state are ignored
    torch.manual_seed(1)
    plain, _ = proposal(bg.SamplerState(samples=x))
    torch.manual_seed(1)
    loaded, _ = proposal(bg.SamplerState(samples=x, velocities=torch.full_like(x, 9.0), forces=torch.full_like(x, -9.0)))
    assert torch.equal(plain.as_dict()["samples"][0], loaded.as_dict()["samples"][0])
    # the fused setup: None on the CPU, for f64, for a temperature mismatch, for a foreign energy, under replica exchange
    assert bg.HMCStep(energy, 0.1)._fused_setup(bg.SamplerState(samples=x)) is None
    assert bg.HMCStep(energy, 0.1)._fused_setup(bg.SamplerState(samples=x.double())) is None
    temps = torch.ones(6)
    launches = {
        "same number": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, 0.1, temperature=2.0), target_temperatures=2.0), True),
        "same tensor": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, 0.1, temperature=temps), target_temperatures=temps), True),
        "other number": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, 0.1, temperature=2.0), target_temperatures=1.0), False),
        "equal tensor, another object": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, 0.1, temperature=temps.clone()),
                                                     target_temperatures=temps), False),
        "tensor and number": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, 0.1, temperature=temps)), False),
        "foreign energy": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(other, 0.1)), False),
        "tensor step size": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, torch.tensor(0.1))), False),
        "negative step size": (bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, -0.1)), False),
    }
    for name, (step, fusable) in launches.items():
        assert (step._chain_launch() is not None) == fusable, name
        assert step._fused_setup(bg.SamplerState(samples=x)) is None, name          # no device here
    remc = bg.ReplicaExchangeMCMCStep(energy, [1.0, 2.0, 3.0], proposal=bg.HamiltonianProposal(energy, 0.1))
    assert remc._fused_setup(bg.SamplerState(samples=x)) is None
    out = remc(bg.SamplerState(samples=x)).as_dict()
    assert out["samples"][0].shape == (6, 8) and remc.n_proposed == 1 and remc.n_exchange_attempts == 0
    # the default: pair targets down to a tile of HMC_FUSED_MIN_ROWS rows (n d <= 79), no box
    from bgflow_amd.distributions import _kernel_plan
    assert sampling.HMC_FUSED_MIN_ROWS == 40 and [sampling.hmc_tile_rows(nd) for nd in (78, 79, 81)] == [40, 40, 39]
    for target, default in ((energy, True), (bg.LennardJonesPotential(78, 26, two_event_dims=False), True),
                            (bg.LennardJonesPotential(81, 27, two_event_dims=False), False),
                            (bg.LennardJonesPotential(192, 64, two_event_dims=False), False),
                            (bg.RepulsiveParticles({**bg.RepulsiveParticles.params_default, "nsolvent": 2}), False)):
        assert sampling.hmc_fused_by_default(_kernel_plan(target, 1.0)) == default
    assert bg.MCMCStep.fused is True
    # the launch cap: whole steps, at least one, fewer for longer trajectories
    caps = [sampling.hmc_max_steps_per_launch(L) for L in (1, 5, 10, 1000)]
    assert caps == sorted(caps, reverse=True) and caps[-1] == 1 and caps[0] <= sampling.MCMC_MAX_STEPS_PER_LAUNCH
    assert bg.HMCStep(energy, 0.1, n_leapfrog=5)._launch_cap() == caps[1]
    assert bg.MCMCStep(energy)._launch_cap() == sampling.MCMC_MAX_STEPS_PER_LAUNCH


def test_c_abi_and_argument_checks(hip_lib):
    """the header-derived signatures of both entries, and the argument checks, which return before any device work"""
    sigs = abi_signatures()
    i32, i64, u32, u64, f64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p
    tail = [p, i32, f64, p, f64, i32, f64, i32, p, p, u64, u32, i64, p, p, i32, p, i32, p]
    want = {"bgk_pair_hmc": [p, i64, i32, i32, i32, f64, f64, f64, f64, f64] + tail, "bgk_box_hmc": [p, i64, i32, i32, p, i32] + tail}
    for name, args in want.items():
        assert name in abi_symbols() and sigs[name] == (ctypes.c_int, args)
        assert list(getattr(hip_lib, name).argtypes) == args
        # the arguments of the Metropolis entry with noise_std replaced by step_size, n_leapfrog, mass
        plain = sigs[name.replace("hmc", "mcmc")][1]
        k = len(args) - len(tail) + 4
        assert args[:k] + [f64] + args[k + 3:] == plain and args[k:k + 3] == [f64, i32, f64]
    assert [sampling.hmc_tile_rows(nd) for nd in (192, 39, 8, 76, 128)] == [16, 64, 64, 41, 24]
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def pair(batch=0, n=13, d=3, h=0.1, L=5, m=1.0, noise=None, unif=None, temp=1.0):
        return hip_lib.bgk_pair_hmc(fake, batch, n, d, 0, 1.0, 1.0, 0.0, 0.0, 0.0, fake, 0, temp, None, h, L, m, 2, noise, unif, 1, 0, 0,
                                    None, None, 0, None, 0, None)

    prm = (ctypes.c_float * 12)(0.7, 1.21, 0.9, 0.81, 150.0, -1.0, 25.0, 10.0, 1.5, 20.0, 3.0, 100.0)

    def box(batch=0, n=38, h=0.1, L=5, m=1.0, noise=None, unif=None, kind=3):
        return hip_lib.bgk_box_hmc(fake, batch, n, kind, prm, 12, fake, 0, 1.0, None, h, L, m, 2, noise, unif, 1, 0, 0,
                                   None, None, 0, None, 0, None)

    for entry in (pair, box):
        assert entry() == 0                                                        # an empty batch: nothing to do
        for bad in (dict(h=0.0), dict(h=-0.1), dict(h=float("nan")), dict(m=0.0), dict(m=-2.0), dict(L=0), dict(L=-3),
                    dict(noise=fake), dict(unif=fake), dict(batch=-1)):
            assert entry(**bad) == -1, bad
        assert entry(noise=fake, unif=fake) == 0
        assert entry(n=65) == -2 and b"envelope" in hip_lib.bgk_last_error()
        assert entry(n=1) == -2 and b"envelope" in hip_lib.bgk_last_error()
    assert pair(d=4) == -2 and b"envelope" in hip_lib.bgk_last_error()
    assert pair(temp=0.0) == -1 and box(kind=1) == -1
    for n in range(2, 65):
        for d in (1, 2, 3):
            assert pair(n=n, d=d) == 0
