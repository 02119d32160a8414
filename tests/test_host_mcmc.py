"""Host: bgflow_amd.sampling -- the general path (torch ops over ``energy.energy``) against the reference's recorded f64 chains
(tests/golden/mcmc.npz, written by tests/golden/make_mcmc_goldens.py), the state bookkeeping, the driver's options, the signatures."""
import importlib
import inspect
import json
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling

from mcmc_common import B, CASES, N_FRAMES, N_STEPS, STRIDE, case_numbers, case_temperatures, make, run_general


@pytest.mark.parametrize("kind,n,d", CASES)
def test_general_path_reproduces_the_reference_chains(golden, kind, n, d):
    """f64 on the CPU, the fixture's random numbers: the same decisions, and states to 1e-12, on EVERY chain"""
    G, P = golden("mcmc"), golden("particles")
    key = f"{kind}_{n}_{d}_"
    noise, unif = case_numbers(G, n, d)
    energy = make(P, kind, n, d)                   # (not .double(): the fixture's script leaves the module's buffers as constructed)
    x0 = torch.tensor(P[f"x_{n}_{d}"]).reshape(B, -1).double()
    frames, sampler, step = run_general(energy, x0, torch.from_numpy(noise), torch.from_numpy(unif), float(G[key + "std"]),
                                        case_temperatures(G, key, torch.float64, "cpu"))
    assert frames.shape == (N_FRAMES, B, n * d) and frames.dtype == torch.float64
    assert np.array_equal(step.n_accepted.numpy(), G[key + "acc"]) and step.n_proposed == N_STEPS
    state = sampler.state.as_dict()
    assert state["energies_up_to_date"]
    x = state["samples"][0].numpy()
    assert np.abs(x[G[key + "rows"]] - G[key + "x64"]).max() <= 1e-12
    e64 = G[key + "e64"]
    assert np.max(np.abs(state["energies"].numpy() - e64) / (1 + np.abs(e64))) <= 1e-12
    assert np.abs(frames[:, :8].numpy() - G[key + "frames64"]).max() <= 1e-12
    assert np.array_equal(frames[-1].numpy(), x)


def test_metropolis_accept_hand_cases():
    cur = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, float("inf")], dtype=torch.float64)
    new = torch.tensor([0.5, 2.0, 2.0, float("inf"), float("nan"), 3.0], dtype=torch.float64)
    r = torch.tensor([0.999, 0.3, 0.4, 1e-300, 1e-300, 0.999], dtype=torch.float64)
    original = torch.rand_like
    torch.rand_like = lambda like: r.to(like.dtype)
    try:
        acc = bg.metropolis_accept(cur, new, 0.0)
        shifted = bg.metropolis_accept(cur, new, torch.tensor([0.0, -1.0, 0.5, 0.0, 0.0, 0.0], dtype=torch.float64))
    finally:
        torch.rand_like = original
    # downhill always; uphill by 1: exp(-1) = 0.3679 against r = 0.3 (yes) and 0.4 (no); +inf and NaN proposals never; out of +inf always
    assert acc.tolist() == [True, True, False, False, False, True]
    # an asymmetric proposal shifts the log ratio: -1 - (-1) = 0 -> accepted; -1 - 0.5 against log 0.4 = -0.92 -> rejected
    assert shifted.tolist() == [True, True, False, False, False, True]
    assert acc.dtype == torch.bool


def test_sampler_state_bookkeeping_and_box_mapping():
    x = torch.arange(6.0).reshape(2, 3)
    s = bg.SamplerState(samples=x)
    d = s.as_dict()
    assert isinstance(d["samples"], tuple) and d["energies"] is None and not d["energies_up_to_date"] and not d["forces_up_to_date"]
    assert d["velocities"] is None and d["forces"] is None and d["box_vectors"] is None
    s2 = s.replace(energies=torch.zeros(2))
    assert s2.as_dict()["energies_up_to_date"] and not s2.as_dict()["forces_up_to_date"] and s2.energies_up_to_date
    s3 = s2.replace(forces=torch.ones(2, 3))
    assert s3.as_dict()["energies_up_to_date"] and s3.as_dict()["forces_up_to_date"] and isinstance(s3.as_dict()["forces"], tuple)
    s4 = s3.replace(samples=(x + 1,))
    assert not s4.as_dict()["energies_up_to_date"] and not s4.as_dict()["forces_up_to_date"]
    s5 = s3.replace(samples=(x + 1,), energies=torch.ones(2))
    assert s5.as_dict()["energies_up_to_date"] and not s5.as_dict()["forces_up_to_date"]
    with pytest.raises(AttributeError, match="no attribute 'nonsense'"):
        s.nonsense
    # evaluate_energy_force: evaluates what is stale, keeps what is up to date
    energy = bg.DoubleWellEnergy(3)
    s6 = s.evaluate_energy_force(energy, evaluate_forces=False)
    assert torch.equal(s6.as_dict()["energies"], energy.energy(x)[:, 0]) and s6.as_dict()["energies_up_to_date"]
    marked = s6.replace(energies=torch.full((2,), 7.0))
    assert torch.equal(marked.evaluate_energy_force(energy, evaluate_forces=False).as_dict()["energies"], torch.full((2,), 7.0))
    # the samples hook runs whenever samples are set
    hooked = bg.SamplerState(samples=x, set_samples_hook=lambda xs: [t.clamp(max=2.0) for t in xs])
    assert float(hooked.replace(samples=(x,)).as_dict()["samples"][0].max()) == 2.0
    # box vectors (upper triangular, columns = lattice vectors): samples are mapped to the primary cell on every replace
    cell = torch.tensor([[2.0, 1.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 4.0]])
    pts = torch.tensor([[2.5, 0.5, -1.0], [4.5, 3.5, 9.0]])
    boxed = bg.SamplerState(samples=pts, box_vectors=cell).replace(samples=(pts,))
    got = boxed.as_dict()["samples"][0]
    frac = torch.linalg.solve(cell, got.T).T
    assert (frac >= 0).all() and (frac < 1).all()
    shift = torch.linalg.solve(cell, (pts - got).T).T
    assert torch.allclose(shift, shift.round(), atol=1e-6)
    assert torch.allclose(got, torch.tensor([[0.5, 0.5, 3.0], [1.5, 0.5, 1.0]]))


class _AddOne(bg.SamplerStep):
    def _step(self, state):
        return state.replace(samples=tuple(x + 1 for x in state.as_dict()["samples"]))


def test_iterative_sampler_options():
    x = torch.zeros(5, 2)
    sampler = bg.IterativeSampler(x, [_AddOne(n_steps=2)], stride=3, n_burnin=4, max_iterations=9)
    assert isinstance(sampler.state, bg.SamplerState) and sampler.i == 4
    assert float(sampler.state.as_dict()["samples"][0][0, 0]) == 4 * 6           # burn-in iterations count, 3 x 2 steps each
    out = sampler.sample(2)
    assert out.shape == (2, 5, 2) and out[:, 0, 0].tolist() == [30.0, 36.0]
    assert iter(sampler) is sampler
    state = next(sampler)
    assert float(state.as_dict()["samples"][0][0, 0]) == 42.0 and sampler.i == 7
    assert len([s for s in sampler]) == 2 and sampler.i == 9                     # the iterations left below max_iterations
    with pytest.raises(StopIteration):
        next(sampler)
    with pytest.raises(StopIteration):
        sampler.sample(1)
    # two events, a progress bar, an extract hook, a return hook
    seen = []
    two = bg.IterativeSampler(bg.SamplerState(samples=(torch.zeros(4, 2), torch.zeros(4, 3))), [_AddOne()],
                              progress_bar=lambda it: seen.append(len(it)) or it,
                              extract_sample_hook=lambda st: [t * 2 for t in st.as_dict()["samples"]],
                              return_hook=lambda xs: [t[:, :1] for t in xs])
    a, b = two.sample(3)
    assert a.shape == (3, 1, 2) and b.shape == (3, 1, 3) and a[:, 0, 0].tolist() == [2.0, 4.0, 6.0] and seen == [0, 3]
    with pytest.raises(TypeError):
        bg.IterativeSampler(x, [_AddOne()], no_such_option=1)
    assert isinstance(sampler, torch.utils.data.Dataset) and isinstance(sampler, bg.Sampler)


def test_gaussian_mcmc_sampler():
    torch.manual_seed(3)
    energy = bg.DoubleWellEnergy(2)
    x0 = torch.randn(7, 2)
    sampler = bg.GaussianMCMCSampler(energy, x0, temperature=torch.linspace(1.0, 2.0, 7), noise_std=0.3, stride=2, n_burnin=5)
    out = sampler.sample(4)
    assert out.shape == (28, 2) and torch.isfinite(out).all()               # the default return hook combines [n, B]
    step = sampler.sampler_steps[0]
    assert isinstance(step, bg.MCMCStep) and isinstance(step.proposal, bg.GaussianProposal) and step.proposal._noise_std == 0.3
    assert step.n_proposed == (5 + 4) * 2 and step.n_accepted.shape == (7,) and int(step.n_accepted.max()) <= step.n_proposed
    assert int(step.n_accepted.sum()) > 0
    kept = bg.GaussianMCMCSampler(energy, x0, return_hook=lambda xs: xs).sample(3)
    assert kept.shape == (3, 7, 2)
    boxed = bg.GaussianMCMCSampler(energy, x0, noise_std=1.0, box_constraint=lambda t: t.clamp(-0.5, 0.5))
    assert float(boxed.sample(5).abs().max()) <= 0.5
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        old = bg.GaussianMCMCSampler(energy, x0, n_stride=4)
    assert old.stride == 4 and any(issubclass(i.category, DeprecationWarning) and "n_stride" in str(i.message) for i in w)
    given = bg.SamplerState(samples=x0, energies=energy.energy(x0)[:, 0])
    assert bg.GaussianMCMCSampler(energy, given).state is given


class _Scale(bg.Flow):
    """x = 2 z, an identity-like project flow with a constant log-determinant"""

    def _forward(self, z, **kwargs):
        return 2 * z, torch.full((z.shape[0], 1), z.shape[1] * np.log(2.0), dtype=z.dtype)

    def _inverse(self, x, **kwargs):
        return x / 2, torch.full((x.shape[0], 1), -x.shape[1] * np.log(2.0), dtype=x.dtype)


def test_latent_proposal():
    torch.manual_seed(0)
    x = torch.randn(6, 3, dtype=torch.float64)
    proposal = bg.LatentProposal(_Scale(), base_proposal=bg.GaussianProposal(noise_std=0.5))
    torch.manual_seed(1)
    new, dlp = proposal(bg.SamplerState(samples=x))
    torch.manual_seed(1)
    eps = torch.randn_like(x)
    assert torch.allclose(new.as_dict()["samples"][0], 2 * (x / 2 + 0.5 * eps), atol=1e-14)
    assert dlp.shape == (6,) and torch.allclose(dlp, torch.zeros(6, dtype=torch.float64), atol=1e-14)     # the two log-determinants cancel
    assert not new.as_dict()["energies_up_to_date"]
    assert isinstance(bg.LatentProposal(_Scale()).base_proposal, bg.GaussianProposal)
    # ... and inside a step: a chain on a normal target stays finite and moves
    step = bg.MCMCStep(bg.NormalDistribution(3), proposal=proposal, n_steps=20)
    out = step(bg.SamplerState(samples=x.float())).as_dict()
    assert torch.isfinite(out["samples"][0]).all() and out["energies_up_to_date"] and int(step.n_accepted.sum()) > 0


def _signature(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        if p.name == "self":
            continue
        d = p.default
        if d is inspect.Parameter.empty:
            d = "<required>" if p.kind is p.POSITIONAL_OR_KEYWORD else f"<{p.kind.name}>"
        elif isinstance(d, torch.nn.Module):
            d = f"{type(d).__name__}({getattr(d, '_noise_std', '')})"
        elif callable(d):
            d = f"<callable {d.__name__}>"
        elif isinstance(d, dict):
            d = dict(d)
        out.append([p.name, d])
    return out


def test_signatures_equal_the_reference(golden):
    import dataclasses
    meta = json.loads(str(golden("mcmc")["meta"]))
    ours = {
        "SamplerState": bg.SamplerState.__init__, "SamplerStep": bg.SamplerStep.__init__, "IterativeSampler": bg.IterativeSampler.__init__,
        "GaussianProposal": bg.GaussianProposal.__init__, "LatentProposal": bg.LatentProposal.__init__, "MCMCStep": bg.MCMCStep.__init__,
        "GaussianMCMCSampler": bg.GaussianMCMCSampler.__init__, "metropolis_accept": bg.metropolis_accept,
        "evaluate_energy_force": bg.SamplerState.evaluate_energy_force,
    }
    for name, fn in ours.items():
        assert _signature(fn) == meta[name], name
    fields = [[f.name, f.default] for f in dataclasses.fields(sampling._SamplerStateData) if f.name != "samples"]
    assert fields == meta["state_fields"]
    assert bg.MCMCStep.fused is True and sampling.MCMC_MAX_STEPS_PER_LAUNCH >= 1


@pytest.mark.parametrize("path,names", [
    ("distribution.sampling", ["IterativeSampler", "SamplerState", "SamplerStep", "MCMCStep", "GaussianMCMCSampler", "GaussianProposal",
                               "LatentProposal", "metropolis_accept", "Sampler"]),
    ("distribution.sampling.iterative", ["IterativeSampler", "SamplerState", "SamplerStep"]),
    ("distribution.sampling.mcmc", ["MCMCStep", "GaussianMCMCSampler", "GaussianProposal", "LatentProposal", "metropolis_accept"]),
    ("distribution", ["IterativeSampler", "MCMCStep"]),
])
def test_dotted_import_paths(path, names):
    mod = importlib.import_module("bgflow_amd." + path)
    for n in names:
        assert getattr(mod, n) is getattr(bg, n), (path, n)


def test_launch_plan_covers_every_step_once():
    """the split of a fused run into launches: every unit recorded once, no launch above the cap"""
    for unit, count, cap in ((3, 16, 256), (3, 16, 5), (3, 16, 3), (7, 4, 5), (1, 9, 4), (600, 2, 256), (5, 1, 5)):
        plan = sampling._launch_plan(unit, count, cap)
        assert sum(s for s, _, _ in plan) == unit * count and sum(f for _, _, f in plan) == count
        assert all(1 <= s <= max(cap, 1) for s, _, _ in plan)
        t, recorded = 0, []
        for steps, every, frames in plan:
            assert steps == every * frames if every else frames == 0
            recorded += [t + (f + 1) * every for f in range(frames)]
            t += steps
        assert recorded == [unit * (k + 1) for k in range(count)]


def test_general_path_without_a_device_is_the_default():
    """CPU tensors never reach the kernel: a particle target on the CPU runs the general path, whatever ``fused`` says"""
    torch.manual_seed(0)
    energy = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    step = bg.MCMCStep(energy, proposal=bg.GaussianProposal(0.3), n_steps=5)
    assert step._fused_setup(bg.SamplerState(samples=torch.randn(9, 8))) is None
    out = step(bg.SamplerState(samples=torch.randn(9, 8))).as_dict()
    assert out["samples"][0].shape == (9, 8) and step.n_proposed == 5
    assert torch.equal(out["energies"], energy.energy(out["samples"][0])[:, 0])
