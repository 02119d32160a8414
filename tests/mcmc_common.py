"""Shared by test_host_mcmc.py and test_gpu_mcmc.py: the cases of tests/golden/mcmc.npz (written by tests/golden/make_mcmc_goldens.py)
rebuilt with this package's classes, their random numbers regenerated from oracle/philox.py, and the general path driven on recorded
numbers the way the fixture's script drives the reference."""
import contextlib
import functools

import numpy as np
import torch

import bgflow_amd as bg
from oracle import philox

B = 150
N_FRAMES, STRIDE = 16, 3
N_STEPS = N_FRAMES * STRIDE
SHAPES = [(2, 1), (4, 2), (13, 3), (64, 3)]
KINDS = ["lj", "mdw", "mfn"]
CASES = [(k, n, d) for k in KINDS for n, d in SHAPES]


def make(P, kind, n, d, two_event_dims=False):
    """the target of a case with the parameters of particles.npz"""
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        return bg.LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=two_event_dims)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in P["mdw_params"])
        return bg.MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=two_event_dims)
    return bg.MeanFreeNormalDistribution(n * d, n, std=float(P["mfn_std"]), two_event_dims=two_event_dims)


@functools.lru_cache(maxsize=None)
def random_numbers(seed, nd, n_steps=N_STEPS, batch=B):
    """(noise [n_steps, batch, nd], uniforms [n_steps, batch]) in f32, as the fixture's script draws them"""
    noise = np.stack([philox.sample_field(seed, s, 0, batch, nd, 1).astype(np.float32) for s in range(n_steps)])
    unif = np.stack([philox.sample_field(seed, s, 1, batch, 1, 0)[:, 0] for s in range(n_steps)])
    return noise, unif


def case_numbers(G, n, d):
    """the case's random numbers, checked against the sums the fixture recorded"""
    noise, unif = random_numbers(int(G["seed"]), n * d)
    assert abs(noise.astype(np.float64).sum() - float(G[f"noise_sum_{n}_{d}"])) <= 1e-9 * noise.size
    assert float(np.abs(noise).max()) == float(G[f"noise_absmax_{n}_{d}"])
    assert abs(unif.astype(np.float64).sum() - float(G["unif_sum"])) <= 1e-12 * unif.size and float(unif.max()) == float(G["unif_absmax"])
    return noise, unif


def case_temperatures(G, key, dtype, device):
    t = G[key + "temps"]
    return float(t) if t.ndim == 0 else torch.tensor(t, dtype=dtype, device=device)


class RecordedProposal(torch.nn.Module):
    """x + noise_std * (the recorded noise of the step), a symmetric proposal"""

    def __init__(self, noise, noise_std):
        super().__init__()
        self.noise, self.noise_std, self.step = noise, noise_std, 0

    def forward(self, state):
        eps = self.noise[self.step]
        self.step += 1
        return state.replace(samples=tuple(x + eps.reshape(x.shape).to(x.dtype) * self.noise_std for x in state.as_dict()["samples"])), 0.0


@contextlib.contextmanager
def recorded_uniforms(uniforms):
    """``torch.rand_like`` returns the rows of ``uniforms`` in turn (the acceptance draw of ``metropolis_accept``)"""
    step = [0]

    def draw(like):
        r = uniforms[step[0]].to(like.dtype).reshape(like.shape)
        step[0] += 1
        return r

    original = torch.rand_like
    torch.rand_like = draw
    try:
        yield step
    finally:
        torch.rand_like = original


def run_general(energy, x0, noise, unif, std, temps, n_frames=N_FRAMES, stride=STRIDE):
    """the general path on recorded numbers: (frames [n_frames, B, ...], sampler, step); x0 / noise / unif: tensors of one device"""
    step = bg.MCMCStep(energy, proposal=RecordedProposal(noise, std), target_temperatures=temps)
    with recorded_uniforms(unif) as count:
        sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=stride)
        frames = sampler.sample(n_frames)
    assert count[0] == n_frames * stride
    return frames, sampler, step
