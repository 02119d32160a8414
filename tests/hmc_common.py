"""Shared by test_host_hmc.py and test_gpu_hmc.py: the cases of tests/golden/hmc.npz (written by tests/golden/make_hmc_goldens.py) rebuilt
with this package's classes, their random numbers regenerated from oracle/philox.py, and the general path driven on recorded numbers the
way the fixture's script drives the reference: ``torch.randn_like`` returns the recorded normals of the momenta, ``torch.rand_like`` the
recorded uniforms of the acceptance draw."""
import contextlib

import numpy as np
import torch

import bgflow_amd as bg

import box_common
import mcmc_common
from mcmc_common import recorded_uniforms

B = 150
N_FRAMES, STRIDE = 6, 2
N_STEPS = N_FRAMES * STRIDE
PAIR_CASES = [(k, n, d) for k in mcmc_common.KINDS for n, d in mcmc_common.SHAPES]
BOX_CASES = [(k, ns) for k in box_common.KINDS for ns in (2, 62)]
CASES = PAIR_CASES + BOX_CASES
IDS = ["_".join(str(v) for v in c) for c in CASES]


def key_of(case):
    return "_".join(str(v) for v in case) + "_"


def is_box(case):
    return case[0] in box_common.KINDS


def make(golden, case, two_event_dims=False):
    """(the target of a case, its start state [B, n d] as an f32 numpy array)"""
    if is_box(case):
        G = golden("box")
        return box_common.make(G, *case), np.ascontiguousarray(G[f"x_{case[1]}"]).reshape(B, -1)
    kind, n, d = case
    P = golden("particles")
    return mcmc_common.make(P, kind, n, d, two_event_dims), np.ascontiguousarray(P[f"x_{n}_{d}"]).reshape(B, -1)


def case_numbers(golden, case, nd):
    """the case's random numbers (xi [12, B, n d], r [12, B]), checked against the sums the fixture recorded"""
    G = golden("hmc")
    seed, tag = (int(G["seed_box"]), f"box_{nd}") if is_box(case) else (int(G["seed"]), f"{nd}")
    noise, unif = mcmc_common.random_numbers(seed, nd, N_STEPS, B)
    assert abs(noise.astype(np.float64).sum() - float(G[f"noise_sum_{tag}"])) <= 1e-9 * noise.size
    assert float(np.abs(noise).max()) == float(G[f"noise_absmax_{tag}"])
    assert abs(unif.astype(np.float64).sum() - float(G[f"unif_sum_{tag}"])) <= 1e-12 * unif.size
    assert float(unif.max()) == float(G[f"unif_absmax_{tag}"])
    return noise, unif


def case_settings(G, key, dtype, device):
    """(step_size, n_leapfrog, mass, temperature) of a case"""
    return (float(G[key + "step_size"]), int(G[key + "n_leapfrog"]), float(G[key + "mass"]),
            mcmc_common.case_temperatures(G, key, dtype, device))


@contextlib.contextmanager
def recorded_normals(noise):
    """``torch.randn_like`` returns the rows of ``noise`` in turn (the momenta of ``HamiltonianProposal``)"""
    step = [0]

    def draw(like):
        xi = noise[step[0]].to(like.dtype).reshape(like.shape)
        step[0] += 1
        return xi

    original = torch.randn_like
    torch.randn_like = draw
    try:
        yield step
    finally:
        torch.randn_like = original


def run_general(energy, x0, noise, unif, settings, n_frames=N_FRAMES, stride=STRIDE, step=None):
    """the general path on recorded numbers: (frames [n_frames, B, ...], sampler, step); x0 / noise / unif: tensors of one device;
    the step is an ``HMCStep`` of the settings (step_size, n_leapfrog, mass, temperature), or ``step``"""
    if step is None:
        h, L, m, temps = settings
        step = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, target_temperatures=temps)
    with recorded_normals(noise) as drawn, recorded_uniforms(unif) as count:
        sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=stride)
        frames = sampler.sample(n_frames)
    assert count[0] == n_frames * stride and drawn[0] == n_frames * stride
    return frames, sampler, step
