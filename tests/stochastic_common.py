"""Shared by test_host_stochastic.py and test_gpu_stochastic.py: the cases of tests/golden/stochastic.npz (written by
tests/golden/make_stochastic_goldens.py) rebuilt with this package's classes, their random numbers regenerated from oracle/philox.py
and checked against the sums the fixture recorded."""
import functools

import numpy as np
import torch

import bgflow_amd as bg
from oracle import philox

from mcmc_common import make  # noqa: F401  (the targets with the parameters of particles.npz)

B = 150
SHAPES = [(2, 1), (4, 2), (13, 3), (64, 3)]
KINDS = ["lj", "mdw", "mfn"]
NSTEPS = (1, 12)
MC_STEPS = 48
GRAD_STEPS = 3
# (layer, kind, n, d, nsteps, tag)
INTEGRATOR_CASES = [(layer, k, n, d, s, "") for layer in ("brownian", "langevin") for k in KINDS for n, d in SHAPES for s in NSTEPS] \
    + [("langevin", k, 13, 3, 12, "_p") for k in KINDS]
METROPOLIS_CASES = [(k, n, d) for k in KINDS for n, d in SHAPES]
GRAD_CASES = [(layer, k) for layer in ("brownian", "langevin") for k in ("lj", "mfn")]


def case_key(layer, kind, n, d, nsteps, tag=""):
    return f"{layer}_{kind}_{n}_{d}_{nsteps}{tag}_"


@functools.lru_cache(maxsize=None)
def _normals(seed, field, nd, n_steps):
    return np.stack([philox.sample_field(seed, s, field, B, nd, 1).astype(np.float32) for s in range(n_steps)])


@functools.lru_cache(maxsize=None)
def _uniforms(seed, n_steps):
    return np.stack([philox.sample_field(seed, s, 1, B, 1, 0)[:, 0] for s in range(n_steps)])


def normals(G, field, n, d, n_steps):
    """the first ``n_steps`` rows [n_steps, B, n d] of the fixture's normals of ``field``, checked against its recorded sums"""
    full = _normals(int(G["seed"]), field, n * d, MC_STEPS if field == 0 else max(NSTEPS))
    assert abs(full.astype(np.float64).sum() - float(G[f"normal_sum_{field}_{n}_{d}"])) <= 1e-9 * full.size
    assert float(np.abs(full).max()) == float(G[f"normal_absmax_{field}_{n}_{d}"])
    return full[:n_steps]


def uniforms(G):
    unif = _uniforms(int(G["seed"]), MC_STEPS)
    assert abs(unif.astype(np.float64).sum() - float(G["unif_sum"])) <= 1e-12 * unif.size and float(unif.max()) == float(G["unif_absmax"])
    return unif


def start_velocities(G, n, d):
    v0 = philox.sample_field(int(G["seed"]), int(G["v0_offset"]), 0, B, n * d, 1).astype(np.float32)
    assert abs(v0.astype(np.float64).sum() - float(G[f"v0_sum_{n}_{d}"])) <= 1e-9 * v0.size
    return v0


def build(G, P, layer, kind, n, d, nsteps, tag="", device="cpu"):
    """(flow with the case's numbers fed, inputs in f32 on ``device``) of a fixture case"""
    key = case_key(layer, kind, n, d, nsteps, tag)
    energy = make(P, kind, n, d).to(device)
    h = float(G[key + "stepsize"])
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=device).reshape(B, -1)

    def dev(a):
        return torch.tensor(a, device=device)

    if layer == "brownian":
        flow = bg.BrownianFlow(energy, nsteps=nsteps, stepsize=h).feed_noise(dev(normals(G, 0, n, d, nsteps)))
        return flow, (x0,)
    if layer == "langevin":
        mass, gamma, kT = (float(v) for v in G[key + "params"])
        flow = bg.LangevinFlow(energy, nsteps=nsteps, stepsize=h, mass=mass, gamma=gamma, kT=kT)
        flow.feed_noise(dev(normals(G, 0, n, d, nsteps)), dev(normals(G, 1, n, d, nsteps)))
        return flow, (x0, dev(start_velocities(G, n, d)))
    flow = bg.MetropolisMCFlow(energy, nsteps=nsteps, stepsize=h).feed_noise(dev(normals(G, 0, n, d, nsteps)), dev(uniforms(G)[:nsteps]))
    return flow, (x0,)
