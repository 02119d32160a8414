"""Shared by test_host_stochastic_backward.py and test_gpu_stochastic_backward.py: the cases of tests/golden/stochastic_grad.npz (written
by tests/golden/make_stochastic_grad_goldens.py) rebuilt with this package's classes on the random numbers of stochastic_common.py."""
import functools

import numpy as np
import torch

import bgflow_amd as bg
from oracle import philox

from stochastic_common import B, KINDS, SHAPES, make, normals, start_velocities

HVP_CASES = [(k, n, d) for k in KINDS for n, d in SHAPES]
# (layer, kind, n, d, nsteps, tag)
LAYER_CASES = [(layer, k, n, d, 3, "") for layer in ("brownian", "langevin") for k in KINDS for n, d in SHAPES] \
    + [(layer, k, 13, 3, 12, "") for layer in ("brownian", "langevin") for k in KINDS] + [("langevin", "lj", 13, 3, 12, "_p")]


def grad_key(layer, kind, n, d, nsteps, tag=""):
    return f"grad_{layer}_{kind}_{n}_{d}_{nsteps}{tag}_"


@functools.lru_cache(maxsize=None)
def _vectors(seed, offset, nd):
    return philox.sample_field(seed, offset, 0, B, nd, 1).astype(np.float32)


def vectors(GG, n, d):
    """the vectors u [B, n d] of the fixture's Hessian products, checked against the sum it recorded"""
    u = _vectors(int(GG["seed"]), int(GG["u_offset"]), n * d)
    assert abs(u.astype(np.float64).sum() - float(GG[f"u_sum_{n}_{d}"])) <= 1e-9 * u.size
    return u


def build_grad(GG, G, P, layer, kind, n, d, nsteps, tag="", device="cpu", feed=True):
    """(flow with ``fused_backward`` set and the case's numbers fed, inputs in f32 on ``device`` that require grad) of a gradient case"""
    key = grad_key(layer, kind, n, d, nsteps, tag)
    energy = make(P, kind, n, d).to(device)
    h = float(GG[key + "stepsize"])
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=device).reshape(B, -1).requires_grad_(True)
    if layer == "brownian":
        flow = bg.BrownianFlow(energy, nsteps=nsteps, stepsize=h)
        fed, xs = [normals(G, 0, n, d, nsteps)], (x0,)
    else:
        mass, gamma, kT = (float(v) for v in GG[key + "params"])
        flow = bg.LangevinFlow(energy, nsteps=nsteps, stepsize=h, mass=mass, gamma=gamma, kT=kT)
        fed = [normals(G, 0, n, d, nsteps), normals(G, 1, n, d, nsteps)]
        xs = (x0, torch.tensor(start_velocities(G, n, d), device=device).requires_grad_(True))
    flow.fused_backward = True
    if feed:
        flow.feed_noise(*[torch.tensor(f, device=device) for f in fed])
    return flow, xs


def within(got, want, err32):
    """max of |got - want| / (4 err32 + 1e-6 (1 + |want|)), and max |got - want| / err32 (the rule of test_gpu_stochastic.py)"""
    diff = np.abs(got.astype(np.float64) - want)
    return float((diff / (4 * err32 + 1e-6 * (1 + np.abs(want)))).max()), float(diff.max() / max(err32, 1e-300))


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def philox_normals(seed, offset, n_steps, batch, nd, dev, row0=0):
    """what bgk_philox_fields writes for (seed, offset + s), fields [normal nd, normal nd]: w1, w2 [n_steps, batch, nd]"""
    from bgflow_amd.distributions import philox_sample
    w1, w2 = [], []
    for s in range(n_steps):
        (a, b), _ = philox_sample([(1, nd, None, None, 1.0, 0.0), (1, nd, None, None, 1.0, 0.0)], batch, dev, seed, offset + s, row0=row0)
        w1.append(a)
        w2.append(b)
    return torch.stack(w1), torch.stack(w2)


def flow_seed(flow):
    """(key, position) of the layer's Philox stream"""
    from bgflow_amd import dp
    st = flow._philox_ids()
    return (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1), st[1]
