"""Shared by test_host_kernel_dynamics.py and test_gpu_kernel_dynamics.py: the cases of tests/golden/kernel_dynamics.npz (written by
tests/golden/make_kernel_dynamics_goldens.py) rebuilt with this package's classes."""
import json

import numpy as np
import torch

import bgflow_amd as bg

SHAPES = [(2, 1), (4, 2), (13, 3), (64, 3)]
SETS = ["ref", "edge"]
PARAMS = ("_weights", "_bias", "_importance", "_neg_log_gammas_time")
CONFIGS = [(m, nt, dr) for m in ("rk4", "euler") for nt in (1, 4) for dr in ("f", "i")]


def kernel_set(name, dtype=torch.float32):
    if name == "ref":
        return dict(mus=torch.linspace(0, 8, 10, dtype=dtype), gammas=torch.full((10,), 0.3, dtype=dtype),
                    mus_time=torch.linspace(0, 1, 5, dtype=dtype), gammas_time=torch.full((5,), 0.3, dtype=dtype))
    return dict(mus=torch.linspace(0, 8, 64, dtype=dtype), gammas=torch.full((64,), 0.3, dtype=dtype),
                mus_time=torch.linspace(0, 1, 16, dtype=dtype), gammas_time=torch.full((16,), 0.1, dtype=dtype))


def make_dynamics(G, name, n, d, dtype=torch.float32, prefix=None):
    """the KernelDynamics of a golden case with its recorded parameter values"""
    dyn = bg.KernelDynamics(n, d, optimize_t_gammas=True, **kernel_set(name, dtype)).to(dtype)
    prefix = prefix or f"{name}_{n}_{d}_"
    with torch.no_grad():
        for p in ("_weights", "_bias", "_importance"):
            getattr(dyn, p).copy_(torch.tensor(G[f"{prefix}p{p}"], dtype=dtype))
    return dyn


_SCALARS = {}


def scalars(G):
    """the fixture's recorded numbers (reference f32 errors ``err_*32``, round-trip errors ``rt64_*``) by name"""
    if id(G) not in _SCALARS:
        _SCALARS[id(G)] = json.loads(str(G["scalars"]))
    return _SCALARS[id(G)]


def bound(G, key):
    """4 x the reference's own f32 error + 1e-6"""
    return 4 * scalars(G)[key] + 1e-6


def cotangents(B, nd):
    """a [B, nd], b [B] of the scalar sum(forces a) + sum(div b) whose gradients the fixture records"""
    i = np.arange(B * nd, dtype=np.float64).reshape(B, nd)
    return torch.tensor(np.cos(0.7 * i + 0.3)), torch.tensor(np.sin(1.3 * np.arange(B, dtype=np.float64) + 0.1))


def evaluate(dyn, x, t):
    """forces, divergence and the gradients of sum(forces a) + sum(div b) w.r.t. x and the parameters, as numpy arrays"""
    x = x.clone().requires_grad_(True)
    ga, gb = cotangents(x.shape[0], x.shape[1])
    forces, neg_div = dyn(t, x)
    assert forces.shape == x.shape and neg_div.shape == (x.shape[0], 1)
    div = -neg_div.reshape(-1)
    loss = (forces * ga.to(x)).sum() + (div * gb.to(x)).sum()
    got = torch.autograd.grad(loss, [x] + [getattr(dyn, p) for p in PARAMS])
    res = {"f": forces, "div": div, "gx": got[0]}
    res.update({"g" + p: g for p, g in zip(PARAMS, got[1:])})
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def flow_of(dyn, method, n_steps, t_max=1.0):
    return bg.DiffEqFlow(dyn, use_checkpoints=True, t_max=t_max, Nt=n_steps, method={"rk4": "RK4", "euler": "Euler"}[method])


def err_s(v, v64):
    """per-sample scalars: max_b |v - v64| / (1 + |v64|)"""
    v, v64 = np.asarray(v, dtype=np.float64).reshape(-1), np.asarray(v64).reshape(-1)
    return float(np.max(np.abs(v - v64) / (1.0 + np.abs(v64))))


def err_a(v, v64):
    """arrays: max |v - v64| / (1 + max |v64|)"""
    v, v64 = np.asarray(v, dtype=np.float64), np.asarray(v64)
    return float(np.max(np.abs(v - v64)) / (1.0 + np.max(np.abs(v64))))
