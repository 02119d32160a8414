#!/usr/bin/env python
"""Generate tests/golden/kernel_dynamics.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_kernel_dynamics_goldens.py

What runs: the UNMODIFIED reference classes ``KernelDynamics`` (nn/flow/dynamics/kernel_dynamic.py), ``DensityDynamics`` (dynamics/density.py)
and ``InversedDynamics`` (dynamics/inversed.py) with the two import shims of make_particle_goldens.py.  The fixture holds DATA only.

Positions: the arrays ``x_{n}_{d}`` of tests/golden/particles.npz (B = 150) for (n, d) in {(2,1), (4,2), (13,3), (64,3)} -- a single pair,
both parities of n d, a partial last tile, the widest row.  Kernel sets: ``ref`` (the reference test's: mus = linspace(0, 8, 10), gammas = 0.3,
mus_time = linspace(0, 1, 5), gammas_time = 0.3) and ``edge`` (the kernel envelope: K = 64 over [0, 8], gammas = 0.3, O = 16 over [0, 1],
gammas_time = 0.1).  Parameters are seeded and all non-zero (``{set}_{n}_{d}_p_{name}``).  Times t in {0, 0.37, 1} (index 0, 1, 2).

Per case ``{set}_{n}_{d}_`` (f64 = the reference on x.double() with f64 parameters, f32 = the same in f32):
  f64_t{i}      forces at TIMES[i]                              div64 [3, B]   the divergence (= -forward()[1]) at the three times
  gx64          f64 autograd of sum(forces a) + sum(div b) w.r.t. x at t = 0.37, a[b, c] = cos(0.7 (b n d + c) + 0.3), b[b] = sin(1.3 b + 0.1)
  g64_{p}       ... w.r.t. the parameter p (_weights, _bias, _importance, _neg_log_gammas_time), stacked over the three times
  y64_{m}{Nt}{dir}, dlogp64 [8, B] (in the order of CONFIGS)   this script's integration (h = t_max / Nt, t_max = 1; classical RK4 with stages at t, t + h/2,
                t + h/2, t + h, or explicit Euler; positions and log-density change with the same tableau) of the reference's
                DensityDynamics (dir f) or DensityDynamics(InversedDynamics) (dir i), m in {rk4, euler}, Nt in {1, 4}
  rt64_{m}{Nt}  max |inverse(forward(x)) - x| of that f64 integration: the round-trip error of the discretisation itself
  err_*32       (in ``scalars``, a JSON dictionary with every recorded number, rt64_* included) the error of the reference's own f32 result against the f64 one: per-sample scalars max_b |v - v64| / (1 + |v64|),
                arrays max |v - v64| / (1 + max |v64|) (the normalisation of test_gpu_particles.py), over the rows that are kept
  rows          the rows the per-coordinate arrays (f64_*, gx64, y64_*) hold

Size: one committed file may hold 1 MiB.  So the per-coordinate f64 arrays are kept for the rows G_ROWS (the first 8 and 118..149, as in
make_particle_goldens.py: the partial last tile of every tile height is whole), the f32 results enter through their errors
only (divergence and dlogp, one number per sample, are kept in f64 on every row), the ``edge`` set keeps positions for Nt = 4 only, gx64 is recorded at t = 0.37 (the
time only scales the pair function), and the widest shape holds forces at t = 0.37 and one trajectory (rk4, Nt = 4, forward; ``ref`` only)
-- its other integrations are covered by dlogp on every row.

Edge rows ``edge_`` (n = 4, d = 3, B = 8, set ``ref``, t = 0.37): two coincident particles in rows 0 and 1, one particle 100 away in rows 2
and 3 (every radial basis function of its pairs underflows).

``meta``: JSON -- constructor signatures of KernelDynamics and DiffEqFlow, parameter names and shapes of a KernelDynamics.
"""
import inspect
import json
import os
import sys

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.nn.flow.diffeq import DiffEqFlow  # noqa: E402
from bgflow.nn.flow.dynamics import DensityDynamics, InversedDynamics, KernelDynamics  # noqa: E402

SEED = 20262
SHAPES = ((2, 1), (4, 2), (13, 3), (64, 3))
TIMES = (0.0, 0.37, 1.0)
T_MAX = 1.0
G_ROWS = np.r_[0:8, 118:150]
PARAMS = ("_weights", "_bias", "_importance", "_neg_log_gammas_time")
CONFIGS = [(m, nt, dr) for m in ("rk4", "euler") for nt in (1, 4) for dr in ("f", "i")]


def kernel_set(name, dtype):
    if name == "ref":
        return dict(mus=torch.linspace(0, 8, 10, dtype=dtype), gammas=torch.full((10,), 0.3, dtype=dtype),
                    mus_time=torch.linspace(0, 1, 5, dtype=dtype), gammas_time=torch.full((5,), 0.3, dtype=dtype))
    return dict(mus=torch.linspace(0, 8, 64, dtype=dtype), gammas=torch.full((64,), 0.3, dtype=dtype),
                mus_time=torch.linspace(0, 1, 16, dtype=dtype), gammas_time=torch.full((16,), 0.1, dtype=dtype))


def make(name, n, d, values, dtype):
    dyn = KernelDynamics(n, d, optimize_t_gammas=True, **kernel_set(name, dtype))
    with torch.no_grad():
        for p in ("_weights", "_bias", "_importance"):
            getattr(dyn, p).data = torch.tensor(values[p], dtype=dtype)
    return dyn


def seeded(rng, K, O, n):
    return {"_weights": rng.normal(size=(K, O)) * np.sqrt(1.0 / K) * 0.5 / np.sqrt(n),
            "_bias": rng.normal(size=(1, O)) * 0.1 / np.sqrt(n),
            "_importance": rng.normal(size=(K,)) * 0.5}


def integrate(dynamics, state, n_steps, method, dtype):
    h = T_MAX / n_steps
    tt = lambda v: torch.tensor(v, dtype=dtype)     # noqa: E731
    for step in range(n_steps):
        t = step * h
        if method == "euler":
            k1 = dynamics(tt(t), state)
            state = tuple(y + h * a for y, a in zip(state, k1))
            continue
        k1 = dynamics(tt(t), state)
        k2 = dynamics(tt(t + 0.5 * h), tuple(y + (0.5 * h) * a for y, a in zip(state, k1)))
        k3 = dynamics(tt(t + 0.5 * h), tuple(y + (0.5 * h) * a for y, a in zip(state, k2)))
        k4 = dynamics(tt(t + h), tuple(y + h * a for y, a in zip(state, k3)))
        state = tuple(y + (h / 6.0) * (a + 2.0 * b + 2.0 * c + e) for y, a, b, c, e in zip(state, k1, k2, k3, k4))
    return state


def flow(dyn, x, n_steps, method, direction):
    dynamics = DensityDynamics(dyn) if direction == "f" else DensityDynamics(InversedDynamics(dyn, T_MAX))
    with torch.no_grad():
        y, dlogp = integrate(dynamics, (x, torch.zeros(x.shape[0], 1, dtype=x.dtype)), n_steps, method, x.dtype)
    return y, dlogp


def err_s(v, v64):
    v, v64 = np.asarray(v, dtype=np.float64).reshape(-1), np.asarray(v64).reshape(-1)
    return np.float64(np.max(np.abs(v - v64) / (1.0 + np.abs(v64))))


def err_a(v, v64):
    v, v64 = np.asarray(v, dtype=np.float64), np.asarray(v64)
    return np.float64(np.max(np.abs(v - v64)) / (1.0 + np.max(np.abs(v64))))


def cotangents(B, nd):
    """a [B, nd] and b [B] of the scalar sum(forces a) + sum(div b) whose gradients are recorded (a formula, so that no array is stored)"""
    i = np.arange(B * nd, dtype=np.float64).reshape(B, nd)
    return torch.tensor(np.cos(0.7 * i + 0.3)), torch.tensor(np.sin(1.3 * np.arange(B, dtype=np.float64) + 0.1))


def evaluate(dyn, x, t, ga, gb, grads):
    x = x.clone().requires_grad_(grads)
    forces, neg_div = dyn(torch.tensor(t, dtype=x.dtype), x)
    div = -neg_div.reshape(-1)
    res = {"f": forces.detach().numpy(), "div": div.detach().numpy()}
    if grads:
        loss = (forces * ga.to(x.dtype)).sum() + (div * gb.to(x.dtype)).sum()
        wrt = [x] + [getattr(dyn, p) for p in PARAMS]
        got = torch.autograd.grad(loss, wrt)
        res["gx"] = got[0].numpy()
        for p, g in zip(PARAMS, got[1:]):
            res["g" + p] = g.numpy()
    return res


def case(out, key, name, n, d, x32, rng, wide_rows, lean):
    B = x32.shape[0]
    K, O = (10, 5) if name == "ref" else (64, 16)
    values = seeded(rng, K, O, n)
    dyn64, dyn32 = make(name, n, d, values, torch.float64), make(name, n, d, values, torch.float32)
    for p, v in values.items():
        out[f"{key}p{p}"] = v
    rows = wide_rows
    out[key + "rows"] = rows.astype(np.int32)
    ga, gb = cotangents(B, n * d)
    x64 = torch.tensor(x32.reshape(B, n * d), dtype=torch.float64)
    xf = torch.tensor(x32.reshape(B, n * d))
    div64, g64 = [], {p: [] for p in PARAMS}
    for i, t in enumerate(TIMES):
        r64, r32 = evaluate(dyn64, x64, t, ga, gb, True), evaluate(dyn32, xf, t, ga, gb, True)
        assert r64["f"].dtype == np.float64 and r32["f"].dtype == np.float32 and np.isfinite(r64["f"]).all()
        if not lean or i == 1:
            out[f"{key}f64_t{i}"] = r64["f"][rows]
        div64.append(r64["div"])
        out[f"{key}err_f32_t{i}"], out[f"{key}err_div32_t{i}"] = err_a(r32["f"][rows], r64["f"][rows]), err_s(r32["div"], r64["div"])
        if i == 1:
            out[key + "gx64"] = r64["gx"][rows]
        out[f"{key}err_gx32_t{i}"] = err_a(r32["gx"][rows], r64["gx"][rows])
        for p in PARAMS:
            g64[p].append(r64["g" + p])
            out[f"{key}err_g32_t{i}{p}"] = err_a(r32["g" + p], r64["g" + p])
        print(f"{key}t{i}: |f| <= {np.abs(r64['f']).max():.3g}, |div| <= {np.abs(r64['div']).max():.3g}, err_f32 {out[f'{key}err_f32_t{i}']:.3g}, "
              f"err_div32 {out[f'{key}err_div32_t{i}']:.3g}, err_gx32 {out[f'{key}err_gx32_t{i}']:.3g}, "
              f"err_gW32 {out[f'{key}err_g32_t{i}_weights']:.3g}")
    out[key + "div64"] = np.stack(div64)
    for p in PARAMS:
        out[f"{key}g64{p}"] = np.stack(g64[p])
    ends, dlogp64 = {}, []
    for m, nt, dr in CONFIGS:
        tag = f"{m}{nt}{dr}"
        y64, l64 = flow(dyn64, x64, nt, m, dr)
        y32, l32 = flow(dyn32, xf, nt, m, dr)
        assert torch.isfinite(y64).all() and torch.isfinite(l64).all()
        ends[tag] = y64
        if (tag == "rk44f" and name == "ref") if lean else (name == "ref" or nt == 4):
            out[f"{key}y64_{tag}"] = y64.numpy()[rows]
        dlogp64.append(l64.numpy().reshape(-1))
        out[f"{key}err_y32_{tag}"] = err_a(y32.numpy()[rows], y64.numpy()[rows])
        out[f"{key}err_dlogp32_{tag}"] = err_s(l32.numpy(), l64.numpy())
        print(f"{key}{tag}: |y| <= {y64.abs().max():.3g}, |dlogp| <= {l64.abs().max():.3g}, err_y32 {out[f'{key}err_y32_{tag}']:.3g}, "
              f"err_dlogp32 {out[f'{key}err_dlogp32_{tag}']:.3g}")
    out[key + "dlogp64"] = np.stack(dlogp64)
    for m in ("rk4", "euler"):
        for nt in (1, 4):
            back, lb = flow(dyn64, ends[f"{m}{nt}f"], nt, m, "i")
            out[f"{key}rt64_{m}{nt}"] = np.float64((back - x64).abs().max())
            print(f"{key}round trip {m}{nt}: {out[f'{key}rt64_{m}{nt}']:.3g}")


def main():
    rng = np.random.default_rng(SEED)
    P = np.load(os.path.join(HERE, "particles.npz"))
    out = {"seed": np.int64(SEED), "times": np.array(TIMES), "t_max": np.float64(T_MAX)}
    for name in ("ref", "edge"):
        for n, d in SHAPES:
            case(out, f"{name}_{n}_{d}_", name, n, d, P[f"x_{n}_{d}"], rng, G_ROWS, lean=n * d > 64)

    # edge rows: coincident particles (0, 1), one particle far away (2, 3)
    n, d = 4, 3
    x = rng.integers(-256, 257, size=(8, n, d)) / 256.0 * 1.5
    x[0, 2] = x[0, 0]
    x[1, 3] = x[1, 1]
    x[2, 1] += 100.0
    x[3, 0, 2] -= 100.0
    x = x.astype(np.float32)
    out["edge_x"] = x
    values = seeded(rng, 10, 5, n)
    for p, v in values.items():
        out[f"edge_p{p}"] = v
    ga, gb = cotangents(8, n * d)
    r64 = evaluate(make("ref", n, d, values, torch.float64), torch.tensor(x.reshape(8, -1), dtype=torch.float64), TIMES[1], ga, gb, True)
    r32 = evaluate(make("ref", n, d, values, torch.float32), torch.tensor(x.reshape(8, -1)), TIMES[1], ga, gb, True)
    assert all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    out["edge_f64"], out["edge_div64"], out["edge_gx64"] = r64["f"], r64["div"], r64["gx"]
    out["edge_f32"], out["edge_div32"], out["edge_gx32"] = r32["f"], r32["div"], r32["gx"]
    out["edge_err_f32"], out["edge_err_div32"], out["edge_err_gx32"] = err_a(r32["f"], r64["f"]), err_s(r32["div"], r64["div"]), err_a(r32["gx"], r64["gx"])
    for p in PARAMS:
        out[f"edge_g64{p}"] = r64["g" + p]
        out[f"edge_err_g32{p}"] = err_a(r32["g" + p], r64["g" + p])
    print("edge rows: err_f32", out["edge_err_f32"], "err_div32", out["edge_err_div32"], "err_gx32", out["edge_err_gx32"])

    def signature(cls):
        return [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name]
                for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]

    dyn = make("ref", 4, 2, seeded(rng, 10, 5, 4), torch.float32)
    meta = {"KernelDynamics": {"parameters": signature(KernelDynamics),
                               "named_parameters": {k: list(v.shape) for k, v in dyn.named_parameters()}},
            "DiffEqFlow": {"parameters": signature(DiffEqFlow)}}
    out["meta"] = np.array(json.dumps(meta))
    scalars = {k: float(v) for k, v in out.items() if isinstance(v, np.float64)}      # one entry instead of several hundred
    for k in scalars:
        del out[k]
    out["scalars"] = np.array(json.dumps(scalars))
    path = os.path.join(HERE, "kernel_dynamics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
