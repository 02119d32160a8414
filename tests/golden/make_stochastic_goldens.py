#!/usr/bin/env python
"""Generate tests/golden/stochastic.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_stochastic_goldens.py

What runs: the UNMODIFIED reference classes ``BrownianFlow`` / ``LangevinFlow`` (nn/flow/stochastic/langevin.py) and ``MetropolisMCFlow``
(stochastic/mcmc.py) on the reference's ``LennardJonesPotential``, ``MultiDoubleWellPotential`` and ``MeanFreeNormalDistribution``
(``two_event_dims=False``), with the two import shims of make_goldens.py.  The random numbers are FIXED: ``torch.Tensor.normal_`` and
``torch.rand`` are patched to hand out recorded rows.  The f64 runs are made under ``torch.set_default_dtype(torch.float64)``: the layers
create their noise and dW with the default dtype.  The fixture holds DATA only.

Inputs: the start states ``x_{n}_{d}`` of particles.npz (B = 150) and its parameters (LJ eps 0.7, rm 1.3, oscillator 0.5; MDW a 0.9,
b -4, c 0.1, offset 4; mean-free normal std 0.8).  Random numbers of step s (regenerated identically by the tests from oracle/philox.py;
only ``normal_sum_{f}_{n}_{d}`` / ``normal_absmax_{f}_{n}_{d}`` / ``unif_sum`` / ``unif_absmax`` / ``v0_sum_{n}_{d}`` are stored):

    normals of field f in {0, 1}:  sample_field(SEED, s, f, 150, n d, 1).astype(float32)     (Brownian w and Metropolis noise: f = 0;
                                                                                              Langevin w1: f = 0, w2: f = 1)
    uniforms:  sample_field(SEED, s, 1, 150, 1, 0)[:, 0]          Langevin start velocities:  sample_field(SEED, V0_OFFSET, 0, 150, n d, 1)

Cases, kind in {lj (oscillator), mdw, mfn} x (n, d) in {(2,1), (4,2), (13,3), (64,3)}:
  brownian_{kind}_{n}_{d}_{nsteps}    nsteps in {1, 12}
  langevin_{kind}_{n}_{d}_{nsteps}    nsteps in {1, 12}, mass = gamma = kT = 1;  langevin_{kind}_13_3_12_p: mass, gamma, kT = PARAMS
  metropolis_{kind}_{n}_{d}_48
Step sizes per case in STEPSIZE (chosen so that the reference alone meets the conditions asserted below).  Per case, from the f64 run:

  x64 (v64)  final state(s), [rows, n d]; ``rows``: all 150 for n d = 2, ROWS (24 rows: the head of the first tile and the tail with the
             partial last tile of every tile height) up to n d = 39, ROWS_WIDE (12 rows) at n d = 192 -- the file stays below 1 MiB
  dW64       [150], every row
  err_x32, err_v32, err_dW32   max |f32 run - f64 run| of the reference over the stored rows (dW: all rows; Metropolis: kept chains)
  metropolis: e64 final energies [150], err_e32, acc accepted steps [150] (int32), margin = min over the steps of
             |min(0, -dE) - log r| per chain, keep = margin >= 1e-3 (as in mcmc.npz)
  stepsize, params (mass, gamma, kT)

Gradients, (4, 2) with nsteps = 3: ``grad_{layer}_{kind}_g64`` = d (dW.sum() + y.sum()) / d x [150, 8] (langevin: y = q' and v', and
``..._gv64`` with respect to v) from the f64 run, ``..._err_g32`` the reference's f32 error of it (``..._err_gv32``); kind in {lj, mfn}:
the reference's multi-double-well goes through ``torch.cdist``, whose backward torch cannot differentiate again.

Asserted here: every stored value is finite in both precisions; |x32 - x64| <= 1e-3 (1 + |x64|) elementwise for the integrators (the
comparison is not about chaotic amplification); keep covers >= 85 % of every Metropolis case; the reference's f32 run decides like its
f64 run at every step of every kept chain; Metropolis acceptance within 25-80 %.

``meta``: JSON -- constructor signatures (parameter names and defaults) of the three classes.
"""
import inspect
import json
import os
import sys

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.distribution.energy.lennard_jones import LennardJonesPotential  # noqa: E402
from bgflow.distribution.energy.multi_double_well_potential import MultiDoubleWellPotential  # noqa: E402
from bgflow.distribution.normal import MeanFreeNormalDistribution  # noqa: E402
from bgflow.nn.flow.stochastic import langevin, mcmc  # noqa: E402
from oracle import philox  # noqa: E402

SEED, B = 20263, 150
V0_OFFSET = 4096
SHAPES = [(2, 1), (4, 2), (13, 3), (64, 3)]
KINDS = ["lj", "mdw", "mfn"]
NSTEPS = (1, 12)
MC_STEPS = 48
GRAD_STEPS = 3
PARAMS = (1.7, 0.6, 1.3)           # mass, gamma, kT of the "_p" cases
ROWS = np.r_[0:8, 134:150]
ROWS_WIDE = np.r_[0:4, 142:150]
MARGIN = 1e-3
# (layer, kind, n, d): stepsize
STEPSIZE = {
    ("brownian", "lj", 2, 1): 1e-3, ("brownian", "lj", 4, 2): 1e-3, ("brownian", "lj", 13, 3): 2e-4, ("brownian", "lj", 64, 3): 1e-4,
    ("brownian", "mdw", 2, 1): 5e-3, ("brownian", "mdw", 4, 2): 5e-3, ("brownian", "mdw", 13, 3): 1e-3, ("brownian", "mdw", 64, 3): 2e-4,
    ("brownian", "mfn", 2, 1): 0.05, ("brownian", "mfn", 4, 2): 0.05, ("brownian", "mfn", 13, 3): 0.05, ("brownian", "mfn", 64, 3): 0.05,
    ("langevin", "lj", 2, 1): 0.02, ("langevin", "lj", 4, 2): 0.02, ("langevin", "lj", 13, 3): 5e-3, ("langevin", "lj", 64, 3): 2e-3,
    ("langevin", "mdw", 2, 1): 0.05, ("langevin", "mdw", 4, 2): 0.05, ("langevin", "mdw", 13, 3): 0.02, ("langevin", "mdw", 64, 3): 5e-3,
    ("langevin", "mfn", 2, 1): 0.1, ("langevin", "mfn", 4, 2): 0.1, ("langevin", "mfn", 13, 3): 0.1, ("langevin", "mfn", 64, 3): 0.1,
    ("metropolis", "lj", 2, 1): 0.2, ("metropolis", "lj", 4, 2): 0.1, ("metropolis", "lj", 13, 3): 0.03, ("metropolis", "lj", 64, 3): 0.015,
    ("metropolis", "mdw", 2, 1): 0.3, ("metropolis", "mdw", 4, 2): 0.3, ("metropolis", "mdw", 13, 3): 0.08, ("metropolis", "mdw", 64, 3): 0.015,
    ("metropolis", "mfn", 2, 1): 1.0, ("metropolis", "mfn", 4, 2): 0.4, ("metropolis", "mfn", 13, 3): 0.2, ("metropolis", "mfn", 64, 3): 0.08,
}


def normals(field, nd, n_steps):
    return np.stack([philox.sample_field(SEED, s, field, B, nd, 1).astype(np.float32) for s in range(n_steps)])


def uniforms(n_steps):
    return np.stack([philox.sample_field(SEED, s, 1, B, 1, 0)[:, 0] for s in range(n_steps)])


class Recorded:
    """patches ``torch.Tensor.normal_`` and ``torch.rand`` to hand out the rows of ``normal_rows`` / ``uniform_rows`` in turn"""

    def __init__(self, normal_rows, uniform_rows=()):
        self.normal_rows, self.uniform_rows = list(normal_rows), list(uniform_rows)
        self.n_normal = self.n_uniform = 0

    def __enter__(self):
        outer = self

        def normal_(tensor, *args, **kwargs):
            row = outer.normal_rows[outer.n_normal]
            outer.n_normal += 1
            with torch.no_grad():
                tensor.copy_(torch.from_numpy(row).reshape(tensor.shape))
            return tensor

        def rand(*size, **kwargs):
            row = outer.uniform_rows[outer.n_uniform]
            outer.n_uniform += 1
            return torch.from_numpy(row).reshape(*size).to(torch.get_default_dtype())

        self.saved = (torch.Tensor.normal_, torch.rand)
        torch.Tensor.normal_, torch.rand = normal_, rand
        return self

    def __exit__(self, *exc):
        torch.Tensor.normal_, torch.rand = self.saved
        assert exc[0] is not None or (self.n_normal == len(self.normal_rows) and self.n_uniform == len(self.uniform_rows))


def make(kind, n, d, P):
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        return LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=False)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in P["mdw_params"])
        return MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)
    return MeanFreeNormalDistribution(n * d, n, std=float(P["mfn_std"]), two_event_dims=False)


class default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.saved = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.saved)


def interleave(a, b):
    return [r for pair in zip(a, b) for r in pair]


def run_integrator(layer, energy, x0, v0, nsteps, stepsize, params, dtype, grad=False):
    """the reference layer on fixed numbers in ``dtype``: numpy (x, [v,] dW [B]) or, with ``grad``, the gradients of dW.sum() + outputs"""
    nd = x0.shape[1]
    w1 = normals(0, nd, nsteps)
    with default_dtype(dtype):
        x = torch.from_numpy(x0).to(dtype).requires_grad_(grad)
        if layer == "brownian":
            flow = langevin.BrownianFlow(energy, nsteps=nsteps, stepsize=stepsize)
            with Recorded(w1):
                *out, dW = flow(x)
            inputs = [x]
        else:
            v = torch.from_numpy(v0).to(dtype).requires_grad_(grad)
            flow = langevin.LangevinFlow(energy, nsteps, stepsize, *params)
            with Recorded(interleave(w1, normals(1, nd, nsteps))):
                *out, dW = flow(x, v)
            inputs = [x, v]
        assert dW.dtype == dtype and all(t.dtype == dtype for t in out) and dW.shape == (B, 1)
        if grad:
            return [g.numpy() for g in torch.autograd.grad(dW.sum() + sum(t.sum() for t in out), inputs)]
        return [t.detach().numpy() for t in out] + [dW.detach().numpy()[:, 0]]


def run_metropolis(energy, x0, stepsize, dtype):
    """-> x [B, n d], e [B], dW [B], decisions [48, B], margins [48, B]"""
    nd = x0.shape[1]
    noise, unif = normals(0, nd, MC_STEPS), uniforms(MC_STEPS)
    calls = []
    original = energy.energy
    energy.energy = lambda x: calls.append(original(x).detach().clone()) or calls[-1]
    try:
        with default_dtype(dtype):
            flow = mcmc.MetropolisMCFlow(energy, nsteps=MC_STEPS, stepsize=stepsize)
            with Recorded(noise, unif):
                x, dW = flow(torch.from_numpy(x0).to(dtype))
    finally:
        del energy.energy
    assert len(calls) == MC_STEPS + 1 and x.dtype == dtype and dW.dtype == dtype
    # the decisions, replayed from the proposal energies the layer saw: acc = r < exp(-(Eprop - E))
    E = calls[0]
    dec, mar = [], []
    for s in range(MC_STEPS):
        r = torch.from_numpy(unif[s]).to(dtype)[:, None]
        log_prob = -(calls[s + 1] - E)
        acc = r < torch.exp(log_prob)
        dec.append(acc[:, 0].numpy())
        mar.append(np.abs(np.minimum(0.0, log_prob.double().numpy()[:, 0]) - np.log(unif[s].astype(np.float64))))
        E = torch.where(acc, calls[s + 1], E)
    assert torch.equal(E - calls[0], dW)
    return x.numpy(), E.numpy()[:, 0], dW.numpy()[:, 0], np.stack(dec), np.stack(mar)


def signature(fn):
    out = []
    for p in list(inspect.signature(fn).parameters.values()):
        if p.name == "self":
            continue
        d = p.default
        out.append([p.name, "<required>" if d is inspect.Parameter.empty else d])
    return out


def stored_rows(nd):
    return np.arange(B) if nd <= 2 else (ROWS if nd <= 64 else ROWS_WIDE)


def main():
    P = np.load(os.path.join(HERE, "particles.npz"))
    out = {"seed": np.int64(SEED), "v0_offset": np.int64(V0_OFFSET), "mc_steps": np.int64(MC_STEPS), "grad_steps": np.int64(GRAD_STEPS),
           "margin_threshold": np.float64(MARGIN), "params_p": np.array(PARAMS, np.float64)}
    unif = uniforms(MC_STEPS)
    out["unif_sum"], out["unif_absmax"] = np.float64(unif.astype(np.float64).sum()), np.float64(unif.max())
    for n, d in SHAPES:
        nd = n * d
        for f in (0, 1):
            w = normals(f, nd, MC_STEPS if f == 0 else max(NSTEPS))
            out[f"normal_sum_{f}_{n}_{d}"], out[f"normal_absmax_{f}_{n}_{d}"] = np.float64(w.astype(np.float64).sum()), np.float64(np.abs(w).max())
        v0 = philox.sample_field(SEED, V0_OFFSET, 0, B, nd, 1).astype(np.float32)
        out[f"v0_sum_{n}_{d}"] = np.float64(v0.astype(np.float64).sum())
        rows = stored_rows(nd)
        for kind in KINDS:
            energy = make(kind, n, d, P)
            x0 = P[f"x_{n}_{d}"].reshape(B, nd)
            # -- the integrators
            for layer in ("brownian", "langevin"):
                h = STEPSIZE[(layer, kind, n, d)]
                variants = [(k, (1.0, 1.0, 1.0), "") for k in NSTEPS]
                if layer == "langevin" and (n, d) == (13, 3):
                    variants.append((max(NSTEPS), PARAMS, "_p"))
                for nsteps, params, tag in variants:
                    key = f"{layer}_{kind}_{n}_{d}_{nsteps}{tag}_"
                    r64 = run_integrator(layer, energy, x0, v0, nsteps, h, params, torch.float64)
                    r32 = run_integrator(layer, energy, x0, v0, nsteps, h, params, torch.float32)
                    assert all(np.isfinite(a).all() for a in r64 + r32), key
                    names = ["x", "dW"] if layer == "brownian" else ["x", "v", "dW"]
                    msg = []
                    for name, a64, a32 in zip(names, r64, r32):
                        assert a64.dtype == np.float64 and a32.dtype == np.float32
                        if name == "dW":
                            out[key + "dW64"], err = a64, np.abs(a32 - a64).max()
                        else:
                            assert (np.abs(a32 - a64) <= 1e-3 * (1 + np.abs(a64))).all(), (key, name, np.abs(a32 - a64).max())
                            out[key + name + "64"], err = a64[rows], np.abs(a32[rows] - a64[rows]).max()
                        out[key + f"err_{name}32"] = np.float64(err)
                        msg.append(f"err_{name}32 {err:.3g}")
                    out[key + "rows"], out[key + "stepsize"], out[key + "params"] = rows.astype(np.int32), np.float64(h), np.array(params, np.float64)
                    print(f"{key[:-1]}: " + ", ".join(msg) + f", |dW| up to {np.abs(r64[-1]).max():.3g}, |x - x0| up to {np.abs(r64[0] - x0).max():.3g}")
                if (n, d) == (4, 2) and kind != "mdw":
                    key = f"grad_{layer}_{kind}_"
                    g64 = run_integrator(layer, energy, x0, v0, GRAD_STEPS, h, (1.0, 1.0, 1.0), torch.float64, grad=True)
                    g32 = run_integrator(layer, energy, x0, v0, GRAD_STEPS, h, (1.0, 1.0, 1.0), torch.float32, grad=True)
                    for name, a64, a32 in zip(("g", "gv"), g64, g32):
                        assert np.isfinite(a64).all() and np.isfinite(a32).all() and a64.dtype == np.float64
                        out[key + name + "64"], out[key + f"err_{name}32"] = a64, np.float64(np.abs(a32 - a64).max())
                        print(f"{key}{name}: |g| up to {np.abs(a64).max():.3g}, f32 error {np.abs(a32 - a64).max():.3g}")
            # -- Metropolis
            h = STEPSIZE[("metropolis", kind, n, d)]
            key = f"metropolis_{kind}_{n}_{d}_{MC_STEPS}_"
            x64, e64, dW64, dec64, mar64 = run_metropolis(energy, x0, h, torch.float64)
            x32, e32, dW32, dec32, _ = run_metropolis(energy, x0, h, torch.float32)
            assert all(np.isfinite(a).all() for a in (x64, e64, dW64, x32, e32, dW32)), key
            margin = mar64.min(axis=0)
            keep = margin >= MARGIN
            acc = dec64.sum(axis=0).astype(np.int32)
            rate = acc.mean() / MC_STEPS
            assert keep.mean() >= 0.85, (key, keep.mean())
            assert (dec32[:, keep] == dec64[:, keep]).all(), key
            assert 0.25 <= rate <= 0.80, (key, rate)
            kr = keep[rows]
            out[key + "x64"], out[key + "rows"], out[key + "e64"], out[key + "dW64"] = x64[rows], rows.astype(np.int32), e64, dW64
            out[key + "acc"], out[key + "margin"], out[key + "keep"] = acc, margin, keep
            out[key + "err_x32"] = np.float64(np.abs(x32[rows][kr] - x64[rows][kr]).max())
            out[key + "err_e32"] = np.float64(np.abs(e32[keep] - e64[keep]).max())
            out[key + "err_dW32"] = np.float64(np.abs(dW32[keep] - dW64[keep]).max())
            out[key + "stepsize"] = np.float64(h)
            print(f"{key[:-1]}: acceptance {rate:.2f}, kept {int(keep.sum())} / {B}, err_x32 {float(out[key + 'err_x32']):.3g}, "
                  f"err_e32 {float(out[key + 'err_e32']):.3g}, err_dW32 {float(out[key + 'err_dW32']):.3g}")

    meta = {"BrownianFlow": signature(langevin.BrownianFlow.__init__), "LangevinFlow": signature(langevin.LangevinFlow.__init__),
            "MetropolisMCFlow": signature(mcmc.MetropolisMCFlow.__init__),
            "OverdampedLangevinFlow_is_BrownianFlow": langevin.OverdampedLangevinFlow is langevin.BrownianFlow}
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "stochastic.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
