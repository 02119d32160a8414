#!/usr/bin/env python
"""Generate tests/golden/particles.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_particle_goldens.py

What runs: the UNMODIFIED reference classes ``LennardJonesPotential`` (distribution/energy/lennard_jones.py),
``MultiDoubleWellPotential`` (energy/multi_double_well_potential.py) and ``MeanFreeNormalDistribution`` (distribution/normal.py), with
the two import shims of make_goldens.py (``numpy.infty``, nflows_stub).  The fixture holds DATA only.

Cases: kind in {lj (oscillator, scale 0.5), ljn (no oscillator), mdw, mfn} x (n, d) in {(2,1), (4,2), (13,3), (55,3), (64,3)}, B = 150.
LJ: eps = 0.7, rm = 1.3; MDW: a = 0.9, b = -4, c = 0.1, offset = 4; mean-free normal: std = 0.8.  Positions ``x_{n}_{d}`` (shared by the
kinds) are a lattice of spacing 1.5 with a jitter of at most 0.2 per coordinate in steps of 1 / 256: the minimum pair distance is
>= 1.1 >= 0.8 rm (asserted), every golden energy is finite and below 1e4 in magnitude (asserted).  Per case ``{kind}_{n}_{d}_*``:

  u64    the reference on x.double()                        u32   the reference on x (f32)
  g64    f64 autograd of u.sum() w.r.t. x                   g_rows   the rows g64 holds
  err_u32 = max_b |u32 - u64| / (1 + |u64|)                 err_g32 = max |g32 - g64| / (1 + max |g64|), g32 the reference's f32 autograd

g64 of the two widest shapes is kept for the rows G_ROWS_WIDE only (the first rows and every row from the last full 32-row tile on, so
the partial last tile of either tile height is whole): all 150 rows of all cases in f64 would be 1.9 MB, beyond what one committed
fixture may hold.  err_g32 is taken over the rows that are kept.

Edge cases ``edge_{lj,mdw}_*`` (n = 4, d = 3, B = 8): samples 0 and 1 have two coincident particles each.  u32 / g32 are the reference's
f32 results as they come (inf / NaN included); u64 / g64 and the errors over samples 2..7 as above.

``meta``: JSON -- constructor signatures (parameter names and defaults) and event shapes of the three classes.
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

from bgflow.distribution.energy.lennard_jones import LennardJonesPotential  # noqa: E402
from bgflow.distribution.energy.multi_double_well_potential import MultiDoubleWellPotential  # noqa: E402
from bgflow.distribution.normal import MeanFreeNormalDistribution  # noqa: E402

SEED, B = 20261, 150
SHAPES = ((2, 1), (4, 2), (13, 3), (55, 3), (64, 3))
LJ = dict(eps=0.7, rm=1.3, oscillator_scale=0.5)
MDW = dict(a=0.9, b=-4.0, c=0.1, offset=4.0)
STD = 0.8
SPACING, JITTER = 1.5, 0.2
G_ROWS_WIDE = np.r_[0:8, 118:150]


def make(kind, n, d):
    if kind == "lj":
        return LennardJonesPotential(n * d, n, oscillator=True, **LJ)
    if kind == "ljn":
        return LennardJonesPotential(n * d, n, oscillator=False, **LJ)
    if kind == "mdw":
        return MultiDoubleWellPotential(n * d, n, **MDW)
    return MeanFreeNormalDistribution(n * d, n, std=STD)


def lattice(rng, n, d, batch):
    side = int(np.ceil(n ** (1.0 / d) - 1e-9))
    pts = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), -1).reshape(-1, d)[:n].astype(np.float64)
    pts = (pts - pts.mean(0)) * SPACING
    steps = int(JITTER * 256)
    x = pts[None] + rng.integers(-steps, steps + 1, size=(batch, n, d)) / 256.0
    return x.astype(np.float32)


def evaluate(energy, x):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x)
    (g,) = torch.autograd.grad(u.sum(), x)
    return u.detach().numpy().reshape(-1), g.numpy().reshape(x.shape[0], -1)


def err_u(v, u64):
    return float(np.max(np.abs(v.astype(np.float64) - u64) / (1.0 + np.abs(u64))))


def err_g(v, g64):
    return float(np.max(np.abs(v.astype(np.float64) - g64)) / (1.0 + np.max(np.abs(g64))))


def main():
    rng = np.random.default_rng(SEED)
    out = {"seed": np.int64(SEED)}
    for n, d in SHAPES:
        x = lattice(rng, n, d, B)
        diff = x[:, :, None].astype(np.float64) - x[:, None].astype(np.float64)
        dist = np.sqrt((diff ** 2).sum(-1)) + 1e9 * np.eye(n)
        assert dist.min() >= 0.8 * LJ["rm"], (n, d, dist.min())
        out[f"x_{n}_{d}"] = x
        xt = torch.from_numpy(x)
        for kind in ("lj", "ljn", "mdw", "mfn"):
            energy = make(kind, n, d)
            u64, g64 = evaluate(energy, xt.double())
            u32, g32 = evaluate(energy, xt)
            assert u64.dtype == np.float64 and u32.dtype == np.float32
            assert np.isfinite(u64).all() and np.abs(u64).max() < 1e4, (kind, n, d, np.abs(u64).max())
            rows = G_ROWS_WIDE if n * d > 64 else np.arange(B)
            key = f"{kind}_{n}_{d}"
            out[key + "_u64"], out[key + "_u32"] = u64, u32
            out[key + "_g64"], out[key + "_g_rows"] = g64[rows], rows.astype(np.int32)
            out[key + "_err_u32"], out[key + "_err_g32"] = np.float64(err_u(u32, u64)), np.float64(err_g(g32[rows], g64[rows]))
            print(f"{key}: |u64| <= {np.abs(u64).max():.4g}, err_u32 {err_u(u32, u64):.3g}, err_g32 {err_g(g32[rows], g64[rows]):.3g}")

    # two coincident particles in samples 0 and 1
    n, d = 4, 3
    x = lattice(rng, n, d, 8)
    x[0, 2] = x[0, 0]
    x[1, 3] = x[1, 1]
    xt = torch.from_numpy(x)
    for kind in ("lj", "mdw"):
        energy = make(kind, n, d)
        u64, g64 = evaluate(energy, xt.double())
        u32, g32 = evaluate(energy, xt)
        key = f"edge_{kind}"
        out[key + "_x"] = x
        out[key + "_u64"], out[key + "_u32"], out[key + "_g64"], out[key + "_g32"] = u64, u32, g64, g32
        out[key + "_err_u32"], out[key + "_err_g32"] = np.float64(err_u(u32[2:], u64[2:])), np.float64(err_g(g32[2:], g64[2:]))
        print(f"{key}: u32[:2] = {u32[:2]}, finite g32 rows: {np.isfinite(g32).all(1)}")

    meta = {}
    for cls in (LennardJonesPotential, MultiDoubleWellPotential, MeanFreeNormalDistribution):
        sig = inspect.signature(cls.__init__)
        params = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in list(sig.parameters.values())[1:]]
        kw = dict(a=1.0, b=1.0, c=1.0, offset=1.0) if cls is MultiDoubleWellPotential else {}
        meta[cls.__name__] = {
            "parameters": params,
            "event_shape_two_dims": list(cls(12, 4, **kw).event_shape),
            "event_shape_one_dim": list(cls(12, 4, two_event_dims=False, **kw).event_shape),
        }
    out["meta"] = np.array(json.dumps(meta))
    out["lj_params"] = np.array([LJ["eps"], LJ["rm"], LJ["oscillator_scale"]])
    out["mdw_params"] = np.array([MDW["a"], MDW["b"], MDW["c"], MDW["offset"]])
    out["mfn_std"] = np.float64(STD)

    path = os.path.join(HERE, "particles.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
