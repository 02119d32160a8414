#!/usr/bin/env python
"""Generate tests/golden/g_clipped.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_clip_goldens.py

What runs: the UNMODIFIED reference functions / classes ``linlogcut``, ``ClipGradient`` (utils/train.py:60-118),
``LinLogCutEnergy``, ``GradientClippedEnergy`` (distribution/energy/clipped.py:8-38) around ``NormalDistribution`` and
``DoubleWellEnergy``, with the two import shims of make_goldens.py (``numpy.infty``, nflows_stub).
The fixture holds DATA only: inputs and the reference's results.

  * ``cut_*``: linlogcut values and gradients of the sum, for (high, max) = (5, 8) and the defaults (1e3, 1e9);
  * ``clip{W}_*``: ClipGradient.clip_tensor with clip = 1 on [12, W] gradients, W = 66 and 6, for norm_dim 1, 3 and -1.  Rows: 0-1 below
    the threshold, 2-3 above, 4-5 mixing both, 6-7 zero, 8-9 with NaN, 10-11 with +-inf.  norm_dim -1 is recorded twice: over all twelve rows
    (``_m1``: whatever the reference does with the +-inf rows) and over rows 0-9 (``_m1f``: a finite whole-tensor norm);
  * ``n66_*`` / ``dw64_*``: energies and x-gradients (of the energy sum) of the wrapper chains at temperatures 1.0 and 1.7.  Per-sample
    input scales spread the uncut energies over all three branches of the cut; no uncut energy lies within 1e-4 of a branch point
    (asserted here).  NormalDistribution(66) has energies >= 33 log(2 pi) = 60.6, so with (5, 8) every sample sits on the clamp
    (gradients 0); the ``n66h_*`` entries repeat the chains with (70, 75), where all three branches occur.
"""
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

from bgflow.distribution.energy.clipped import GradientClippedEnergy, LinLogCutEnergy  # noqa: E402
from bgflow.distribution.energy.double_well import DoubleWellEnergy  # noqa: E402
from bgflow.distribution.normal import NormalDistribution  # noqa: E402
from bgflow.utils.train import ClipGradient, linlogcut  # noqa: E402

SEED, B = 20251, 24
TEMPERATURES = (1.0, 1.7)


def clip_rows(gen, w):
    g = torch.randn(12, w, generator=gen)
    g[0:2] *= 0.05                      # every group (1, 3, whole row of 6) below clip = 1
    g[2:4] = g[2:4] * 3.0 + 4.0 * torch.sign(g[2:4])    # every element above
    g[4:6, ::2] *= 0.05                 # both kinds in one row
    g[4:6, 1::2] *= 5.0
    g[6:8] = 0.0
    g[8, 1] = g[8, w - 1] = float("nan")
    g[9, 0::3] = float("nan")
    g[10, 2] = float("inf")
    g[10, w - 2] = -float("inf")
    g[11, 0] = -float("inf")
    g[11, 3] = float("nan")
    return g


def branch_margin(v, high, max_):
    """distance of the uncut energies from the two branch points of linlogcut(., high, max_)"""
    clamp_from = high - 1.0 + np.exp(max_ - high)
    return float(torch.minimum((v - high).abs(), (v - clamp_from).abs()).min())


def energy_and_grad(energy, x, temperature):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x, temperature=temperature)
    (g,) = torch.autograd.grad(u.sum(), x)
    return u.detach(), g


def main():
    out = {"seed": np.int64(SEED), "temperatures": np.array(TEMPERATURES)}
    gen = torch.Generator().manual_seed(SEED)

    # linlogcut
    v = torch.cat([torch.linspace(-30.0, 60.0, 91), torch.tensor([4.9999, 5.0, 5.0001, 24.0, 24.2, 999.0, 1000.0, 1001.0, 1e6, 1e12, 3e38])])
    out["cut_vals"] = v
    for tag, kw in (("58", dict(high_val=5.0, max_val=8.0)), ("def", {})):
        x = v.clone().requires_grad_(True)
        y = linlogcut(x, **kw)
        (g,) = torch.autograd.grad(y.sum(), x)
        out[f"cut_{tag}_out"], out[f"cut_{tag}_grad"] = y.detach(), g

    # ClipGradient.clip_tensor
    clip = torch.tensor(1.0)
    for w in (66, 6):
        g = clip_rows(gen, w)
        out[f"clip{w}_in"] = g
        for nd in (1, 3):
            out[f"clip{w}_n{nd}"] = ClipGradient.clip_tensor(g, clip, nd)
        out[f"clip{w}_m1"] = ClipGradient.clip_tensor(g, clip, -1)
        out[f"clip{w}_m1f"] = ClipGradient.clip_tensor(g[:10], clip, -1)
    out["clip_value"] = clip

    # wrapper chains
    scale = torch.linspace(0.05, 2.7, B)[:, None]
    xn = torch.randn(B, 66, generator=gen) * scale
    xd = torch.randn(B, 64, generator=gen) * torch.linspace(0.05, 1.3, B)[:, None]
    xd[:, 0] = torch.randn(B, generator=gen) * 1.5
    out["n66_x"], out["dw64_x"] = xn, xd
    normal, well = NormalDistribution(66), DoubleWellEnergy(64)
    vn, vd = normal.energy(xn), well.energy(xd)
    out["n66_uncut"], out["dw64_uncut"] = vn, vd
    for name, vv, hm in (("n66", vn, (5.0, 8.0)), ("n66h", vn, (70.0, 75.0)), ("dw64", vd, (5.0, 8.0))):
        m = branch_margin(vv.double(), *hm)
        assert m > 1e-4, (name, m)
        lo, mid = int((vv < hm[0]).sum()), int(((vv >= hm[0]) & (vv < hm[0] - 1 + np.exp(hm[1] - hm[0]))).sum())
        print(f"{name}: margin to a branch point {m:.3g}; samples below / log / clamped: {lo} / {mid} / {B - lo - mid}")
    out["n_clip"], out["n_norm_dim"], out["dw_clip"], out["dw_norm_dim"] = np.float32(0.05), np.int64(3), np.float32(0.02), np.int64(1)
    clip_n = lambda: ClipGradient(0.05, 3)       # noqa: E731
    clip_d = lambda: ClipGradient(0.02, 1)       # noqa: E731
    chains = {
        "n66_cut_clip": (LinLogCutEnergy(GradientClippedEnergy(normal, clip_n()), 5.0, 8.0), xn),
        "n66_clip_cut": (GradientClippedEnergy(LinLogCutEnergy(normal, 5.0, 8.0), clip_n()), xn),
        "n66h_cut_clip": (LinLogCutEnergy(GradientClippedEnergy(normal, clip_n()), 70.0, 75.0), xn),
        "n66h_clip_cut": (GradientClippedEnergy(LinLogCutEnergy(normal, 70.0, 75.0), clip_n()), xn),
        "dw64_cut": (LinLogCutEnergy(well, 5.0, 8.0), xd),
        "dw64_clip": (GradientClippedEnergy(well, clip_d()), xd),
    }
    for name, (energy, x) in chains.items():
        for t in TEMPERATURES:
            u, g = energy_and_grad(energy, x, t)
            out[f"{name}_T{t}_u"], out[f"{name}_T{t}_g"] = u, g

    path = os.path.join(HERE, "g_clipped.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")
    G = np.load(path)
    for w in (66, 6):
        print(f"width {w}: +-inf rows under norm_dim 1:", G[f"clip{w}_n1"][10, [2, w - 2]], G[f"clip{w}_n1"][11, [0, 3]],
              "norm_dim 3:", G[f"clip{w}_n3"][10, :6], "norm_dim -1, max |.|:", np.abs(G[f"clip{w}_m1"]).max())


if __name__ == "__main__":
    main()
