#!/usr/bin/env python
"""Generate tests/golden/anneal.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_anneal_goldens.py

What runs: the UNMODIFIED reference class ``MCMCStep`` (distribution/sampling/mcmc.py) with ``SamplerState`` (sampling/iterative.py) on
the reference's ``LennardJonesPotential``, ``MultiDoubleWellPotential``, ``MeanFreeNormalDistribution``, ``RepulsiveParticles`` and
``HarmonicParticles``, with the two import shims of make_goldens.py.  The reference has no annealed switching, so the protocol of
bgflow_amd/annealing.py is driven STAGE BY STAGE by this script: a small ``Energy`` of THIS script (``Interpolated``: cA e_A + cB e_B, a
coefficient that is exactly 0 dropping its term) is the target of a reference ``MCMCStep(n_steps=K)`` at temperature 1, one per stage;
before every stage the work increment of the current state is added in f64.  As in make_mcmc_goldens.py the proposal adds recorded noise
and ``torch.rand_like`` is patched for the acceptance draw.  The fixture holds DATA only.

Coefficients: (cA_m, cB_m) = ((1 - l_m) / T_A, l_m / T_B) formed in f64 and rounded to f32 once -- the definition of annealing.py; the
f64 run computes with the rounded values.  LAMBDAS = [0, 0.05, 0.2, 0.45, 0.7, 0.9, 1]: M = 6 stages, K = 2 steps each, 12 steps.

Inputs: the start states and parameters of particles.npz (pair kinds, ``two_event_dims=False``) and box.npz (``x_{nsolvent}``, eps 0.7,
spring constant 150), B = 150 (a partial last tile at both tile heights).  The biased box is the repulsive box with the umbrella
k (d - m)^2 on the dimer distance folded into its parameters (dimer_slope + k (dimer_dmid - m), dimer_a - k / 4), k = 50, m = 1.5.
Random numbers of step s, from mcmc_common.random_numbers / oracle/philox.py (regenerated identically by the tests; only checksums
are stored):   xi_s = sample_field(SEED, s, 0, 150, n d, 1).astype(float32)        r_s = sample_field(SEED, s, 1, 150, 1, 0)[:, 0]

Cases (CASES: the ends, the start state, noise_std, T_A, T_B).  Per case, from the f64 run (start state and noise converted to f64):

  work64   the work per chain [150]                     acc     accepted steps per chain [150] (int32)
  x64      the final state of the first 8 chains [8, n d]
  e_a64 / e_b64   the raw energies of the final state at either end [150]
  margin   min over the steps of |min(0, -du) - log r| per chain [150]
  keep     margin >= 1e-3: below that an f32 evaluation may legitimately decide otherwise, and the chains part ways
  err_x32, err_w32, err_e32   the errors of the same protocol in f32 (the reference's f32 energies; the work still summed in f64 from
           them) on the kept chains: max |x32 - x64|; max |W32 - W64| / (1 + |W64|); max over both ends of |e32 - e64| / (1 + |e64|)
  std, t_a, t_b   the settings

Asserted here: keep covers >= 85 % of every case; the f32 run takes the f64 run's decision at every step of every kept chain (so the
errors measure rounding, not chains that parted ways); the acceptance rate of every case lies in [0.2, 0.9].
"""
import os
import sys

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.distribution.energy.base import Energy  # noqa: E402
from bgflow.distribution.energy.lennard_jones import LennardJonesPotential  # noqa: E402
from bgflow.distribution.energy.multi_double_well_potential import MultiDoubleWellPotential  # noqa: E402
from bgflow.distribution.energy.particles import HarmonicParticles, RepulsiveParticles  # noqa: E402
from bgflow.distribution.normal import MeanFreeNormalDistribution  # noqa: E402
from bgflow.distribution.sampling import iterative, mcmc  # noqa: E402
from mcmc_common import random_numbers  # noqa: E402

SEED, B = 20266, 150
LAMBDAS = [0.0, 0.05, 0.2, 0.45, 0.7, 0.9, 1.0]
K = 2
N_STEPS = (len(LAMBDAS) - 1) * K
CHAINS = 8
MARGIN = 1e-3
EPS, SPRING = 0.7, 150.0          # the box parameters of make_box_goldens.py
UMBRELLA_K, UMBRELLA_M = 50.0, 1.5
# case: (end A, end B, noise_std, T_A, T_B); an end is (kind, n, d) or (box kind, nsolvent); the start state is end A's
CASES = {
    "mfn_lj_2_1": (("mfn", 2, 1), ("lj", 2, 1), 0.3, 1.0, 1.0),
    "mfn_lj_13_3": (("mfn", 13, 3), ("lj", 13, 3), 0.04, 1.0, 1.0),
    "mfn_lj_64_3": (("mfn", 64, 3), ("lj", 64, 3), 0.015, 1.0, 1.0),
    "lj_mdw_4_2": (("lj", 4, 2), ("mdw", 4, 2), 0.15, 1.0, 1.0),
    "lj_mdw_64_3": (("lj", 64, 3), ("mdw", 64, 3), 0.015, 1.0, 1.0),
    "mdw_mfn_13_3": (("mdw", 13, 3), ("mfn", 13, 3), 0.1, 1.0, 1.0),
    "lj_lj_13_3": (("lj", 13, 3), ("lj", 13, 3), 0.03, 1.0, 2.0),
    "rep_biased_2": (("rep", 2), ("biased", 2), 0.05, 1.0, 1.0),
    "rep_biased_62": (("rep", 62), ("biased", 62), 0.008, 1.0, 1.0),
    "rep_harm_36": (("rep", 36), ("harm", 36), 0.02, 1.0, 1.0),
}


class Interpolated(Energy):
    """c_a e_A + c_b e_B of the reference's energies; a coefficient that is exactly 0 drops its term"""

    def __init__(self, energy_a, energy_b, dim):
        super().__init__(dim)
        self.energy_a, self.energy_b, self.c = energy_a, energy_b, (1.0, 0.0)

    def ends(self, x):
        return self.energy_a.energy(x), self.energy_b.energy(x)

    def _energy(self, x):
        e_a, e_b = self.ends(x)
        c_a, c_b = self.c
        u = c_a * e_a if c_a != 0 else torch.zeros_like(e_a)
        return u + c_b * e_b if c_b != 0 else u


class RecordedProposal(torch.nn.Module):
    """x + noise_std * (the recorded noise of the step), a symmetric proposal"""

    def __init__(self, noise, noise_std):
        super().__init__()
        self.noise, self.noise_std, self.step = noise, noise_std, 0

    def forward(self, state):
        eps = self.noise[self.step]
        self.step += 1
        return state.replace(samples=tuple(x + eps.reshape(x.shape).to(x.dtype) * self.noise_std for x in state.as_dict()["samples"])), 0.0


class RecordedUniforms:
    """stands in for torch.rand_like in metropolis_accept: returns the recorded uniforms of the step and keeps its argument"""

    def __init__(self, uniforms):
        self.uniforms, self.step, self.log_ratio = uniforms, 0, []

    def __call__(self, like):
        self.log_ratio.append(like.detach().clone())
        r = self.uniforms[self.step].to(like.dtype)
        self.step += 1
        return r


def box_parameters(nsolvent, biased=False):
    p = {**RepulsiveParticles.params_default, "nsolvent": nsolvent, "eps": EPS}
    if biased:
        p["dimer_slope"] = p["dimer_slope"] + UMBRELLA_K * (p["dimer_dmid"] - UMBRELLA_M)
        p["dimer_a"] = p["dimer_a"] - UMBRELLA_K / 4
    return p


def make(end, P):
    kind = end[0]
    if kind in ("rep", "biased"):
        return RepulsiveParticles(box_parameters(end[1], kind == "biased"))
    if kind == "harm":
        return HarmonicParticles(spring_constant=SPRING, params=box_parameters(end[1]))
    n, d = end[1:]
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        return LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=False)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in P["mdw_params"])
        return MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)
    return MeanFreeNormalDistribution(n * d, n, std=float(P["mfn_std"]), two_event_dims=False)


def coefficients(t_a, t_b):
    lam = np.array(LAMBDAS, dtype=np.float64)
    return np.stack([(1.0 - lam) / t_a, lam / t_b], axis=1).astype(np.float32).astype(np.float64)


def run(energy, x0, noise, unif, std, table, dtype):
    """the protocol on fixed numbers: final x [B, n d], work [B] (f64), e_a, e_b [B], decisions [12, B], margins [12, B]"""
    x = torch.from_numpy(x0).reshape(B, -1).to(dtype)
    draws = RecordedUniforms(torch.from_numpy(unif))
    proposal = RecordedProposal(torch.from_numpy(noise), std)
    work = torch.zeros(B, dtype=torch.float64)
    original = torch.rand_like
    torch.rand_like = draws
    try:
        for m in range(1, len(table)):
            e_a, e_b = (e[:, 0].double() for e in energy.ends(x))
            d_a, d_b = float(table[m, 0] - table[m - 1, 0]), float(table[m, 1] - table[m - 1, 1])
            work = work + ((d_a * e_a if d_a != 0 else 0.0) + (d_b * e_b if d_b != 0 else 0.0))
            energy.c = (float(table[m, 0]), float(table[m, 1]))
            step = mcmc.MCMCStep(energy, proposal=proposal, target_temperatures=1.0, n_steps=K)
            x = step.forward(iterative.SamplerState(samples=x)).as_dict()["samples"][0]
    finally:
        torch.rand_like = original
    assert draws.step == N_STEPS and proposal.step == N_STEPS and x.dtype == dtype
    log_ratio = torch.stack(draws.log_ratio).double().numpy()
    log_r = np.log(unif.astype(np.float64)) if dtype == torch.float64 else torch.from_numpy(unif).log().double().numpy()
    e_a, e_b = (e[:, 0].detach().numpy() for e in energy.ends(x))
    return x.reshape(B, -1).numpy(), work.numpy(), e_a, e_b, log_ratio >= log_r, np.abs(log_ratio - log_r)


def main():
    P = np.load(os.path.join(HERE, "particles.npz"))
    BOX = np.load(os.path.join(HERE, "box.npz"))
    out = {"seed": np.int64(SEED), "lambdas": np.array(LAMBDAS), "n_steps": np.int64(K), "margin_threshold": np.float64(MARGIN)}
    for key, (end_a, end_b, std, t_a, t_b) in CASES.items():
        x0 = BOX[f"x_{end_a[1]}"] if len(end_a) == 2 else P[f"x_{end_a[1]}_{end_a[2]}"]
        x0 = np.ascontiguousarray(x0).reshape(B, -1)
        nd = x0.shape[1]
        noise, unif = random_numbers(SEED, nd, N_STEPS, B)
        assert noise.dtype == np.float32 and unif.dtype == np.float32
        out[f"noise_sum_{nd}"], out[f"noise_absmax_{nd}"] = np.float64(noise.astype(np.float64).sum()), np.float64(np.abs(noise).max())
        out["unif_sum"], out["unif_absmax"] = np.float64(unif.astype(np.float64).sum()), np.float64(unif.max())
        energy = Interpolated(make(end_a, P), make(end_b, P), nd)
        table = coefficients(t_a, t_b)
        x64, w64, a64, b64, dec64, mar64 = run(energy, x0, noise, unif, std, table, torch.float64)
        x32, w32, a32, b32, dec32, _ = run(energy, x0, noise, unif, std, table, torch.float32)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and a32.dtype == np.float32 and w32.dtype == np.float64
        assert np.isfinite(w64).all() and np.isfinite(x64).all()
        margin = mar64.min(axis=0)
        keep = margin >= MARGIN
        acc = dec64.sum(axis=0).astype(np.int32)
        rate = acc.mean() / N_STEPS
        same = bool((dec32[:, keep] == dec64[:, keep]).all())
        print(f"{key}: std {std}, acceptance {rate:.2f}, kept {int(keep.sum())} / {B}, f32 = f64 decisions on the kept chains: {same}, "
              f"work {w64.mean():.3f} +- {w64.std():.3f}")
        assert keep.mean() >= 0.85, (key, keep.mean())
        assert same, key
        assert 0.2 <= rate <= 0.9, (key, rate)
        kc = keep[:CHAINS]
        err_x = np.abs(x32[:CHAINS][kc] - x64[:CHAINS][kc]).max()
        err_w = np.max(np.abs(w32[keep] - w64[keep]) / (1.0 + np.abs(w64[keep])))
        err_e = max(np.max(np.abs(e32[keep] - e64[keep]) / (1.0 + np.abs(e64[keep]))) for e32, e64 in ((a32, a64), (b32, b64)))
        print(f"    err_x32 {err_x:.3g}, err_w32 {err_w:.3g}, err_e32 {err_e:.3g}")
        k = key + "_"
        out[k + "work64"], out[k + "x64"], out[k + "acc"], out[k + "e_a64"], out[k + "e_b64"] = w64, x64[:CHAINS], acc, a64, b64
        out[k + "margin"], out[k + "keep"] = margin, keep
        out[k + "err_x32"], out[k + "err_w32"], out[k + "err_e32"] = np.float64(err_x), np.float64(err_w), np.float64(err_e)
        out[k + "std"], out[k + "t_a"], out[k + "t_b"] = np.float64(std), np.float64(t_a), np.float64(t_b)
    path = os.path.join(HERE, "anneal.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
