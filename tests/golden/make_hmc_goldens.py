#!/usr/bin/env python
"""Generate tests/golden/hmc.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_hmc_goldens.py

What runs: the UNMODIFIED reference classes ``IterativeSampler`` / ``SamplerState`` (distribution/sampling/iterative.py), ``MCMCStep`` and
``metropolis_accept`` (sampling/mcmc.py) on the reference's ``LennardJonesPotential``, ``MultiDoubleWellPotential``,
``MeanFreeNormalDistribution``, ``RepulsiveParticles`` and ``HarmonicParticles``, with the two import shims of make_goldens.py.  The
reference has no Hamiltonian proposal outside its OpenMM integrators, so the proposal is a small module of THIS script
(``RecordedHamiltonian``: ``MCMCStep`` takes any proposal) -- the leapfrog rule of ``bgflow_amd.HamiltonianProposal`` on the reference's
forces with recorded normals; ``torch.rand_like`` is patched for the acceptance draw, as in make_mcmc_goldens.py.  The fixture holds DATA
only.

Forces: the pair kinds use the reference's ``energy.force``.  The particle box cannot: the reference's analytic ``force`` reshapes to 76
columns (36 solvent particles only) and belongs to the repulsive pair term, and the autograd gradient of its ``HarmonicParticles`` is NaN
(make_box_goldens.py).  So ``rep`` uses minus the autograd gradient of the reference's ``energy``, and ``harm`` minus that of
``harmonic_pairs``, make_box_goldens.py's statement of the same energy over the pairs i < j.

Inputs: the start states and parameters of particles.npz (pair kinds, ``two_event_dims=False``) and box.npz (``x_{nsolvent}``), B = 150.
Random numbers of step s, as in make_mcmc_goldens.py / make_box_goldens.py (regenerated identically by the tests from oracle/philox.py;
only checksums are stored):

    xi_s = oracle.philox.sample_field(seed, s, 0, 150, n d, 1).astype(float32)        r_s = sample_field(seed, s, 1, 150, 1, 0)[:, 0]

with seed = SEED for the pair kinds and SEED_BOX for the box.

Cases ``{kind}_{n}_{d}``, kind in {lj (oscillator), mdw, mfn} x (n, d) in {(2,1), (4,2), (13,3), (64,3)}, and ``{rep, harm}_{nsolvent}``,
nsolvent in {2, 62}: 12 steps as ``IterativeSampler(stride=2).sample(6)`` of an ``MCMCStep(n_steps=1)``; 5 leapfrog steps, (2, 1): 1 (the
MALA limit); mass 1, mfn_13_3: 2.5; temperature 1, mdw_13_3: per-chain temperatures alternating 1 and 2 (the case of mcmc.npz with a
tensor).  The step sizes are in CASES.  Per case, from the f64 run (start state and normals converted to f64):

  x64      final state, [rows, n d]; rows = all 150, for n d > 64 the rows G_ROWS_WIDE of make_particle_goldens.py (``rows``)
  e64      final energies [150]                     acc      accepted steps per chain [150] (int32)
  frames64 the 6 recorded states of the first 8 chains, [6, 8, n d]
  margin   min over the steps of |min(0, log ratio) - log r| per chain [150]
  keep     margin >= 1e-3: below that an f32 evaluation may legitimately decide otherwise, and the chains part ways
  err_x32  max |x32 - x64| over the kept chains of x64 and frames64, x32 this script's own f32 run of the same chains
  err_e32  max |e32 - e64| / (1 + |e64|) over the kept chains
  step_size, n_leapfrog, mass, temps   the settings

Asserted here, as conditions of the fixture: keep covers >= 85 % of every case; the f64 acceptance rate over the 12 steps lies in
[0.3, 0.95], so both branches of the accept are exercised in every case; the f32 run takes the same decision as the f64 run at every step
of every kept chain, so that err_x32 / err_e32 measure rounding and not chains that parted ways.
"""
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
from bgflow.distribution.energy.particles import HarmonicParticles, RepulsiveParticles  # noqa: E402
from bgflow.distribution.normal import MeanFreeNormalDistribution  # noqa: E402
from bgflow.distribution.sampling import iterative, mcmc  # noqa: E402
from oracle import philox  # noqa: E402

SEED, SEED_BOX, B = 20262, 20265, 150
N_FRAMES, STRIDE = 6, 2
N_STEPS = N_FRAMES * STRIDE
G_ROWS_WIDE = np.r_[0:8, 118:150]
MARGIN = 1e-3
EPS, SPRING = 0.7, 150.0          # the box parameters of make_box_goldens.py
# case: (step_size, n_leapfrog, mass, temperature); "alt" = per-chain temperatures alternating 1 and 2
CASES = {
    ("lj", 2, 1): (0.3, 1, 1.0, 1.0), ("lj", 4, 2): (0.1, 5, 1.0, 1.0), ("lj", 13, 3): (0.06, 5, 1.0, 1.0), ("lj", 64, 3): (0.03, 5, 1.0, 1.0),
    ("mdw", 2, 1): (0.2, 1, 1.0, 1.0), ("mdw", 4, 2): (0.15, 5, 1.0, 1.0), ("mdw", 13, 3): (0.1, 5, 1.0, "alt"), ("mdw", 64, 3): (0.054, 5, 1.0, 1.0),
    ("mfn", 2, 1): (1.2, 1, 1.0, 1.0), ("mfn", 4, 2): (0.9, 5, 1.0, 1.0), ("mfn", 13, 3): (1.2, 5, 2.5, 1.0), ("mfn", 64, 3): (0.6, 5, 1.0, 1.0),
    ("rep", 2): (0.03, 5, 1.0, 1.0), ("harm", 2): (0.04, 5, 1.0, 1.0), ("rep", 62): (0.01, 5, 1.0, 1.0), ("harm", 62): (0.03, 5, 1.0, 1.0),
}


class RecordedHamiltonian(torch.nn.Module):
    """the leapfrog proposal on recorded normals: p0 = sqrt(m) xi, a half kick, n_leapfrog drifts with kicks between them and a half
    kick at the end, in the potential force(x) / T; delta_log_prob = K(p) - K(p0), K = |p|^2 / (2 m)"""

    def __init__(self, force, noise, step_size, n_leapfrog, mass, temperature):
        super().__init__()
        self.force, self.noise, self.step = force, noise, 0
        self.h, self.n_leapfrog, self.m, self.temperature = step_size, n_leapfrog, mass, temperature

    def scaled_force(self, x):
        t = self.temperature
        if torch.is_tensor(t):
            t = t.to(x.dtype).reshape(-1, 1)
        return self.force(x.detach().clone()).detach() / t

    def forward(self, state):
        (x,) = state.as_dict()["samples"]
        x = x.detach()
        xi = self.noise[self.step].reshape(x.shape).to(x.dtype)
        self.step += 1
        h, m = self.h, self.m
        p0 = m ** 0.5 * xi
        p = p0 + (h / 2) * self.scaled_force(x)
        for k in range(self.n_leapfrog):
            x = x + (h / m) * p
            p = p + (h if k + 1 < self.n_leapfrog else h / 2) * self.scaled_force(x)
        kinetic = [(q * q).sum(dim=-1) / (2 * m) for q in (p, p0)]
        return state.replace(samples=(x,)), kinetic[0] - kinetic[1]


class RecordedUniforms:
    """stands in for torch.rand_like in metropolis_accept: returns the recorded uniforms of the step and keeps its argument"""

    def __init__(self, uniforms):
        self.uniforms, self.step, self.log_ratio = uniforms, 0, []

    def __call__(self, like):
        self.log_ratio.append(like.detach().clone())
        r = self.uniforms[self.step].to(like.dtype)
        self.step += 1
        return r


def random_numbers(seed, nd):
    noise = np.stack([philox.sample_field(seed, s, 0, B, nd, 1).astype(np.float32) for s in range(N_STEPS)])
    unif = np.stack([philox.sample_field(seed, s, 1, B, 1, 0)[:, 0] for s in range(N_STEPS)])
    assert noise.dtype == np.float32 and unif.dtype == np.float32
    return noise, unif


def temperatures(spec, dtype):
    if spec == "alt":
        return torch.tensor([1.0, 2.0], dtype=dtype).repeat(B // 2)
    return spec


def harmonic_pairs(energy, x):
    """HarmonicParticles._energy over the pairs i < j except (0, 1), the root taken of the kept pairs only: [B] (make_box_goldens.py)"""
    n, p = energy.nparticles, energy.params
    xp = x.reshape(x.shape[0], n, 2)
    i, j = torch.triu_indices(n, n, offset=1)
    i, j = i[1:], j[1:]
    d2 = (xp[:, i] - xp[:, j]).pow(2).sum(-1)
    close, apart = d2 < p["rc"] ** 2, d2 > 0
    dist = torch.where(apart, torch.where(apart, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    pair = energy.spring_constant * torch.where(close, (dist - p["rc"]) ** 2, torch.zeros_like(d2)).sum(-1)
    return pair + energy.dimer_energy_torch(x) + energy.box_energy_torch(x)


def minus_gradient(fn):
    def force(x):
        with torch.enable_grad():
            x = x.requires_grad_(True)
            return -torch.autograd.grad(fn(x).sum(), x)[0]
    return force


def make(case, P):
    """(the reference's energy, the force of the proposal, the start state [B, n d], the seed)"""
    kind = case[0]
    if kind in ("rep", "harm"):
        ns = case[1]
        params = {**RepulsiveParticles.params_default, "nsolvent": ns, "eps": EPS}
        x0 = np.load(os.path.join(HERE, "box.npz"))[f"x_{ns}"]
        if kind == "rep":
            energy = RepulsiveParticles(params)
            return energy, minus_gradient(energy.energy), x0, SEED_BOX
        energy = HarmonicParticles(spring_constant=SPRING, params=params)
        return energy, minus_gradient(lambda x: harmonic_pairs(energy, x)), x0, SEED_BOX
    n, d = case[1:]
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        energy = LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=False)
    elif kind == "mdw":
        a, b, c, off = (float(v) for v in P["mdw_params"])
        energy = MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)
    else:
        energy = MeanFreeNormalDistribution(n * d, n, std=float(P["mfn_std"]), two_event_dims=False)
    return energy, energy.force, P[f"x_{n}_{d}"], SEED


def run(energy, force, x0, noise, unif, settings, dtype):
    """the reference's sampler on fixed numbers: frames [6, B, n d], final x [B, n d], e [B], decisions [12, B], margins [12, B]"""
    h, n_leapfrog, mass, temp_spec = settings
    x = torch.from_numpy(x0).reshape(B, -1).to(dtype)
    draws = RecordedUniforms(torch.from_numpy(unif))
    temps = temperatures(temp_spec, dtype)
    proposal = RecordedHamiltonian(force, torch.from_numpy(noise), h, n_leapfrog, mass, temps)
    step = mcmc.MCMCStep(energy, proposal=proposal, target_temperatures=temps)
    original = torch.rand_like
    torch.rand_like = draws
    try:
        sampler = iterative.IterativeSampler(iterative.SamplerState(samples=x), [step], stride=STRIDE)
        frames = sampler.sample(N_FRAMES)
    finally:
        torch.rand_like = original
    assert draws.step == N_STEPS and proposal.step == N_STEPS and frames.dtype == dtype
    final = sampler.state.as_dict()
    log_ratio = torch.stack(draws.log_ratio).double().numpy()
    log_r = np.log(unif.astype(np.float64)) if dtype == torch.float64 else torch.from_numpy(unif).log().double().numpy()
    e = energy.energy(final["samples"][0])[:, 0]
    return (frames.reshape(N_FRAMES, B, -1).numpy(), final["samples"][0].reshape(B, -1).numpy(), e.detach().numpy(),
            log_ratio >= log_r, np.abs(log_ratio - log_r))


def main():
    P = np.load(os.path.join(HERE, "particles.npz"))
    out = {"seed": np.int64(SEED), "seed_box": np.int64(SEED_BOX), "n_steps": np.int64(N_STEPS), "stride": np.int64(STRIDE),
           "margin_threshold": np.float64(MARGIN)}
    numbers = {}
    for case, settings in CASES.items():
        energy, force, x0, seed = make(case, P)
        x0 = np.ascontiguousarray(x0).reshape(B, -1)
        nd = x0.shape[1]
        key = "_".join(str(v) for v in case) + "_"
        if (seed, nd) not in numbers:
            numbers[seed, nd] = random_numbers(seed, nd)
            noise, unif = numbers[seed, nd]
            tag = f"{'box_' if seed == SEED_BOX else ''}{nd}"
            out[f"noise_sum_{tag}"], out[f"noise_absmax_{tag}"] = np.float64(noise.astype(np.float64).sum()), np.float64(np.abs(noise).max())
            out[f"unif_sum_{tag}"], out[f"unif_absmax_{tag}"] = np.float64(unif.astype(np.float64).sum()), np.float64(unif.max())
        noise, unif = numbers[seed, nd]
        f64, x64, e64, dec64, mar64 = run(energy, force, x0, noise, unif, settings, torch.float64)
        f32, x32, e32, dec32, _ = run(energy, force, x0, noise, unif, settings, torch.float32)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and np.isfinite(e64).all() and np.isfinite(x64).all()
        margin = mar64.min(axis=0)
        keep = margin >= MARGIN
        acc = dec64.sum(axis=0).astype(np.int32)
        rate = acc.mean() / N_STEPS
        same = bool((dec32[:, keep] == dec64[:, keep]).all())
        print(f"{key[:-1]}: h {settings[0]}, acceptance {rate:.2f}, kept {int(keep.sum())} / {B}, f32 = f64 decisions on the kept chains: {same}")
        assert keep.mean() >= 0.85, (case, keep.mean())
        assert 0.3 <= rate <= 0.95, (case, rate)
        assert same, case               # else err_x32 / err_e32 would measure chains that parted ways, not rounding
        rows = G_ROWS_WIDE if nd > 64 else np.arange(B)
        chains = 8
        kr, kc = keep[rows], keep[:chains]
        err_x = max(np.abs(x32[rows][kr] - x64[rows][kr]).max(), np.abs(f32[:, :chains][:, kc] - f64[:, :chains][:, kc]).max())
        err_e = np.max(np.abs(e32[keep] - e64[keep]) / (1.0 + np.abs(e64[keep])))
        out[key + "x64"], out[key + "rows"], out[key + "e64"] = x64[rows], rows.astype(np.int32), e64
        out[key + "frames64"], out[key + "acc"], out[key + "margin"], out[key + "keep"] = f64[:, :chains], acc, margin, keep
        out[key + "err_x32"], out[key + "err_e32"] = np.float64(err_x), np.float64(err_e)
        out[key + "step_size"], out[key + "n_leapfrog"], out[key + "mass"] = np.float64(settings[0]), np.int64(settings[1]), np.float64(settings[2])
        out[key + "temps"] = temperatures(settings[3], torch.float64).numpy() if settings[3] == "alt" else np.float64(settings[3])
        print(f"    err_x32 {err_x:.3g}, err_e32 {err_e:.3g}")
    path = os.path.join(HERE, "hmc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
