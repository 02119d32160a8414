#!/usr/bin/env python
"""Generate tests/golden/mcmc.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_mcmc_goldens.py

What runs: the UNMODIFIED reference classes ``IterativeSampler`` / ``SamplerState`` (distribution/sampling/iterative.py) and ``MCMCStep``
(sampling/mcmc.py) on the reference's ``LennardJonesPotential``, ``MultiDoubleWellPotential`` and ``MeanFreeNormalDistribution``, with the
two import shims of make_goldens.py.  The random numbers are FIXED: the proposal is a small module of this script that adds recorded
noise (``MCMCStep`` takes any proposal), and ``torch.rand_like`` is patched for the acceptance draw (its argument there is the log
acceptance ratio min(0, -du), which the patch records).  The fixture holds DATA only.

Inputs: the start states ``x_{n}_{d}`` of particles.npz (B = 150) and its parameters (LJ eps 0.7, rm 1.3, oscillator 0.5; MDW a 0.9,
b -4, c 0.1, offset 4; mean-free normal std 0.8), all with ``two_event_dims=False``: the reference's step selects
with ``accept[..., None]``, i.e. on samples [B, n d].  Random numbers of step s (the same for every case of a shape; regenerated identically
by the tests from oracle/philox.py, only ``noise_sum_{n}_{d}`` / ``noise_absmax_{n}_{d}`` / ``unif_sum`` / ``unif_absmax`` are stored):

    noise_s = oracle.philox.sample_field(SEED, s, 0, 150, n d, 1).astype(float32)        r_s = sample_field(SEED, s, 1, 150, 1, 0)[:, 0]

Cases ``{kind}_{n}_{d}``: kind in {lj (oscillator), mdw, mfn} x (n, d) in {(2,1), (4,2), (13,3), (64,3)}; 48 steps as
``IterativeSampler(stride=3).sample(16)`` of an ``MCMCStep(n_steps=1)``; ``noise_std`` and the temperature per case in CASES (chosen for
25-80 % acceptance, asserted); mdw_13_3 runs at per-chain temperatures alternating 1 and 2.  Per case, from the f64 run (start state and
noise converted to f64):

  x64      final state, [rows, n d]; rows = all 150, for n d > 64 the rows G_ROWS_WIDE of make_particle_goldens.py (``rows``)
  e64      final energies [150]                     acc      accepted steps per chain [150] (int32)
  frames64 the 16 recorded states of the first 8 chains, [16, 8, n d]
  margin   min over the steps of |min(0, -du) - log r| per chain [150]
  keep     margin >= 1e-3: below that an f32 evaluation may legitimately decide otherwise, and the chains part ways
  err_x32  max |x32 - x64| over the kept chains of x64 and frames64, x32 the reference's own f32 run of the same chains
  err_e32  max |e32 - e64| / (1 + |e64|) over the kept chains
  std, temps   the settings

Asserted here: keep covers >= 85 % of every case; the reference's f32 run takes the same decision as its f64 run at every step of
every kept chain; the acceptance rate of every case is within 25-80 %.

``meta``: JSON -- constructor / function signatures (parameter names and defaults; callables by name) of the sampling classes.
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
from bgflow.distribution.sampling import iterative, mcmc, _iterative_helpers  # noqa: E402
from oracle import philox  # noqa: E402

SEED, B = 20262, 150
N_FRAMES, STRIDE = 16, 3
N_STEPS = N_FRAMES * STRIDE
G_ROWS_WIDE = np.r_[0:8, 118:150]
MARGIN = 1e-3
# (kind, n, d): (noise_std, temperature); "alt" = per-chain temperatures alternating 1 and 2
CASES = {
    ("lj", 2, 1): (0.2, 1.0), ("lj", 4, 2): (0.1, 1.0), ("lj", 13, 3): (0.03, 1.0), ("lj", 64, 3): (0.015, 1.0),
    ("mdw", 2, 1): (0.3, 1.0), ("mdw", 4, 2): (0.3, 1.0), ("mdw", 13, 3): (0.1, "alt"), ("mdw", 64, 3): (0.02, 2.0),
    ("mfn", 2, 1): (1.0, 1.0), ("mfn", 4, 2): (0.4, 1.0), ("mfn", 13, 3): (0.2, 1.0), ("mfn", 64, 3): (0.08, 1.0),
}


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


def random_numbers(nd):
    noise = np.stack([philox.sample_field(SEED, s, 0, B, nd, 1).astype(np.float32) for s in range(N_STEPS)])
    unif = np.stack([philox.sample_field(SEED, s, 1, B, 1, 0)[:, 0] for s in range(N_STEPS)])
    assert noise.dtype == np.float32 and unif.dtype == np.float32
    return noise, unif


def temperatures(spec, dtype):
    if spec == "alt":
        return torch.tensor([1.0, 2.0], dtype=dtype).repeat(B // 2)
    return spec


def make(kind, n, d, P):
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        return LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=False)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in P["mdw_params"])
        return MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)
    return MeanFreeNormalDistribution(n * d, n, std=float(P["mfn_std"]), two_event_dims=False)


def run(energy, x0, noise, unif, std, temp_spec, dtype):
    """the reference's sampler on fixed numbers: frames [16, B, n d], final x [B, n d], e [B], decisions [48, B], margins [48, B]"""
    x = torch.from_numpy(x0).reshape(B, -1).to(dtype)
    draws = RecordedUniforms(torch.from_numpy(unif))
    step = mcmc.MCMCStep(energy, proposal=RecordedProposal(torch.from_numpy(noise), std), target_temperatures=temperatures(temp_spec, dtype))
    original = torch.rand_like
    torch.rand_like = draws
    try:
        sampler = iterative.IterativeSampler(iterative.SamplerState(samples=x), [step], stride=STRIDE)
        frames = sampler.sample(N_FRAMES)
    finally:
        torch.rand_like = original
    assert draws.step == N_STEPS and frames.dtype == dtype
    final = sampler.state.as_dict()
    log_ratio = torch.stack(draws.log_ratio).double().numpy()
    log_r = np.log(unif.astype(np.float64)) if dtype == torch.float64 else torch.from_numpy(unif).log().double().numpy()
    e = energy.energy(final["samples"][0])[:, 0]
    return (frames.reshape(N_FRAMES, B, -1).numpy(), final["samples"][0].reshape(B, -1).numpy(), e.detach().numpy(),
            log_ratio >= log_r, np.abs(log_ratio - log_r))


def signature(fn):
    out = []
    for p in list(inspect.signature(fn).parameters.values()):
        if p.name == "self":
            continue
        d = p.default
        if d is inspect.Parameter.empty:
            d = "<required>" if p.kind is p.POSITIONAL_OR_KEYWORD else f"<{p.kind.name}>"
        elif isinstance(d, torch.nn.Module):
            d = f"{type(d).__name__}({getattr(d, '_noise_std', '')})"
        elif callable(d):
            d = f"<callable {d.__name__}>"
        elif isinstance(d, dict):
            d = dict(d)
        out.append([p.name, d])
    return out


def main():
    P = np.load(os.path.join(HERE, "particles.npz"))
    out = {"seed": np.int64(SEED), "n_steps": np.int64(N_STEPS), "stride": np.int64(STRIDE), "margin_threshold": np.float64(MARGIN)}
    numbers = {}
    for (kind, n, d), (std, temp_spec) in CASES.items():
        nd = n * d
        if nd not in numbers:
            numbers[nd] = random_numbers(nd)
            noise, unif = numbers[nd]
            out[f"noise_sum_{n}_{d}"], out[f"noise_absmax_{n}_{d}"] = np.float64(noise.astype(np.float64).sum()), np.float64(np.abs(noise).max())
            out["unif_sum"], out["unif_absmax"] = np.float64(unif.astype(np.float64).sum()), np.float64(unif.max())
        noise, unif = numbers[nd]
        x0 = P[f"x_{n}_{d}"]
        energy = make(kind, n, d, P)
        f64, x64, e64, dec64, mar64 = run(energy, x0, noise, unif, std, temp_spec, torch.float64)
        f32, x32, e32, dec32, _ = run(energy, x0, noise, unif, std, temp_spec, torch.float32)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and np.isfinite(e64).all()
        margin = mar64.min(axis=0)
        keep = margin >= MARGIN
        acc = dec64.sum(axis=0).astype(np.int32)
        rate = acc.mean() / N_STEPS
        assert keep.mean() >= 0.85, (kind, n, d, keep.mean())
        assert (dec32[:, keep] == dec64[:, keep]).all(), (kind, n, d)
        assert 0.25 <= rate <= 0.80, (kind, n, d, rate)
        rows = G_ROWS_WIDE if nd > 64 else np.arange(B)
        chains = 8
        kr, kc = keep[rows], keep[:chains]
        err_x = max(np.abs(x32[rows][kr] - x64[rows][kr]).max(), np.abs(f32[:, :chains][:, kc] - f64[:, :chains][:, kc]).max())
        err_e = np.max(np.abs(e32[keep] - e64[keep]) / (1.0 + np.abs(e64[keep])))
        key = f"{kind}_{n}_{d}_"
        out[key + "x64"], out[key + "rows"], out[key + "e64"] = x64[rows], rows.astype(np.int32), e64
        out[key + "frames64"], out[key + "acc"], out[key + "margin"], out[key + "keep"] = f64[:, :chains], acc, margin, keep
        out[key + "err_x32"], out[key + "err_e32"] = np.float64(err_x), np.float64(err_e)
        out[key + "std"] = np.float64(std)
        out[key + "temps"] = temperatures(temp_spec, torch.float64).numpy() if temp_spec == "alt" else np.float64(temp_spec)
        print(f"{key[:-1]}: acceptance {rate:.2f}, kept {int(keep.sum())} / {B}, f32 = f64 decisions on all chains: "
              f"{bool((dec32 == dec64).all())}, err_x32 {err_x:.3g}, err_e32 {err_e:.3g}")

    meta = {
        "SamplerState": signature(iterative.SamplerState.__init__), "SamplerStep": signature(iterative.SamplerStep.__init__),
        "IterativeSampler": signature(iterative.IterativeSampler.__init__), "GaussianProposal": signature(mcmc.GaussianProposal.__init__),
        "LatentProposal": signature(mcmc.LatentProposal.__init__), "MCMCStep": signature(mcmc.MCMCStep.__init__),
        "GaussianMCMCSampler": signature(mcmc.GaussianMCMCSampler.__init__), "metropolis_accept": signature(mcmc.metropolis_accept),
        "evaluate_energy_force": signature(_iterative_helpers.AbstractSamplerState.evaluate_energy_force),
        "state_fields": [[f.name, f.default] for f in __import__("dataclasses").fields(iterative._SamplerStateData) if f.name != "samples"],
    }
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "mcmc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
