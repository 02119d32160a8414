#!/usr/bin/env python
"""Generate tests/golden/box.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_box_goldens.py

What runs: the UNMODIFIED reference classes ``RepulsiveParticles`` and ``HarmonicParticles`` (distribution/energy/particles.py), and for
the chains ``IterativeSampler`` / ``SamplerState`` / ``MCMCStep`` as in make_mcmc_goldens.py, with the two import shims of
make_goldens.py (``numpy.infty``, nflows_stub).  The fixture holds DATA only.

Cases ``{rep, harm}_{nsolvent}``, nsolvent in {0, 2, 36, 62} (2, 4, 38, 64 particles in 2 dimensions), B = 150.  Parameters:
``params_default`` except eps = 0.7; spring_constant = 150.  Positions ``x_{nsolvent}`` (shared by the kinds): a square lattice, spacing
1.15 (nsolvent = 62: 1.0), jitter of at most 0.15 per coordinate in steps of 1 / 256.  The two small lattices (2 and 4 particles) would
neither reach a wall nor bring a pair within rc that way: they have the spacing 0.95 and are moved by (+2.5, -2.5), so that they straddle
the upper x wall and the lower y wall at +-3 and their neighbours fall on both sides of rc = 0.9.  Per case:

  u64    the reference on x.double()                        u32   the reference on x (f32)
  g64    f64 gradient of u.sum() w.r.t. x (see below)       g_rows   the rows g64 holds (dim > 64: G_ROWS_WIDE of make_particle_goldens.py)
  err_u32 = max_b |u32 - u64| / (1 + |u64|)                 err_g32 = max |g32 - g64| / (1 + max |g64|)
  close  (harm) the fraction of the unmasked pairs with D < rc

rep: g64 / g32 are the reference's autograd; ``rep_36_force64`` is the reference's analytic ``force`` in f64 (rows g_rows; its
``box_force_torch`` reshapes to 76 columns, so it runs for nsolvent = 36 only), asserted equal to -g64 to 1e-10; ``rep_{ns}_surrogate64``
is ``surrogate_energy`` in f64.
harm: the reference takes the root of its [B, n, n] matrix with the zero diagonal, and its autograd gradient is NaN in every entry
(asserted, so that the reason stays on record).  g64 / g32 come from f64 / f32 autograd of ``harmonic_pairs`` below, this script's own
statement of the same energy over the pairs i < j; its f64 energy equals the reference's to 1e-12 relative (asserted).

Asserted: at least 5 % of the coordinates of every case lie outside the box; all energies are finite and below 1e4 in magnitude; for
nsolvent >= 2 the harmonic pairs fall on both sides of rc: at 4 particles 5 % .. 95 % of the unmasked pairs have D < rc; at 38 and 64
particles only lattice neighbours can be that close, a few per cent of ALL pairs at most, so there at least 5 % of the SAMPLES must hold
such a pair (and at most 95 % of the pairs be that close).

Edge cases ``edge_{rep,harm}_*`` (nsolvent = 2, B = 8): samples 0 and 1 have two coincident solvent particles, sample 2 has the dimer
particles 0.3 apart (the (0, 1) mask at work).  u64 / u32 as they come (rep: inf); g64 as above.

Chains ``mc_{kind}_{nsolvent}_*``, nsolvent in {2, 36, 62}: as in make_mcmc_goldens.py -- random numbers of oracle/philox.py (SEED_MC; only
their checksums are stored), a recording proposal, patched ``rand_like``, 48 steps as ``IterativeSampler(stride=3).sample(16)``; x64, rows,
e64, acc, frames64, margin, keep, err_x32, err_e32, std, temps as there; harm_36 at per-chain temperatures alternating 1 and 2.  Asserted:
keep >= 85 %, the f32 run decides like the f64 run on every kept chain, acceptance within 25-80 %.

``meta``: JSON -- constructor signatures and ``params_default`` of both classes.
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

from bgflow.distribution.energy.particles import HarmonicParticles, RepulsiveParticles  # noqa: E402
from bgflow.distribution.sampling import iterative, mcmc  # noqa: E402
from oracle import philox  # noqa: E402

SEED, SEED_MC, B = 20264, 20265, 150
NSOLVENT = (0, 2, 36, 62)
EPS, SPRING = 0.7, 150.0
JITTER = 0.15
G_ROWS_WIDE = np.r_[0:8, 118:150]
N_FRAMES, STRIDE = 16, 3
N_STEPS = N_FRAMES * STRIDE
MARGIN = 1e-3
# (kind, nsolvent): (noise_std, temperature); "alt" = per-chain temperatures alternating 1 and 2
MC_CASES = {
    ("rep", 2): (0.05, 1.0), ("harm", 2): (0.05, 1.0), ("rep", 36): (0.02, 1.0), ("harm", 36): (0.05, "alt"),
    ("rep", 62): (0.008, 1.0), ("harm", 62): (0.02, 1.0),
}


def parameters(nsolvent):
    return {**RepulsiveParticles.params_default, "nsolvent": nsolvent, "eps": EPS}


def make(kind, nsolvent):
    return RepulsiveParticles(parameters(nsolvent)) if kind == "rep" else HarmonicParticles(spring_constant=SPRING, params=parameters(nsolvent))


def lattice(rng, n, batch):
    side = int(np.ceil(np.sqrt(n) - 1e-9))
    pts = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64)
    pts = (pts - pts.mean(0)) * (1.0 if n == 64 else 1.15 if n > 4 else 0.95)
    if n <= 4:
        pts = pts + np.array([2.5, -2.5])
    steps = int(JITTER * 256)
    x = pts[None] + rng.integers(-steps, steps + 1, size=(batch, n, 2)) / 256.0
    return x.astype(np.float32).reshape(batch, 2 * n)


def harmonic_pairs(energy, x):
    """HarmonicParticles._energy over the pairs i < j except (0, 1), the root taken of the kept pairs only: [B]"""
    n, p = energy.nparticles, energy.params
    xp = x.reshape(x.shape[0], n, 2)
    i, j = torch.triu_indices(n, n, offset=1)
    i, j = i[1:], j[1:]
    d2 = (xp[:, i] - xp[:, j]).pow(2).sum(-1)
    close, apart = d2 < p["rc"] ** 2, d2 > 0
    dist = torch.where(apart, torch.where(apart, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    pair = energy.spring_constant * torch.where(close, (dist - p["rc"]) ** 2, torch.zeros_like(d2)).sum(-1)
    return pair + energy.dimer_energy_torch(x) + energy.box_energy_torch(x)


def evaluate(fn, x):
    x = x.clone().requires_grad_(True)
    u = fn(x)
    (g,) = torch.autograd.grad(u.sum(), x)
    return u.detach().numpy().reshape(-1), g.numpy().reshape(x.shape[0], -1)


def energies_and_gradients(kind, energy, xt):
    """u64, u32 of the reference; g64, g32 of the reference (rep) or of harmonic_pairs (harm)"""
    u64, g64 = evaluate(energy.energy, xt.double())
    u32, g32 = evaluate(energy.energy, xt)
    if kind == "harm":
        assert np.isnan(g64).all() and np.isnan(g32).all()          # the reference's sqrt of the zero diagonal
        own64, g64 = evaluate(lambda x: harmonic_pairs(energy, x), xt.double())
        _, g32 = evaluate(lambda x: harmonic_pairs(energy, x), xt)
        fin = np.isfinite(u64)
        assert float(np.max(np.abs(own64[fin] - u64[fin]) / (1.0 + np.abs(u64[fin])))) <= 1e-12
    return u64, u32, g64, g32


def err_u(v, u64):
    return float(np.max(np.abs(v.astype(np.float64) - u64) / (1.0 + np.abs(u64))))


def err_g(v, g64):
    return float(np.max(np.abs(v.astype(np.float64) - g64)) / (1.0 + np.max(np.abs(g64))))


# ---- chains: make_mcmc_goldens.py's fixed random numbers ----------------------------------------------------------------------------
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
    noise = np.stack([philox.sample_field(SEED_MC, s, 0, B, nd, 1).astype(np.float32) for s in range(N_STEPS)])
    unif = np.stack([philox.sample_field(SEED_MC, s, 1, B, 1, 0)[:, 0] for s in range(N_STEPS)])
    assert noise.dtype == np.float32 and unif.dtype == np.float32
    return noise, unif


def temperatures(spec, dtype):
    if spec == "alt":
        return torch.tensor([1.0, 2.0], dtype=dtype).repeat(B // 2)
    return spec


def run(energy, x0, noise, unif, std, temp_spec, dtype):
    """the reference's sampler on fixed numbers: frames [16, B, dim], final x [B, dim], e [B], decisions [48, B], margins [48, B]"""
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


def main():
    rng = np.random.default_rng(SEED)
    out = {"seed": np.int64(SEED), "eps": np.float64(EPS), "spring_constant": np.float64(SPRING)}
    half, rc = RepulsiveParticles.params_default["box_halfsize"], RepulsiveParticles.params_default["rc"]
    for ns in NSOLVENT:
        n = ns + 2
        x = lattice(rng, n, B)
        outside = float((np.abs(x) > half).mean())
        assert outside >= 0.05, (ns, outside)
        out[f"x_{ns}"] = x
        xt = torch.from_numpy(x)
        xp = x.reshape(B, n, 2).astype(np.float64)
        i, j = np.triu_indices(n, 1)
        dist = np.sqrt(((xp[:, i[1:]] - xp[:, j[1:]]) ** 2).sum(-1))                # [B, unmasked pairs]
        rows = G_ROWS_WIDE if 2 * n > 64 else np.arange(B)
        for kind in ("rep", "harm"):
            energy = make(kind, ns)
            u64, u32, g64, g32 = energies_and_gradients(kind, energy, xt)
            assert u64.dtype == np.float64 and u32.dtype == np.float32
            assert np.isfinite(u64).all() and np.abs(u64).max() < 1e4, (kind, ns, np.abs(u64).max())
            key = f"{kind}_{ns}"
            out[key + "_u64"], out[key + "_u32"] = u64, u32
            out[key + "_g64"], out[key + "_g_rows"] = g64[rows], rows.astype(np.int32)
            out[key + "_err_u32"], out[key + "_err_g32"] = np.float64(err_u(u32, u64)), np.float64(err_g(g32[rows], g64[rows]))
            note = ""
            if kind == "rep":
                out[key + "_surrogate64"] = energy.surrogate_energy(xt.double()).numpy().reshape(-1)
                if ns == 36:
                    force = energy.force(xt.double()).numpy()
                    dev = float(np.max(np.abs(force + g64)) / (1.0 + np.max(np.abs(g64))))
                    assert dev <= 1e-10, dev
                    out[key + "_force64"] = force[rows]
                    note = f", |force + g64| {dev:.2g}"
            elif ns >= 2:
                close = dist < rc
                out[key + "_close"] = np.float64(close.mean())
                covered = close.mean() if n <= 4 else close.any(axis=1).mean()
                assert close.mean() <= 0.95 and covered >= 0.05, (ns, close.mean(), covered)
                note = f", pairs with D < rc: {close.mean():.4f} of all, {int(close.sum())} pairs in {int(close.any(axis=1).sum())} samples"
            print(f"{key}: outside {outside:.2f}, |u64| <= {np.abs(u64).max():.4g}, err_u32 {err_u(u32, u64):.3g}, "
                  f"err_g32 {err_g(g32[rows], g64[rows]):.3g}{note}")

    # coincident solvent particles in samples 0 and 1, a close dimer in sample 2
    x = lattice(rng, 4, 8).reshape(8, 4, 2)
    x[0, 3] = x[0, 2]
    x[1, 2] = x[1, 3]
    x[2, 1] = x[2, 0] + np.array([0.3, 0.0], dtype=np.float32)
    x = x.reshape(8, 8)
    xt = torch.from_numpy(x)
    for kind in ("rep", "harm"):
        energy = make(kind, 2)
        u64, u32, g64, g32 = energies_and_gradients(kind, energy, xt)
        key = f"edge_{kind}"
        out[key + "_x"] = x
        out[key + "_u64"], out[key + "_u32"], out[key + "_g64"], out[key + "_g32"] = u64, u32, g64, g32
        fin = np.isfinite(u64)
        out[key + "_err_u32"] = np.float64(err_u(u32[fin], u64[fin]))
        out[key + "_err_g32"] = np.float64(err_g(g32[fin], g64[fin]))
        print(f"{key}: u32[:3] = {u32[:3]}, finite g64 rows: {np.isfinite(g64).all(1)}")

    # chains
    out["seed_mc"], out["n_steps"], out["stride"], out["margin_threshold"] = np.int64(SEED_MC), np.int64(N_STEPS), np.int64(STRIDE), np.float64(MARGIN)
    numbers = {}
    for (kind, ns), (std, temp_spec) in MC_CASES.items():
        nd = 2 * (ns + 2)
        if nd not in numbers:
            numbers[nd] = random_numbers(nd)
            noise, unif = numbers[nd]
            out[f"noise_sum_{ns}"], out[f"noise_absmax_{ns}"] = np.float64(noise.astype(np.float64).sum()), np.float64(np.abs(noise).max())
            out["unif_sum"], out["unif_absmax"] = np.float64(unif.astype(np.float64).sum()), np.float64(unif.max())
        noise, unif = numbers[nd]
        x0 = out[f"x_{ns}"]
        energy = make(kind, ns)
        f64, x64, e64, dec64, mar64 = run(energy, x0, noise, unif, std, temp_spec, torch.float64)
        f32, x32, e32, dec32, _ = run(energy, x0, noise, unif, std, temp_spec, torch.float32)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and np.isfinite(e64).all()
        margin = mar64.min(axis=0)
        keep = margin >= MARGIN
        acc = dec64.sum(axis=0).astype(np.int32)
        rate = acc.mean() / N_STEPS
        print(f"mc_{kind}_{ns}: acceptance {rate:.2f}, kept {int(keep.sum())} / {B}")
        assert keep.mean() >= 0.85, (kind, ns, keep.mean())
        assert (dec32[:, keep] == dec64[:, keep]).all(), (kind, ns)
        assert 0.25 <= rate <= 0.80, (kind, ns, rate)
        rows = G_ROWS_WIDE if nd > 64 else np.arange(B)
        chains = 8
        kr, kc = keep[rows], keep[:chains]
        err_x = max(np.abs(x32[rows][kr] - x64[rows][kr]).max(), np.abs(f32[:, :chains][:, kc] - f64[:, :chains][:, kc]).max())
        err_e = np.max(np.abs(e32[keep] - e64[keep]) / (1.0 + np.abs(e64[keep])))
        key = f"mc_{kind}_{ns}_"
        out[key + "x64"], out[key + "rows"], out[key + "e64"] = x64[rows], rows.astype(np.int32), e64
        out[key + "frames64"], out[key + "acc"], out[key + "margin"], out[key + "keep"] = f64[:, :chains], acc, margin, keep
        out[key + "err_x32"], out[key + "err_e32"] = np.float64(err_x), np.float64(err_e)
        out[key + "std"] = np.float64(std)
        out[key + "temps"] = temperatures(temp_spec, torch.float64).numpy() if temp_spec == "alt" else np.float64(temp_spec)
        print(f"    f32 = f64 decisions on all chains: {bool((dec32 == dec64).all())}, err_x32 {err_x:.3g}, err_e32 {err_e:.3g}")

    meta = {"params_default": dict(RepulsiveParticles.params_default),
            "harmonic_params_default": dict(HarmonicParticles.params_default)}
    for cls in (RepulsiveParticles, HarmonicParticles):
        sig = inspect.signature(cls.__init__)
        meta[cls.__name__] = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in list(sig.parameters.values())[1:]]
    out["meta"] = np.array(json.dumps(meta))

    path = os.path.join(HERE, "box.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
