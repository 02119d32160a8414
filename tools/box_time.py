"""Time the particle box (``RepulsiveParticles`` / ``HarmonicParticles``, 38 particles, the reference's ``params_default``):
energy forward and forward + backward at 2^18 samples on bgk_box_energy / _backward against the class's own torch formulas (``_energy``,
the pair sums over i < j), and 1000 Metropolis steps (Gaussian proposal) at 4096 and 65536 chains -- (a) the fused launches of
bgk_box_mcmc, (b) the general path with the energy kernel per step, (c) the general path over the torch formulas.  HIP-event timed,
alternated, median of the repetitions; prints the tables of DESIGN.md's "Particle box".

    python tools/box_time.py [--reps 5] [--steps 1000] [--batch 262144]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import sampling  # noqa: E402

from mcmc_time import TorchFormulas, lattice, timed  # noqa: E402


def fwd_bwd(fn, x):
    xg = x.detach().requires_grad_(True)
    fn(xg).sum().backward()
    return xg.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1 << 18)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nd = 38, 76
    systems = (("repulsive", lambda: bg.RepulsiveParticles(), 0.02), ("harmonic", lambda: bg.HarmonicParticles(), 0.05))
    print(f"{torch.cuda.get_device_name(0)}; 38 particles; median of {args.reps} (ms)")
    print(f"| system | samples | forward, kernel | forward, torch | forward + backward, kernel | forward + backward, torch | force, kernel |")
    print("|---|---|---|---|---|---|---|")
    for label, build, _ in systems:
        torch.manual_seed(0)
        energy = build().to(dev)
        x = lattice(n, 2, 1.0, args.batch, 0.05, dev)
        with torch.no_grad():
            err = float(((energy.energy(x[:4096]) - energy._energy(x[:4096])).abs() / (1 + energy._energy(x[:4096]).abs())).max())
        assert err < 1e-5, err
        runs = {"fk": lambda: energy.energy(x), "ft": lambda: energy._energy(x), "bk": lambda: fwd_bwd(energy.energy, x),
                "bt": lambda: fwd_bwd(energy._energy, x), "force": lambda: energy.force(x)}
        times = timed(runs, args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"<!-- {label}: min .. max " + ", ".join(f"({k}) {min(v):.3f} .. {max(v):.3f}" for k, v in times.items()) + " -->")
        print(f"| {label} | {args.batch} | {med['fk']:.3f} | {med['ft']:.2f} | {med['bk']:.3f} | {med['bt']:.2f} | {med['force']:.3f} |")
    steps = args.steps
    print(f"{steps} Metropolis steps; launches of at most {sampling.MCMC_MAX_STEPS_PER_LAUNCH} steps")
    print("| system | chains | (a) fused | (b) general, energy kernel | (c) general, torch formulas | (a) us per step | acceptance | (a) grid x block, rows per tile, dynamic LDS |")
    print("|---|---|---|---|---|---|---|---|")
    for label, build, std in systems:
        for B in (4096, 65536):
            torch.manual_seed(0)
            energy = build().to(dev)
            formulas = TorchFormulas(energy, nd).to(dev)
            x = lattice(n, 2, 1.0, B, 0.05, dev)
            fused = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=steps)
            general = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=steps)
            general.fused = False
            chain = bg.MCMCStep(formulas, proposal=bg.GaussianProposal(std), n_steps=steps)
            state = bg.SamplerState(samples=x)
            assert fused._fused_setup(state) is not None and general._fused_setup(state) is None and chain._fused_setup(state) is None
            with torch.no_grad():
                times = timed({"a": lambda: fused(state), "b": lambda: general(state), "c": lambda: chain(state)}, min(args.reps, 3))
            med = {k: statistics.median(v) for k, v in times.items()}
            rate = float(fused.n_accepted.float().mean()) / fused.n_proposed
            S = nd | 1
            rows = sampling.mcmc_tile_rows(nd)
            tiles = (B + rows - 1) // rows
            cfg = f"{min(tiles, 4096)} x 64, {rows}, {(((rows * S + 31) & ~31) + rows * S) * 4} B"
            print(f"<!-- {label} {B}: min .. max " + ", ".join(f"({k}) {min(v):.2f} .. {max(v):.2f}" for k, v in times.items()) + " -->")
            print(f"| {label} | {B} | {med['a']:.2f} | {med['b']:.0f} | {med['c']:.0f} | {med['a'] / steps * 1e3:.2f} | {rate:.2f} | {cfg} |")


if __name__ == "__main__":
    main()
