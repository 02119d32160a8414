"""Time Metropolis sampling (Gaussian proposal, 1000 steps) of LJ13 and DW4 at 4096 and 65536 chains: (a) the fused launches of
bgk_pair_mcmc (``MCMCStep.forward``, split at ``MCMC_MAX_STEPS_PER_LAUNCH``), (b) the general path -- the reference's step in torch ops
with the energy from bgk_pair_energy, one step at a time, (c) the general path over the class's torch formulas ``_energy`` (the
reference's op chain on the same GPU).  HIP-event timed, alternated, median of the repetitions; prints the table of DESIGN.md's
"Metropolis chains".  The last line times ONE launch at the widest shape of the envelope (Lennard-Jones, n = 64, d = 3, 2^16 chains):
the measured basis of ``MCMC_MAX_STEPS_PER_LAUNCH``.

    python tools/mcmc_time.py [--reps 3] [--steps 1000]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import sampling  # noqa: E402
from bgflow_amd.distributions import _kernel_plan  # noqa: E402


class TorchFormulas(bg.Energy):
    """the target's own torch formulas, whatever the input: the reference's op chain"""

    def __init__(self, inner, dim):
        super().__init__(dim)
        self.inner = inner

    def _energy(self, x):
        return self.inner._energy(x)


def timed(runs, reps):
    """{name: [ms, ...]}: every run warmed up once, then ``reps`` rounds that alternate the runs"""
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def lattice(n, d, spacing, batch, jitter, dev):
    side = int(round(n ** (1.0 / d) + 0.499999))
    pts = torch.stack(torch.meshgrid(*[torch.arange(float(side))] * d, indexing="ij"), -1).reshape(-1, d)[:n]
    pts = (pts - pts.mean(0)) * spacing
    return (pts.reshape(1, -1) + jitter * torch.randn(batch, n * d)).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--cap-steps", type=int, default=64, help="steps of the single launch at the widest shape")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    steps = args.steps
    print(f"{torch.cuda.get_device_name(0)}; {steps} Metropolis steps; median of {args.reps} (ms); launches of at most "
          f"{sampling.MCMC_MAX_STEPS_PER_LAUNCH} steps")
    print("| system | chains | (a) fused | (b) general, energy kernel | (c) general, torch formulas | (a) us per step | acceptance | (a) grid x block, rows per tile, dynamic LDS |")
    print("|---|---|---|---|---|---|---|---|")
    systems = (("LJ13", lambda: bg.LennardJonesPotential(39, 13, eps=1.0, rm=1.0, two_event_dims=False), 13, 3, 1.1, 0.02, 0.03),
               ("DW4", lambda: bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.0, 4.0, two_event_dims=False), 4, 2, 4.0, 0.3, 0.3))
    for label, build, n, d, spacing, jitter, std in systems:
        for B in (4096, 65536):
            torch.manual_seed(0)
            energy = build().to(dev)
            formulas = TorchFormulas(energy, n * d).to(dev)
            x = lattice(n, d, spacing, B, jitter, dev)
            fused = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=steps)
            general = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=steps)
            general.fused = False
            chain = bg.MCMCStep(formulas, proposal=bg.GaussianProposal(std), n_steps=steps)
            state = bg.SamplerState(samples=x)
            assert fused._fused_setup(state) is not None and general._fused_setup(state) is None and chain._fused_setup(state) is None
            with torch.no_grad():
                times = timed({"a": lambda: fused(state), "b": lambda: general(state), "c": lambda: chain(state)}, args.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            rate = float(fused.n_accepted.float().mean()) / fused.n_proposed
            rate_b = float(general.n_accepted.float().mean()) / general.n_proposed
            S = (n * d) | 1
            rows = sampling.mcmc_tile_rows(n * d)
            tiles = (B + rows - 1) // rows
            cfg = f"{min(tiles, 4096)} x 64, {rows}, {(((rows * S + 31) & ~31) + rows * S) * 4} B"
            print(f"<!-- {label} {B}: min .. max " + ", ".join(f"({k}) {min(v):.2f} .. {max(v):.2f}" for k, v in times.items())
                  + f"; acceptance of (b) {rate_b:.2f} -->")
            print(f"| {label} | {B} | {med['a']:.2f} | {med['b']:.0f} | {med['c']:.0f} | {med['a'] / steps * 1e3:.2f} | {rate:.2f} | {cfg} |")
    # the widest shape of the envelope, one launch
    n, d, B, k = 64, 3, 1 << 16, args.cap_steps
    torch.manual_seed(0)
    energy = bg.LennardJonesPotential(n * d, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x = lattice(n, d, 1.1, B, 0.02, dev)
    e = torch.empty(B, device=dev)
    acc = torch.empty(B, dtype=torch.int32, device=dev)
    times = timed({"one": lambda: sampling.pair_mcmc(plan, x, e, False, 1.0, 0.01, k, seed=1, n_accepted=acc)}, args.reps)["one"]
    per_step = statistics.median(times) / k
    print(f"widest shape (LJ, n = 64, d = 3, {B} chains): one launch of {k} steps {statistics.median(times):.2f} ms (min .. max "
          f"{min(times):.2f} .. {max(times):.2f}) = {per_step * 1e3:.1f} us per step; a quarter of a second = {int(250.0 / per_step)} steps; "
          f"acceptance {float(acc.float().mean()) / k:.2f}")


if __name__ == "__main__":
    main()
