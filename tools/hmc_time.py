"""Time Hamiltonian Monte Carlo (10 leapfrog steps, 100 steps per ``sample`` call, 2^16 chains) of LJ13 and the particle box of 38
particles: (a) the fused launches of bgk_pair_hmc / bgk_box_hmc (``IterativeSampler.sample`` of an ``HMCStep``, split at
``hmc_max_steps_per_launch``), (b) the general path on the same device -- the same classes with ``step.fused = False``: the energy and
backward kernels per force call, the elementwise ops and the accept chain in torch ops -- for a few steps, scaled.  HIP-event timed,
alternated, median of the repetitions; prints the table of DESIGN.md's "Hamiltonian Monte Carlo".  The last lines time ONE launch at the
widest shape of the envelope (Lennard-Jones, n = 64, d = 3, 2^16 chains) at 1 and at 10 leapfrog steps next to one launch of
bgk_pair_mcmc on the same chains: the measured basis of ``hmc_max_steps_per_launch``.  Between them a table of Lennard-Jones clusters of
growing n, fused (forced) against general per step: the measured basis of ``HMC_FUSED_MIN_ROWS``.

    python tools/hmc_time.py [--reps 3] [--steps 100] [--general-steps 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import sampling  # noqa: E402
from bgflow_amd.distributions import _kernel_plan  # noqa: E402
from mcmc_time import lattice, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--general-steps", type=int, default=5, help="steps of the general path's run (its time is scaled to --steps)")
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--cap-steps", type=int, default=8, help="steps of the single launches at the widest shape")
    ap.add_argument("--crossover", type=int, nargs="*", default=[16, 20, 26, 40, 64], help="Lennard-Jones cluster sizes of the crossover table")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    steps, B, L = args.steps, args.chains, args.leapfrog
    print(f"{torch.cuda.get_device_name(0)}; {steps} HMC steps of {L} leapfrog steps per sample call, {B} chains; median of {args.reps} "
          f"(ms); launches of at most {sampling.hmc_max_steps_per_launch(L)} steps")
    print(f"| system | step size | (a) fused | (b) general ({args.general_steps} steps, scaled) | (b) / (a) | (a) ms per step | acceptance (a) | acceptance (b) | (a) rows per tile |")
    print("|---|---|---|---|---|---|---|---|---|")
    systems = (("LJ13", lambda: bg.LennardJonesPotential(39, 13, eps=1.0, rm=1.0, two_event_dims=False), 13, 3, 1.1, 0.02, 0.03),
               ("box of 38", lambda: bg.RepulsiveParticles(), 38, 2, 1.0, 0.05, 0.012))
    for label, build, n, d, spacing, jitter, h in systems:
        torch.manual_seed(0)
        energy = build().to(dev)
        x = lattice(n, d, spacing, B, jitter, dev)
        fused_step = bg.HMCStep(energy, h, n_leapfrog=L)
        fused_step.fused = "always"
        fused = bg.IterativeSampler(bg.SamplerState(samples=x), [fused_step], stride=steps)
        general_step = bg.HMCStep(energy, h, n_leapfrog=L)
        general_step.fused = False
        general = bg.IterativeSampler(bg.SamplerState(samples=x), [general_step], stride=args.general_steps)
        assert fused._fused_setup() is not None and general._fused_setup() is None
        times = timed({"a": lambda: fused.sample(1), "b": lambda: general.sample(1)}, args.reps)
        scale = steps / args.general_steps
        med = {"a": statistics.median(times["a"]), "b": statistics.median(times["b"]) * scale}
        rate_a = float(fused_step.n_accepted.float().mean()) / fused_step.n_proposed
        rate_b = float(general_step.n_accepted.float().mean()) / general_step.n_proposed
        print(f"<!-- {label}: min .. max (a) {min(times['a']):.2f} .. {max(times['a']):.2f}, (b, scaled) {min(times['b']) * scale:.0f} .. "
              f"{max(times['b']) * scale:.0f} -->")
        print(f"| {label} | {h} | {med['a']:.2f} | {med['b']:.0f} | {med['b'] / med['a']:.1f} | {med['a'] / steps:.3f} | {rate_a:.2f} | "
              f"{rate_b:.2f} | {sampling.hmc_tile_rows(n * d)} |")
    # where the fused path stops paying: Lennard-Jones clusters of growing n, the kernel forced (fused = "always")
    print("| system | rows per tile | (a) fused, ms per step (min .. max) | (b) general, ms per step (min .. max) | (b) / (a) |")
    print("|---|---|---|---|---|")
    for n in args.crossover:
        torch.manual_seed(0)
        energy = bg.LennardJonesPotential(3 * n, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
        x = lattice(n, 3, 1.1, B, 0.02, dev)
        ka, kb = 14, 2
        fused_step = bg.HMCStep(energy, 0.01, n_leapfrog=L)
        fused_step.fused = "always"
        fused = bg.IterativeSampler(bg.SamplerState(samples=x), [fused_step], stride=ka)
        general_step = bg.HMCStep(energy, 0.01, n_leapfrog=L)
        general_step.fused = False
        general = bg.IterativeSampler(bg.SamplerState(samples=x), [general_step], stride=kb)
        assert fused._fused_setup() is not None and general._fused_setup() is None
        times = timed({"a": lambda: fused.sample(1), "b": lambda: general.sample(1)}, args.reps)
        ta, tb = [t / ka for t in times["a"]], [t / kb for t in times["b"]]
        print(f"| LJ{n} | {sampling.hmc_tile_rows(3 * n)} | {statistics.median(ta):.3f} ({min(ta):.3f} .. {max(ta):.3f}) | "
              f"{statistics.median(tb):.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {statistics.median(tb) / statistics.median(ta):.2f} |")
    # the widest shape of the envelope, one launch each
    n, d, k = 64, 3, args.cap_steps
    torch.manual_seed(0)
    energy = bg.LennardJonesPotential(n * d, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x = lattice(n, d, 1.1, B, 0.02, dev)
    e = torch.empty(B, device=dev)
    acc = torch.empty(B, dtype=torch.int32, device=dev)
    runs = {"mcmc": lambda: sampling.pair_mcmc(plan, x.clone(), e, False, 1.0, 0.01, 8 * k, seed=1, n_accepted=acc),
            "hmc 1": lambda: sampling.pair_hmc(plan, x.clone(), e, False, 1.0, 0.01, 1, 1.0, k, seed=1, n_accepted=acc),
            f"hmc {L}": lambda: sampling.pair_hmc(plan, x.clone(), e, False, 1.0, 0.01, L, 1.0, k, seed=1, n_accepted=acc)}
    times = timed(runs, args.reps)
    per = {}
    for name, count in (("mcmc", 8 * k), ("hmc 1", k), (f"hmc {L}", k)):
        per[name] = statistics.median(times[name]) / count
        print(f"widest shape (LJ, n = 64, d = 3, {B} chains), {name}: one launch of {count} steps {statistics.median(times[name]):.2f} ms "
              f"(min .. max {min(times[name]):.2f} .. {max(times[name]):.2f}) = {per[name]:.3f} ms per step")
    per_leapfrog = (per[f"hmc {L}"] - per["hmc 1"]) / max(1, L - 1)
    print(f"an HMC step of L leapfrog steps = ({per_leapfrog / per['mcmc']:.2f} L + {(per['hmc 1'] - per_leapfrog) / per['mcmc']:.2f}) Metropolis steps; "
          f"acceptance of the last launch {float(acc.float().mean()) / k:.2f}")


if __name__ == "__main__":
    main()
