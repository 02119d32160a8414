"""Time annealed switching (``AnnealedSwitching``: 16 linear stages, ``--stage-steps`` steps per stage, 2^16 chains) between the ends

    mean-free normal -> LJ13          mean-free normal -> LJ64 (41 rows per tile)          box of 38 -> its ``biased_system``

(a) the fused launches of bgk_pair_anneal / bgk_box_anneal (``fused = "always"``, split at ``ANNEAL_MAX_STEPS_PER_LAUNCH``), (b) the general
path on the same device -- ``fused = False``: both ends' energy kernels per proposal, the elementwise ops and the accept chain in torch
ops -- for the first ``--general-stages`` stages, scaled.  HIP-event timed, alternated, median of the repetitions; prints the table of
DESIGN.md's "Annealed switching".  Then a table of mean-free normal -> Lennard-Jones clusters of growing n, fused (forced) against
general per step: the measured basis of ``ANNEAL_FUSED_MIN_ROWS``.  The last lines time ONE launch of ``--cap-steps``
steps at the widest shape of the envelope (n = 64, d = 3, 2^16 chains) next to one launch of bgk_pair_mcmc on the same chains: the
measured basis of ``ANNEAL_MAX_STEPS_PER_LAUNCH``.

    python tools/anneal_time.py [--reps 3] [--stage-steps 4] [--general-stages 2]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import annealing, sampling  # noqa: E402
from bgflow_amd.distributions import _kernel_plan  # noqa: E402
from mcmc_time import lattice, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", type=int, default=16)
    ap.add_argument("--stage-steps", type=int, default=4)
    ap.add_argument("--general-stages", type=int, default=2, help="stages of the general path's run (its time is scaled to --stages)")
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--cap-steps", type=int, default=32, help="steps of the single launches at the widest shape")
    ap.add_argument("--crossover", type=int, nargs="*", default=[26, 32, 41, 48, 56], help="Lennard-Jones cluster sizes of the crossover table")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M, K, B = args.stages, args.stage_steps, args.chains
    print(f"{torch.cuda.get_device_name(0)}; {M} stages x {K} steps, {B} chains; median of {args.reps} (ms); launches of at most "
          f"{annealing.ANNEAL_MAX_STEPS_PER_LAUNCH} steps")
    print(f"| ends | noise_std | (a) fused | (b) general ({args.general_stages} stages, scaled) | (b) / (a) | (a) ms per step | (b) ms per step | "
          f"acceptance (a) | (a) rows per tile |")
    print("|---|---|---|---|---|---|---|---|---|")

    def lj(n):
        return (bg.MeanFreeNormalDistribution(3 * n, n, std=1.0, two_event_dims=False),
                bg.LennardJonesPotential(3 * n, n, eps=1.0, rm=1.0, two_event_dims=False))

    def box():
        system = bg.RepulsiveParticles()
        return system, bg.biased_system(system, 50.0, 1.5)

    systems = (("mean-free normal -> LJ13", lambda: lj(13), 13, 3, 1.1, 0.02, 0.03),
               ("mean-free normal -> LJ64", lambda: lj(64), 64, 3, 1.1, 0.02, 0.01),
               ("box of 38 -> biased box", box, 38, 2, 1.0, 0.05, 0.02))
    for label, build, n, d, spacing, jitter, std in systems:
        torch.manual_seed(0)
        a, b = (e.to(dev) for e in build())
        x = lattice(n, d, spacing, B, jitter, dev)
        lambdas = [i / M for i in range(M + 1)]
        fused = bg.AnnealedSwitching(a, b, lambdas, n_steps=K, noise_std=std)
        fused.fused = "always"
        general = bg.AnnealedSwitching(a, b, lambdas[:args.general_stages + 1], n_steps=K, noise_std=std)
        general.fused = False
        assert fused._fused_setup(x) is not None and general._fused_setup(x) is None
        times = timed({"a": lambda: fused(x), "b": lambda: general(x)}, args.reps)
        scale = M / args.general_stages
        med = {"a": statistics.median(times["a"]), "b": statistics.median(times["b"]) * scale}
        rate = float(fused.n_accepted.float().mean()) / fused.n_proposed
        print(f"<!-- {label}: min .. max (a) {min(times['a']):.2f} .. {max(times['a']):.2f}, (b, scaled) {min(times['b']) * scale:.1f} .. "
              f"{max(times['b']) * scale:.1f} -->")
        print(f"| {label} | {std} | {med['a']:.2f} | {med['b']:.1f} | {med['b'] / med['a']:.2f} | {med['a'] / (M * K):.3f} | "
              f"{med['b'] / (M * K):.3f} | {rate:.2f} | {sampling.mcmc_tile_rows(n * d)} |")
    # where the fused path stops paying: mean-free normal -> Lennard-Jones clusters of growing n, the kernel forced
    print("| ends | rows per tile | (a) fused, ms per step (min .. max) | (b) general, ms per step (min .. max) | (b) / (a) |")
    print("|---|---|---|---|---|")
    for n in args.crossover:
        torch.manual_seed(0)
        a, b = (e.to(dev) for e in lj(n))
        x = lattice(n, 3, 1.1, B, 0.02, dev)
        ka, kb = 16, 4
        fused = bg.AnnealedSwitching(a, b, [i / 4 for i in range(5)], n_steps=ka // 4, noise_std=0.01)
        fused.fused = "always"
        general = bg.AnnealedSwitching(a, b, [i / 4 for i in range(5)], n_steps=kb // 4, noise_std=0.01)
        general.fused = False
        assert fused._fused_setup(x) is not None and general._fused_setup(x) is None
        times = timed({"a": lambda: fused(x), "b": lambda: general(x)}, args.reps)
        ta, tb = [t / ka for t in times["a"]], [t / kb for t in times["b"]]
        print(f"| mean-free normal -> LJ{n} | {sampling.mcmc_tile_rows(3 * n)} | {statistics.median(ta):.3f} ({min(ta):.3f} .. {max(ta):.3f}) | "
              f"{statistics.median(tb):.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {statistics.median(tb) / statistics.median(ta):.2f} |")
    # the widest shape of the envelope, one launch each
    n, d, k = 64, 3, args.cap_steps
    torch.manual_seed(0)
    a, b = (e.to(dev) for e in lj(n))
    plan_a, plan_b = _kernel_plan(a, 1.0), _kernel_plan(b, 1.0)
    x = lattice(n, d, 1.1, B, 0.02, dev)
    e_a, e_b = torch.empty(B, device=dev), torch.empty(B, device=dev)
    work = torch.empty(B, dtype=torch.float64, device=dev)
    acc = torch.empty(B, dtype=torch.int32, device=dev)
    table = annealing.anneal_coefficients([i / 8 for i in range(9)]).to(dev)
    assert k % 8 == 0
    runs = {"mcmc": lambda: sampling.pair_mcmc(plan_b, x.clone(), e_b, False, 1.0, 0.01, k, seed=1, n_accepted=acc),
            "anneal": lambda: annealing.pair_anneal(plan_a, plan_b, x.clone(), table, k // 8, 0, k, 0.01, e_a, e_b, False, work, seed=1,
                                                    n_accepted=acc)}
    times = timed(runs, args.reps)
    per = {name: statistics.median(times[name]) / k for name in runs}
    for name in runs:
        print(f"widest shape (n = 64, d = 3, {B} chains), {name}: one launch of {k} steps {statistics.median(times[name]):.2f} ms "
              f"(min .. max {min(times[name]):.2f} .. {max(times[name]):.2f}) = {per[name]:.3f} ms per step")
    print(f"an annealed step = {per['anneal'] / per['mcmc']:.2f} Metropolis steps; {int(0.25e3 / per['anneal'])} steps are 0.25 s")


if __name__ == "__main__":
    main()
