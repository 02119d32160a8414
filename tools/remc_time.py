"""Time replica exchange inside the chain kernel at the widest shape of the envelope -- Lennard-Jones, n = 64, d = 3, 13107 ladders of
K = 5 temperatures (65535 chains): ONE launch of bgk_pair_remc of 64 steps at ``exchange_every`` = 1 and 16, against one launch of
bgk_pair_mcmc on the same chains and temperatures (no exchange), and the general path (``MCMCStep._step`` and the exchange in torch ops,
energies from bgk_pair_energy) for a few steps.  HIP-event timed, alternated, median of the repetitions; prints the table of DESIGN.md's
"Replica exchange" and the capped-launch line (``MCMC_MAX_STEPS_PER_LAUNCH`` steps at the measured time per step).

    python tools/remc_time.py [--reps 3] [--steps 64] [--general-steps 8]
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

from mcmc_time import lattice, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--general-steps", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, K, L, k, std = 64, 3, 5, 13107, args.steps, 0.01
    B = K * L
    torch.manual_seed(0)
    energy = bg.LennardJonesPotential(n * d, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x = lattice(n, d, 1.1, B, 0.02, dev)
    ladder = torch.tensor([1.0, 1.1, 1.21, 1.331, 1.4641])
    temps = ladder.to(dev).repeat(L)
    e = torch.empty(B, device=dev)
    acc = torch.empty(B, dtype=torch.int32, device=dev)
    nex = {every: torch.empty(B, dtype=torch.int32, device=dev) for every in (1, 16)}      # the counts of the run's last launch, per run
    walkers = torch.arange(K, dtype=torch.int32, device=dev).repeat(L)

    def plain():
        sampling.pair_mcmc(plan, x, e, False, temps, std, k, seed=1, n_accepted=acc)

    def exchange(every):
        def run():
            sampling.pair_mcmc(plan, x, e, False, temps, std, k, seed=1, n_accepted=acc, n_replicas=K, exchange_every=every,
                               n_exchanged=nex[every], walkers=walkers)
        return run

    general = bg.ReplicaExchangeMCMCStep(energy, ladder, proposal=bg.GaussianProposal(std), n_steps=args.general_steps)
    general.fused = False
    state = bg.SamplerState(samples=x.clone())
    assert general._fused_setup(state) is None
    with torch.no_grad():
        times = timed({"plain": plain, "every 1": exchange(1), "every 16": exchange(16), "general": lambda: general(state)}, args.reps)
    rows, rows_x = sampling.mcmc_tile_rows(n * d), sampling.mcmc_tile_rows(n * d) // K * K
    med = {name: statistics.median(v) for name, v in times.items()}
    print(f"{torch.cuda.get_device_name(0)}; LJ n = {n}, d = {d}, {L} ladders of {K} = {B} chains; one launch of {k} steps; median of "
          f"{args.reps} (ms)")
    print("| launch | rows per tile | ms | min .. max | us per step | against bgk_pair_mcmc |")
    print("|---|---|---|---|---|---|")
    for name, label, r in (("plain", "bgk_pair_mcmc, no exchange", rows), ("every 1", "bgk_pair_remc, exchange_every = 1", rows_x),
                           ("every 16", "bgk_pair_remc, exchange_every = 16", rows_x)):
        v = times[name]
        print(f"| {label} | {r} | {med[name]:.2f} | {min(v):.2f} .. {max(v):.2f} | {med[name] / k * 1e3:.1f} | {med[name] / med['plain'] - 1:+.1%} |")
    per_step = med["every 1"] / k
    g_step = med["general"] / args.general_steps
    print(f"general path on the device (exchange_every = 1): {med['general']:.1f} ms for {args.general_steps} steps = {g_step:.2f} ms per step "
          f"(min .. max {min(times['general']):.1f} .. {max(times['general']):.1f}); the exchange launch is {g_step / per_step:.1f} x faster per step")
    cap = sampling.MCMC_MAX_STEPS_PER_LAUNCH
    print(f"a capped exchange launch: {cap} steps x {per_step * 1e3:.1f} us = {cap * per_step:.1f} ms")
    for every in (1, 16):
        pairs = L * sum(len(range(j & 1, K - 1, 2)) for j in range(k // every))
        print(f"exchange_every = {every}: {int(nex[every].sum())} of {pairs} exchanges accepted in the last launch"
              + (f" ({int(nex[every].sum()) / pairs:.2f})" if pairs else ""))
    print(f"Metropolis acceptance of the last launch {float(acc.float().mean()) / k:.2f}")


if __name__ == "__main__":
    main()
