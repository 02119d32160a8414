"""Time the equivariant flow (RK4, Nt = 20, K = 50 distance and O = 10 time kernels) on LJ13 at 2^16 samples and DW4 at 2^18 samples:
(a) the fused launch bgk_kdyn_integrate, (b) the same tableau composed from 4 Nt bgk_kdyn_eval launches, (c) the same composition on
``KernelDynamics._forward_torch`` (the reference's op chain on the same GPU).  HIP-event timed, alternated, median of the repetitions;
prints the table of DESIGN.md's "Equivariant kernel dynamics".

    python tools/kdyn_time.py [--reps 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd.dynamics import integrate_fixed  # noqa: E402


class TorchFormulas(torch.nn.Module):
    def __init__(self, dyn):
        super().__init__()
        self.dyn = dyn

    def forward(self, t, x):
        return self.dyn._forward_torch(t, x)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K, O, Nt = 50, 10, 20
    print(f"{torch.cuda.get_device_name(0)}; RK4, Nt = {Nt}, K = {K}, O = {O}; median of {args.reps} (ms)")
    print("| system | B | (a) fused launch | (b) 4 Nt eval launches | (c) torch formulas | exp / s in (a) | (a) grid x block, rows per tile, dynamic LDS |")
    print("|---|---|---|---|---|---|---|")
    for label, n, d, B, spread in (("LJ13", 13, 3, 1 << 16, 1.0), ("DW4", 4, 2, 1 << 18, 2.0)):
        torch.manual_seed(0)
        dyn = bg.KernelDynamics(n, d, torch.linspace(0, 8, K), torch.full((K,), 0.3), torch.linspace(0, 1, O), torch.full((O,), 0.3)).to(dev)
        with torch.no_grad():
            dyn._weights.mul_(0.1)
            dyn._bias.fill_(0.01)
            dyn._importance.fill_(0.1)
        flow = bg.DiffEqFlow(dyn, use_checkpoints=True, Nt=Nt, method="RK4")
        x = bg.MeanFreeNormalDistribution(n * d, n, std=spread, two_event_dims=False).to(dev).sample(B).contiguous()
        zeros = torch.zeros(B, 1, device=dev)
        composed = bg.DensityDynamics(dyn)
        formulas = bg.DensityDynamics(TorchFormulas(dyn))
        with torch.no_grad():
            ya, la = flow(x)
            yb, lb = integrate_fixed(composed, (x, zeros), 1.0, Nt, "rk4")
            print(f"<!-- {label}: fused vs composed max |dy| {float((ya - yb).abs().max()):.3g}, max |ddlogp| {float((la - lb).abs().max()):.3g} -->")
            runs = {"a": lambda: flow(x), "b": lambda: integrate_fixed(composed, (x, zeros), 1.0, Nt, "rk4"),
                    "c": lambda: integrate_fixed(formulas, (x, zeros), 1.0, Nt, "rk4")}
            times = timed(runs, args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        exps = B * (n * (n - 1) // 2) * K * 4 * Nt
        rows = min(64, 63488 // (4 * ((n * d) | 1) * 4))
        tiles = (B + rows - 1) // rows
        cfg = f"{min(tiles, 4096)} x 64, {rows}, {rows * 4 * ((n * d) | 1) * 4} B"
        print(f"<!-- {label}: min .. max " + ", ".join(f"({k}) {min(v):.2f} .. {max(v):.2f}" for k, v in times.items()) + " -->")
        print(f"| {label} | {B} | {med['a']:.2f} | {med['b']:.2f} | {med['c']:.1f} | {exps / med['a'] * 1e3:.3g} | {cfg} |")


if __name__ == "__main__":
    main()
