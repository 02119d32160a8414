"""Time the stochastic integrators (200 steps) of LJ13 and DW4 at 4096 and 65536 samples: (a) the fused launches of bgk_pair_langevin
(``BrownianFlow`` / ``LangevinFlow``, split at ``LANGEVIN_MAX_STEPS_PER_LAUNCH``), (b) ``fused = False`` -- the reference's step in torch
ops with the forces from bgk_pair_energy / bgk_pair_energy_backward, one step at a time.  HIP-event timed, one warm-up, alternated
rounds, median; prints the table of DESIGN.md's "Stochastic layers".  The last lines time ONE launch at the widest shape of the envelope
(Lennard-Jones, n = 64, d = 3, 2^16 samples) for either integrator: the measured basis of ``LANGEVIN_MAX_STEPS_PER_LAUNCH``.

    python tools/langevin_time.py [--reps 3] [--steps 200] [--cap-steps 16]

``--backward``: a training step instead -- the layer's forward on inputs that require grad and the backward of dW.sum() + outputs.sum(),
``--train-steps`` (10) steps -- (a) with ``fused_backward = True`` (bgk_pair_langevin_record + bgk_pair_langevin_backward), (b) on the
general path (the reference's op chain with ``autograd.grad(..., create_graph=True)`` over the torch formulas and a backward through that
graph: what a layer without the switch runs); same shapes, same timing.  Its last lines time ONE launch of bgk_pair_langevin_backward
at the widest shape: the measured basis of ``LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH``.

    python tools/langevin_time.py --backward [--reps 3] [--train-steps 10] [--cap-steps 16]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import stochastic  # noqa: E402
from bgflow_amd.distributions import _kernel_plan  # noqa: E402

from mcmc_time import lattice, timed  # noqa: E402


def tile_config(nd, tiles, B):
    S = nd | 1
    rows = 64
    while tiles * rows * S * 4 > 63488:
        rows -= 1
    n_tiles = (B + rows - 1) // rows
    return f"{min(n_tiles, 4096)} x 64, {rows}, {tiles * rows * S * 4} B"


SYSTEMS = (("LJ13", lambda: bg.LennardJonesPotential(39, 13, eps=1.0, rm=1.0, two_event_dims=False), 13, 3, 1.1, 0.02, 1e-4),
           ("DW4", lambda: bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.0, 4.0, two_event_dims=False), 4, 2, 4.0, 0.3, 1e-3))


def backward_mode(args, dev):
    steps = args.train_steps
    print(f"{torch.cuda.get_device_name(0)}; training step (forward + backward) of {steps} steps; median of {args.reps} (ms); backward "
          f"launches of at most {stochastic.LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH} steps")
    print("| layer | system | samples | (a) fused backward | (b) general path | (b) / (a) | (a) backward grid x block, rows per tile, dynamic LDS |")
    print("|---|---|---|---|---|---|---|")

    def train_step(flow, xs):
        *ys, dW = flow(*xs)
        return torch.autograd.grad(dW.sum() + sum(y.sum() for y in ys), xs)

    for label, build, n, d, spacing, jitter, h in SYSTEMS:
        for B in (4096, 65536):
            torch.manual_seed(0)
            energy = build().to(dev)
            x = lattice(n, d, spacing, B, jitter, dev).requires_grad_(True)
            v = torch.randn(B, n * d, device=dev).requires_grad_(True)
            for layer, cls, xs in (("Brownian", bg.BrownianFlow, (x,)), ("Langevin", bg.LangevinFlow, (x, v))):
                fused = cls(energy, nsteps=steps, stepsize=h)
                fused.fused_backward = True
                general = cls(energy, nsteps=steps, stepsize=h)
                assert fused._fused_train_setup(*xs) is not None and general._fused_setup(*xs) is None and not general.fused_backward
                times = timed({"a": lambda: train_step(fused, xs), "b": lambda: train_step(general, xs)}, args.reps)
                ga = train_step(fused, xs)
                finite = all(bool(torch.isfinite(g).all()) for g in ga)
                med = {k: statistics.median(t) for k, t in times.items()}
                print(f"<!-- {layer} {label} {B}: min .. max " + ", ".join(f"({k}) {min(t):.2f} .. {max(t):.2f}" for k, t in times.items())
                      + f"; gradients finite {finite} -->")
                print(f"| {layer} | {label} | {B} | {med['a']:.2f} | {med['b']:.1f} | {med['b'] / med['a']:.1f} | {tile_config(n * d, 5, B)} |")
    # the widest shape of the envelope, one backward launch
    n, d, B, k = 64, 3, 1 << 16, args.cap_steps
    torch.manual_seed(0)
    energy = bg.LennardJonesPotential(n * d, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x0 = lattice(n, d, 1.1, B, 0.02, dev)
    dW, g_dW = torch.empty(B, device=dev), torch.ones(B, device=dev)
    for layer, with_v in (("Brownian", False), ("Langevin", True)):
        q, v0 = x0.clone(), (torch.zeros_like(x0) if with_v else None)
        v = None if v0 is None else v0.clone()
        tq = torch.empty((k,) + x0.shape, device=dev)
        tv = torch.empty_like(tq) if with_v else None
        stochastic.pair_langevin_record(plan, q, v, 1e-5, 1.0, 1.0, 1.0, k, dW, tq, tv, seed=1)
        gq, carry = torch.empty_like(x0), torch.empty_like(x0)
        gv = torch.empty_like(x0) if with_v else None
        times = []
        for r in range(args.reps + 1):                     # one warm-up; the adjoints are reset before every launch, outside the timed region
            gq.fill_(1.0)
            carry.zero_()
            if with_v:
                gv.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            stochastic.pair_langevin_backward(plan, x0, v0, tq, tv, 1e-5, 1.0, 1.0, 1.0, g_dW, gq, gv, carry, True, seed=1)
            b.record()
            torch.cuda.synchronize()
            if r > 0:
                times.append(a.elapsed_time(b))
        finite = bool(torch.isfinite(gq).all()) and (not with_v or bool(torch.isfinite(gv).all()))
        per_step = statistics.median(times) / k
        print(f"widest shape, {layer} backward (LJ, n = 64, d = 3, {B} samples): one launch of {k} steps {statistics.median(times):.2f} ms (min .. "
              f"max {min(times):.2f} .. {max(times):.2f}) = {per_step * 1e3:.1f} us per step; a quarter of a second = {int(250.0 / per_step)} "
              f"steps; recorded states finite {bool(torch.isfinite(tq).all())}, gradients finite {finite}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cap-steps", type=int, default=16, help="steps of the single launch at the widest shape")
    ap.add_argument("--backward", action="store_true", help="time a training step and the backward launch instead")
    ap.add_argument("--train-steps", type=int, default=10, help="nsteps of the layer in the training step (--backward)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.backward:
        return backward_mode(args, dev)
    steps = args.steps
    print(f"{torch.cuda.get_device_name(0)}; {steps} steps; median of {args.reps} (ms); launches of at most "
          f"{stochastic.LANGEVIN_MAX_STEPS_PER_LAUNCH} steps")
    print("| layer | system | samples | (a) fused | (b) general, energy kernels | (a) us per step | (a) grid x block, rows per tile, dynamic LDS |")
    print("|---|---|---|---|---|---|---|")
    for label, build, n, d, spacing, jitter, h in SYSTEMS:
        for B in (4096, 65536):
            torch.manual_seed(0)
            energy = build().to(dev)
            x = lattice(n, d, spacing, B, jitter, dev)
            v = torch.randn_like(x)
            for layer, cls, xs, tiles in (("Brownian", bg.BrownianFlow, (x,), 4), ("Langevin", bg.LangevinFlow, (x, v), 5)):
                fused = cls(energy, nsteps=steps, stepsize=h)
                general = cls(energy, nsteps=steps, stepsize=h)
                general.fused = False
                assert fused._fused_setup(*xs) is not None and general._fused_setup(*xs) is None
                with torch.no_grad():
                    times = timed({"a": lambda: fused(*xs), "b": lambda: general(*xs)}, args.reps)
                    finite = bool(torch.isfinite(fused(*xs)[-1]).all())
                med = {k: statistics.median(t) for k, t in times.items()}
                print(f"<!-- {layer} {label} {B}: min .. max " + ", ".join(f"({k}) {min(t):.2f} .. {max(t):.2f}" for k, t in times.items())
                      + f"; dW finite {finite} -->")
                print(f"| {layer} | {label} | {B} | {med['a']:.2f} | {med['b']:.0f} | {med['a'] / steps * 1e3:.2f} | {tile_config(n * d, tiles, B)} |")
    # the widest shape of the envelope, one launch
    n, d, B, k = 64, 3, 1 << 16, args.cap_steps
    torch.manual_seed(0)
    energy = bg.LennardJonesPotential(n * d, n, eps=1.0, rm=1.0, two_event_dims=False).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x0 = lattice(n, d, 1.1, B, 0.02, dev)
    dW = torch.empty(B, device=dev)
    for layer, with_v in (("Brownian", False), ("Langevin", True)):
        x, v = x0.clone(), (torch.zeros_like(x0) if with_v else None)
        times = timed({"one": lambda: stochastic.pair_langevin(plan, x, v, 1e-5, 1.0, 1.0, 1.0, k, dW, seed=1)}, args.reps)["one"]
        per_step = statistics.median(times) / k
        print(f"widest shape, {layer} (LJ, n = 64, d = 3, {B} samples): one launch of {k} steps {statistics.median(times):.2f} ms (min .. max "
              f"{min(times):.2f} .. {max(times):.2f}) = {per_step * 1e3:.1f} us per step; a quarter of a second = {int(250.0 / per_step)} steps; "
              f"states finite {bool(torch.isfinite(x).all())}")


if __name__ == "__main__":
    main()
