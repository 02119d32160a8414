"""Time what the robust-training wrappers cost, HIP-event timed, alternating the two forms, and print the lines of profiles/README.md:

    python tools/clipped_time.py [--batch 262144] [--iters 20] [--repeats 5] [--out FILE]

  * the cfg-3 KL training step (KLTrainer + FlatAdam, batch 2^18) with the plain NormalDistribution target (generation tail with the
    fused KL epilogue) and with LinLogCutEnergy(GradientClippedEnergy(Normal, ClipGradient(., 3))) (the tail's training launch followed
    by the one energy launch, bgk_energy_fields_cut);
  * FlatAdam.step() on cfg 3's bucket with and without max_grad_norm.
A record, not a pass criterion."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bgflow_amd as bg                                   # noqa: E402
from bgflow_amd import configs                            # noqa: E402
from bgflow_amd.training import FlatAdam, KLTrainer       # noqa: E402


def event_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(forms, iters, repeats):
    for fn in forms.values():
        event_ms(fn, 3)
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(event_ms(fn, iters))
    return {k: float(np.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clipped_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    trainers = {}
    for name in ("plain Normal target", "LinLogCut(GradientClipped(Normal, ClipGradient(1e-5, 3)))"):
        gen = configs.make_ala2_spline_generator(dev)
        if not name.startswith("plain"):
            gen._target = bg.LinLogCutEnergy(bg.GradientClippedEnergy(gen._target, bg.ClipGradient(1e-5, 3))).to(dev)
        trainers[name] = KLTrainer(gen, optim=FlatAdam([p for p in gen.parameters() if p.requires_grad], lr=1e-4), train_likelihood=False)
    steps = alternate({k: (lambda t=t: t.train(1, batchsize=args.batch)) for k, t in trainers.items()}, args.iters, args.repeats)
    lines = [f"device: {torch.cuda.get_device_name(0)}, cfg-3 KL step at batch {args.batch}, {args.iters} steps per window, median of "
             f"{args.repeats} alternated windows"]
    lines += [f"  KL step, {k}: {v:.3f} ms" for k, v in steps.items()]
    gen = configs.make_ala2_spline_generator(dev)
    opts = {}
    for name, m in (("FlatAdam.step()", None), ("FlatAdam.step(), max_grad_norm=1", 1.0)):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in gen.parameters() if p.requires_grad]
        opts[name] = FlatAdam(ps, lr=1e-4, max_grad_norm=m)
        opts[name].grad.normal_()
    adam = alternate({k: o.step for k, o in opts.items()}, 10 * args.iters, args.repeats)
    lines += [f"  {k} on {next(iter(opts.values())).flat.numel()} parameters: {v * 1e3:.1f} us" for k, v in adam.items()]
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
