"""Time the particle-system energies on bgk_pair_energy / bgk_pair_energy_backward against each class's own torch formula (``_energy``:
what runs outside the kernel's envelope) on the same GPU, HIP-event timed, alternating the two, and print the lines of DESIGN.md's
"Particle systems" table.

    python tools/pair_time.py [--batch 262144] [--iters 50] [--torch-iters 5] [--repeats 3] [--out FILE]

Systems: DW4 (MultiDoubleWellPotential, n = 4, d = 2), LJ13 and LJ55 (LennardJonesPotential with the oscillator, d = 3).  Bytes of a
launch = 4 (n d + 1) per sample forward, 4 (2 n d + 1) backward; the fraction is of the 8 TB/s HBM peak the project's rooflines use.
The backward is timed alone (the graph of one forward, ``torch.autograd.grad`` with retain_graph).  Energies and gradients of the two
forms are compared before timing."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bgflow_amd as bg                                   # noqa: E402

HBM_PEAK = 8.0e12


def event_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def lattice(n, d, batch, dev, spacing=1.5, jitter=0.2):
    side = int(np.ceil(n ** (1.0 / d) - 1e-9))
    pts = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=torch.float32)] * d, indexing="ij"), -1).reshape(-1, d)[:n]
    pts = ((pts - pts.mean(0)) * spacing).to(dev)
    return (pts[None] + (torch.rand(batch, n, d, device=dev) * 2 - 1) * jitter).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pair_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    systems = [("DW4", bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.0, 4.0), 4, 2),
               ("LJ13", bg.LennardJonesPotential(39, 13, eps=1.0, rm=1.0, oscillator=True, oscillator_scale=1.0), 13, 3),
               ("LJ55", bg.LennardJonesPotential(165, 55, eps=1.0, rm=1.0, oscillator=True, oscillator_scale=1.0), 55, 3)]
    lines = [f"device: {torch.cuda.get_device_name(0)}, batch {args.batch}, {args.iters} kernel / {args.torch_iters} torch launches per window, "
             f"median of {args.repeats} alternated windows",
             "| system | pass | kernel (us) | torch formula (us) | torch / kernel | kernel bytes (MB) | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    for name, energy, n, d in systems:
        spacing = 1.5 if name == "DW4" else 1.1
        x = lattice(n, d, args.batch, dev, spacing=spacing, jitter=0.1).requires_grad_(True)
        g = torch.ones(args.batch, 1, device=dev)
        uk, ut = energy.energy(x), energy._energy(x)
        scale = 1.0 + float(ut.abs().max())
        assert float((uk - ut).abs().max()) <= 1e-4 * scale, (name, float((uk - ut).abs().max()), scale)
        gk, gt = torch.autograd.grad(uk, x, g, retain_graph=True)[0], torch.autograd.grad(ut, x, g, retain_graph=True)[0]
        assert float((gk - gt).abs().max()) <= 1e-4 * (1.0 + float(gt.abs().max())), name
        xd = x.detach()
        passes = [("forward", lambda: energy.energy(xd), lambda: energy._energy(xd), 4.0 * (n * d + 1)),
                  ("backward", lambda: torch.autograd.grad(uk, x, g, retain_graph=True), lambda: torch.autograd.grad(ut, x, g, retain_graph=True),
                   4.0 * (2 * n * d + 1))]
        for what, kernel, torch_form, row_bytes in passes:
            event_ms(kernel, 5), event_ms(torch_form, 2)          # warm-up
            tk, tt = [], []
            for _ in range(args.repeats):
                tk.append(event_ms(kernel, args.iters))
                tt.append(event_ms(torch_form, args.torch_iters))
            k_ms, t_ms = float(np.median(tk)), float(np.median(tt))
            nbytes = row_bytes * args.batch
            bw = nbytes / (k_ms * 1e-3)
            lines.append(f"| {name} | {what} | {k_ms * 1e3:.1f} | {t_ms * 1e3:.1f} | {t_ms / k_ms:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | "
                         f"{100 * bw / HBM_PEAK:.1f} % |")
            print(lines[-1], flush=True)
        del uk, ut, gk, gt, x
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
