"""Time the four constraint layers on bgk_colmap against the same layers written with torch ops (the reference's op chain through
PyTorch-ROCm) on the same GPU, HIP-event timed, alternating the two, and print the lines of profiles/constraints_colmap.md.

    python tools/colmap_time.py [--batch 1048576] [--iters 200] [--repeats 5] [--out FILE]

Layers: constraint merge 17 -> 21 (SetConstantFlow + index MergeFlow, 4 constants), and on the 17- and 21-wide fields the circular
shift, the multiplicity layer (forward and inverse) and the chirality affine.  Bytes of a kernel launch = 4 (n_in + n_out) per
sample; the fraction is of the 8 TB/s HBM peak the project's rooflines use.  Outputs of the two forms are compared before timing."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bgflow_amd as bg                                   # noqa: E402
from bgflow_amd import modulo                             # noqa: E402

HBM_PEAK = 8.0e12


def event_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def layers(n, dev):
    """[(name, kernel form, torch form, n_in, n_out)] on an n-wide field"""
    shift = torch.linspace(-1.3, 1.7, n)
    mult = torch.arange(n) % 6 + 1
    loc, scale = torch.zeros(n), torch.ones(n)
    loc[[4, 9]], scale[[4, 9]] = 0.5, 0.5
    sh, mu = bg.CircularShiftFlow(shift).to(dev), bg.IncreaseMultiplicityFlow(mult).to(dev)
    af = bg.TorchTransform(torch.distributions.AffineTransform(loc.to(dev), scale.to(dev)), 1)
    s_d, m_d = shift.to(dev), mult.to(dev)
    delegate = af._delegate_transform

    def check(x):
        if (x > 1 + 1e-6).any() or (x < -1e-6).any():
            raise ValueError()

    def t_shift(x):
        check(x)
        return (x + s_d) % 1, torch.zeros_like(x[..., [0]])

    def t_mult_fwd(x):
        check(x)
        m = torch.ones_like(x) * m_d
        sheaves = torch.floor(torch.rand(m.shape, device=m.device) * m)
        return (x + sheaves) / m_d, torch.zeros_like(x[..., [0]])

    def t_mult_inv(x):
        check(x)
        return (x % (1 / m_d)) * m_d, torch.zeros_like(x[..., [0]])

    def t_affine(x):
        y = delegate(x)
        return y, delegate.log_abs_det_jacobian(x, y)[..., None]
    return [("circular shift", lambda x: sh(x), t_shift, n, n), ("multiplicity forward", lambda x: mu(x), t_mult_fwd, n, n),
            ("multiplicity inverse", lambda x: mu(x, inverse=True), t_mult_inv, n, n), ("chirality affine", lambda x: af(x), t_affine, n, n)]


def merge_layer(n_free, n_const, dev):
    n = n_free + n_const
    fixed = np.linspace(1, n - 2, n_const).astype(np.int64)
    free = np.setdiff1d(np.arange(n), fixed)
    value = torch.linspace(0.1, 0.11, n_const).to(dev)
    const = bg.SetConstantFlow([1], [value])
    wrap = bg.WrapFlow(bg.MergeFlow(free, fixed), [0, 1], [0])
    fused = modulo.FusedConstantMerge(const, wrap)

    def torch_form(x):
        *ys, d0 = const(x)
        y, d1 = wrap(*ys)
        return y, d0 + d1
    return ("constraint merge", lambda x: fused(x), torch_form, n_free, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "colmap_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = [merge_layer(17, 4, dev)] + [(f"{name} {n}", k, t, a, b) for n in (17, 21) for name, k, t, a, b in layers(n, dev)]
    lines = [f"device: {torch.cuda.get_device_name(0)}, batch {args.batch}, {args.iters} launches per window, median of {args.repeats} alternated windows",
             "| layer | kernel (us) | torch ops (us) | torch / kernel | kernel bytes (MB) | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    with torch.no_grad():
        for name, kernel, torch_form, n_in, n_out in cases:
            x = torch.rand(args.batch, n_in, device=dev)
            yk, dk = kernel(x)
            yt, dt = torch_form(x)
            if "forward" not in name:                 # (the forward multiplicity layer draws: different generators)
                assert torch.equal(yk, yt), name
            assert dk.shape == dt.shape and float((dk - dt).abs().max()) <= 1e-6 * max(1.0, float(dt.abs().max())), name
            for fn in (kernel, torch_form):           # warm-up
                event_ms(lambda: fn(x), 10)
            tk, tt = [], []
            for _ in range(args.repeats):
                tk.append(event_ms(lambda: kernel(x), args.iters))
                tt.append(event_ms(lambda: torch_form(x), args.iters))
            k_ms, t_ms = float(np.median(tk)), float(np.median(tt))
            nbytes = 4.0 * (n_in + n_out) * args.batch
            bw = nbytes / (k_ms * 1e-3)
            lines.append(f"| {name} | {k_ms * 1e3:.1f} | {t_ms * 1e3:.1f} | {t_ms / k_ms:.2f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
