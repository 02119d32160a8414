"""Time ``circular_bump_transform`` at B = 2^18 rows for (K, D) in {(8, 7), (16, 19), (32, 3)}: (a) the kernel path of
csrc/bgk_circular.hip, (b) this package's torch path on the same device and the same inputs (``circular.FUSED`` all False).  Three
operations: forward (no autograd), forward + backward (gradients of y and the four raw parameter tensors), inverse (no autograd).

HIP-event timed, every run warmed up once, then ``--reps`` rounds that alternate (a) and (b) in one process; median and min .. max
in ms.  Prints the table of DESIGN.md "Circular bump mixture".

    python tools/circular_time.py [--reps 5] [--rows 262144]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bgflow_amd import circular  # noqa: E402
from bgflow_amd.circular import circular_bump_transform  # noqa: E402
from mcmc_time import timed  # noqa: E402

SHAPES = ((8, 7), (16, 19), (32, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 18)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "circular_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    B = args.rows
    print(f"{torch.cuda.get_device_name(0)}; B = {B} rows; median of {args.reps} (min .. max), ms")
    print("| (K, D) | operation | (a) kernel | (b) torch path | (b) / (a) |")
    print("|---|---|---|---|---|")
    for K, D in SHAPES:
        g = torch.Generator().manual_seed(1000 * K + D)
        mr, ls, lw = (s * torch.randn(B, K * D, generator=g) for s in (3.0, 1.5, 2.0))
        le = 2.0 * torch.randn(B, D, generator=g) - 3.0
        y = torch.rand(B, D, generator=g)
        mr, ls, lw, le, y = (v.to(dev) for v in (mr, ls, lw, le, y))
        circular.FUSED.update(forward=True, inverse=True, backward=True)
        assert circular._kernel_takes(y, (mr, ls, lw, le), K, False)

        def run(fused, op):
            circular.FUSED.update(forward=fused, inverse=fused, backward=fused)
            if op == "forward + backward":
                leaves = [v.detach().requires_grad_(True) for v in (y, mr, ls, lw, le)]
                out, dlogp = circular_bump_transform(*leaves)
                return torch.autograd.grad(out.sum() + dlogp.sum(), leaves)
            with torch.no_grad():
                return circular_bump_transform(y, mr, ls, lw, le, inverse=(op == "inverse"))

        for op in ("forward", "forward + backward", "inverse"):
            t = timed({"a": lambda: run(True, op), "b": lambda: run(False, op)}, args.reps)
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            print(f"| ({K}, {D}) | {op} | {ma:.3f} ({min(t['a']):.3f} .. {max(t['a']):.3f}) | {mb:.3f} ({min(t['b']):.3f} .. {max(t['b']):.3f}) | "
                  f"{mb / ma:.1f} |", flush=True)


if __name__ == "__main__":
    main()
