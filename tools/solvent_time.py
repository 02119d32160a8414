"""Time ``MolecularMechanicsEnergy`` with an implicit solvent (GBSA-OBC) at B = 2^18 rows of butane (4 atoms), alanine dipeptide (22) and
a 64-atom chain, each the synthetic force field of ``configs.synthetic_forcefield(..., implicit_solvent=True)``:

    (i)    the solvent kernels of csrc/bgk_molecule.hip (``fused = "always"``)
    (ii)   the class's own torch formulas on the same device and inputs (``fused = False``); where rows x n^2 exceeds ``--elements``
           (2^27: only the 64-atom chain, 8 chunks of 2^15 rows) in chunks of rows, so that the [rows, n, n] intermediates and their
           autograd copies fit -- one measurement, one pair of events around all chunks
    (iii)  the vacuum kernel (the same force field without the solvent) on the same rows: what the solvent terms cost on top of it

Two workloads: the energy (no autograd) and the energy with its gradient with respect to x.  HIP-event timed, every run warmed up twice,
then ``--reps`` rounds that alternate the three; median and min .. max in ms.  Also printed: the largest difference of (i) and (ii) on the
first chunk, relative to 1 + |u|.  Prints the table of DESIGN.md's "Implicit solvent".

    python tools/solvent_time.py [--reps 5] [--rows 262144] [--elements 134217728]
"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

from bgflow_amd import configs, molecule  # noqa: E402
from bgflow_amd.distributions import MoleculePlan, _kernel_plan  # noqa: E402
from mcmc_time import timed  # noqa: E402
import molecule_common as mm  # noqa: E402


def systems():
    z, xyz = mm.ala2_topology()
    return (("butane4", mm.chain_z_matrix(4), mm.chain_xyz(4)), ("ala2", z, xyz), ("chain64", mm.chain_z_matrix(64), mm.chain_xyz(64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--elements", type=int, default=1 << 27)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "solvent_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    B = args.rows
    print(f"{torch.cuda.get_device_name(0)}; B = {B} rows; median of {args.reps} (min .. max), ms")
    print("| system | workload | (i) solvent kernel | (ii) torch formulas | (iii) vacuum kernel | (ii) / (i) | (i) / (iii) |")
    print("|---|---|---|---|---|---|---|")
    for name, z, xyz in systems():
        kernel = configs.synthetic_forcefield(z, xyz, seed=0, implicit_solvent=True).to(dev)
        kernel.fused = "always"
        general = configs.synthetic_forcefield(z, xyz, seed=0, implicit_solvent=True).to(dev)
        general.fused = False
        vacuum = configs.synthetic_forcefield(z, xyz, seed=0).to(dev)
        vacuum.fused = "always"
        g = torch.Generator().manual_seed(7)
        x = (torch.from_numpy(xyz.reshape(1, -1)).float() + mm.NOISE * torch.randn(B, xyz.size, generator=g)).to(dev).contiguous()
        for e in (kernel, vacuum):
            plan = _kernel_plan(e, 1.0)
            assert isinstance(plan, MoleculePlan) and molecule._kernel_operands(plan, (x,)) is not None
        assert _kernel_plan(general, 1.0) is None
        chunk = min(B, max(1, args.elements // (len(xyz) ** 2)))
        chunks = [x[lo:lo + chunk] for lo in range(0, B, chunk)]
        with torch.no_grad():
            ua, ub = kernel.energy(chunks[0]), general.energy(chunks[0])
        diff = float(((ua - ub).abs() / (1.0 + ub.abs())).max())

        def energy(m, parts):
            with torch.no_grad():
                return [m.energy(p) for p in parts]

        def grad(m, parts):
            out = []
            for p in parts:
                xg = p.detach().requires_grad_(True)
                out.append(torch.autograd.grad(m.energy(xg).sum(), xg)[0])
            return out

        for label, fn in (("energy", energy), ("energy + grad", grad)):
            runs = {"i": lambda: fn(kernel, [x]), "ii": lambda: fn(general, chunks), "iii": lambda: fn(vacuum, [x])}
            for run in runs.values():
                run()                                                    # (timed() warms every run up once more)
            t = timed(runs, args.reps)
            med = {k: statistics.median(v) for k, v in t.items()}
            cell = lambda k: f"{med[k]:.3f} ({min(t[k]):.3f} .. {max(t[k]):.3f})"       # noqa: E731
            print(f"| {name} | {label} | {cell('i')} | {cell('ii')} | {cell('iii')} | {med['ii'] / med['i']:.1f} | {med['i'] / med['iii']:.1f} |")
        print(f"<!-- {name}: max |u_i - u_ii| / (1 + |u_ii|) = {diff:.2e} on the first {len(chunks[0])} rows; (ii) in {len(chunks)} chunk(s) -->")


if __name__ == "__main__":
    main()
