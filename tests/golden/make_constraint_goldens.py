#!/usr/bin/env python
"""Generate tests/golden/g_constraints.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_constraint_goldens.py

What runs: the UNMODIFIED reference classes CircularShiftFlow, IncreaseMultiplicityFlow (nn/flow/modulo.py), TorchTransform
(nn/flow/torchtransform.py), SetConstantFlow / MergeFlow / WrapFlow and the four constraint methods of BoltzmannGeneratorBuilder
(factory/generator_builder.py:461-526), with the two import shims of make_goldens.py (``numpy.infty``, nflows_stub).
The fixture holds DATA only: inputs, the ``torch.rand`` draws of the sheaf choice (recorded by replaying the seed), expected outputs
and log-dets.  Inputs carry the edge cases: 0, 1, values within 1e-6 outside [0, 1], negative and > 1 shifts, multiplicities 1..6,
and x + shift landing exactly on an integer.
"""
import os
import sys

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.factory.generator_builder import BoltzmannGeneratorBuilder  # noqa: E402
from bgflow.factory.tensor_info import ShapeDictionary, BONDS, ANGLES, TORSIONS, FIXED  # noqa: E402
from bgflow.nn.flow.modulo import CircularShiftFlow, IncreaseMultiplicityFlow  # noqa: E402
from bgflow.nn.flow.torchtransform import TorchTransform  # noqa: E402

B, SEED = 256, 20240
N = 17
SHIFTS = np.array([0.25, -0.5, -1.3, 1.7, 0.0, 1.0, -1.0, 0.1, 0.9, 2.25, -0.75, 0.333, -0.001, 0.5, 0.7, -2.6, 1e-3], np.float32)
MULTS = np.array([1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 3, 2, 6, 5, 4], np.int64)
C_IDX, C_VAL = np.array([3, 11]), np.array([0.109, 0.101], np.float32)
HALPHA = np.array([4, 9])


def unit_inputs(gen, n):
    x = torch.rand(B, n, generator=gen)
    x[0], x[1], x[2], x[3] = 0.0, 1.0, 1.0 + 5e-7, -5e-7
    x[4] = torch.tensor([0.75, 0.5, 0.3, 0.3, 1.0, 0.0, 1.0, 0.9, 0.1, 0.75, 0.75, 0.667, 0.001, 0.5, 0.3, 0.6, 0.999][:n])  # x + shift integer
    x[5] = torch.tensor([1 / m for m in MULTS[:n]], dtype=torch.float32)        # on a period boundary of the multiplicity fold
    x[6] = torch.tensor([(m - 1) / m for m in MULTS[:n]], dtype=torch.float32)
    return x


def main():
    out = {"seed": np.int64(SEED), "shifts": SHIFTS, "mults": MULTS, "c_idx": C_IDX, "c_val": C_VAL, "halpha": HALPHA}
    gen = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        # each flow alone
        x = unit_inputs(gen, N)
        f = CircularShiftFlow(torch.tensor(SHIFTS))
        y, d = f(x)
        xi, di = f(x, inverse=True)
        out.update(shift_x=x, shift_fwd=y, shift_inv=xi, shift_dlogp=d, shift_dlogp_inv=di)

        f = IncreaseMultiplicityFlow(torch.tensor(MULTS))
        torch.manual_seed(SEED + 1)
        u = torch.rand(B, N)
        torch.manual_seed(SEED + 1)
        y, d = f(x)
        xi, di = f(x, inverse=True)
        out.update(mult_x=x, mult_u=u, mult_fwd=y, mult_inv=xi, mult_dlogp=d)
        assert torch.equal(y, (x + torch.floor(u * torch.tensor(MULTS))) / torch.tensor(MULTS))

        loc, scale = torch.randn(N, generator=gen), torch.randn(N, generator=gen) * 2
        f = TorchTransform(torch.distributions.AffineTransform(loc=loc, scale=scale), 1)
        xa = torch.randn(B, N, generator=gen)
        y, d = f(xa)
        xi, di = f(xa, inverse=True)
        out.update(aff_loc=loc, aff_scale=scale, aff_x=xa, aff_fwd=y, aff_inv=xi, aff_dlogp=d, aff_dlogp_inv=di,
                   aff_logdet64=np.float64(scale.double().abs().log().sum().item()))
        f = TorchTransform(torch.distributions.AffineTransform(loc=0.25, scale=-3.0), 1)       # scalar parameters
        y, d = f(xa)
        out.update(affs_fwd=y, affs_dlogp=d)

        # the four builder layers on the 15 / 17 / 17 / 9 shapes
        shapes = ShapeDictionary()
        shapes[BONDS], shapes[ANGLES], shapes[TORSIONS], shapes[FIXED] = (15,), (17,), (17,), (9,)
        b = BoltzmannGeneratorBuilder(shapes)
        b.add_merge_constraints(C_IDX, C_VAL)
        assert b.current_dims[BONDS] == (17,)
        b.add_torsion_multiplicities(torch.tensor(MULTS))
        b.add_torsion_shifts(torch.tensor(SHIFTS))
        b.add_constrain_chirality(HALPHA)
        flow = b.build_flow()
        zs = [torch.rand(B, 15, generator=gen), torch.rand(B, 17, generator=gen), unit_inputs(gen, N), torch.rand(B, 9, generator=gen)]
        torch.manual_seed(SEED + 2)
        u = torch.rand(B, N)
        torch.manual_seed(SEED + 2)
        *ys, d = flow(*zs)
        *zi, di = flow(*ys, inverse=True)
        for k, t in enumerate(zs):
            out[f"flow_z{k}"] = t
        for k, t in enumerate(ys):
            out[f"flow_y{k}"] = t
        for k, t in enumerate(zi):
            out[f"flow_zi{k}"] = t
        out.update(flow_u=u, flow_dlogp=d, flow_dlogp_inv=di)
        # the merge pair alone (first two layers)
        *ym, dm = flow[:2](*zs)
        *zm, _ = flow[:2](*ym, inverse=True)
        out.update(merge_fwd=ym[0], merge_inv=zm[0], merge_dlogp=dm)
        err = max(float((a[8:] - c[8:]).abs().max()) for a, c in zip(zi, zs))      # (rows 0-7: edge values, 1 folds onto 0)
        print(f"round trip {err:.1e}, chirality log-det {float(d[0]):.7f} (2 ln 0.5 = {2 * np.log(0.5):.7f})")
    path = os.path.join(HERE, "g_constraints.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
