"""Writes tests/golden/molecule.npz: the yardstick of the ``MolecularMechanicsEnergy`` tests.

No force-field evaluator is at hand, so the formulas are stated HERE, term by term, in f64 torch with autograd for the gradient
(nothing of bgflow_amd is imported but ``configs.ala2_system()`` for the topology, through tests/molecule_common.py):

    bonds      k / 2 (r - r0)^2
    angles     k / 2 (theta - theta0)^2,  theta = atan2(|a x b|, a . b) at the middle atom
    torsions   k (1 + cos(n phi - phase)),  phi = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))
    pairs      4 eps ((sigma / r)^12 - (sigma / r)^6) + 138.935458 qq / r  over the pairs that interact (tests/molecule_common.pair_table:
               a brute-force loop over i < j, an exception replacing the Lorentz-Berthelot rule)

The autograd gradient is checked once per case against central differences in f64.  Per case (key prefix ``<case>_``): the inputs'
checksum, u64 [150] and g64 [150, 3 n] (the gradient of sum_b a_b u_b) in f64, and per row class (bulk, s0..s3) the errors
``err_u32_<class>`` / ``err_g32_<class>`` of the SAME formulas run in f32, by the measures of molecule_common.

    python tests/golden/make_molecule_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import molecule_common as mm  # noqa: E402


def energy(t, x):
    """E [B] in kJ/mol of the rows x [B, 3 n] in x's dtype"""
    dt = x.dtype
    p = x.reshape(x.shape[0], -1, 3)
    as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64), dtype=dt)       # noqa: E731
    e = torch.zeros(x.shape[0], dtype=dt)
    for (i, j), r0, k in zip(t["bond_idx"].tolist(), as_t(t["bond_r0"]), as_t(t["bond_k"])):
        r = (p[:, i] - p[:, j]).pow(2).sum(-1).sqrt()
        e = e + 0.5 * k * (r - r0) ** 2
    for (i, j, k_), th0, k in zip(t["angle_idx"].tolist(), as_t(t["angle_theta0"]), as_t(t["angle_k"])):
        a, b = p[:, i] - p[:, j], p[:, k_] - p[:, j]
        theta = torch.atan2(torch.linalg.cross(a, b).pow(2).sum(-1).sqrt(), (a * b).sum(-1))
        e = e + 0.5 * k * (theta - th0) ** 2
    for (i, j, k_, l), n, phase, k in zip(t["torsion_idx"].tolist(), t["torsion_periodicity"].tolist(), as_t(t["torsion_phase"]),
                                          as_t(t["torsion_k"])):
        b1, b2, b3 = p[:, j] - p[:, i], p[:, k_] - p[:, j], p[:, l] - p[:, k_]
        n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
        phi = torch.atan2(b2.pow(2).sum(-1).sqrt() * (b1 * n2).sum(-1), (n1 * n2).sum(-1))
        e = e + k * (1 + torch.cos(n * phi - phase))
    li, lj, qq, sigma, eps4 = mm.live_pairs(t)
    for i, j, q, s, e4 in zip(li.tolist(), lj.tolist(), as_t(qq), as_t(sigma), as_t(eps4)):
        r = (p[:, i] - p[:, j]).pow(2).sum(-1).sqrt()
        s6 = (s / r) ** 6
        e = e + e4 * (s6 * s6 - s6) + q / r
    return e


def u_and_g(t, x, a, dtype):
    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    u = energy(t, x)
    g, = torch.autograd.grad((torch.tensor(a, dtype=dtype) * u).sum(), x)
    return u.detach().numpy(), g.numpy()


def check_gradient(t, x, a):
    """the autograd gradient of sum_b a_b u_b against central differences in f64, on the first rows"""
    rows = np.array([0, 1, 2, 7])
    xr, ar = x[rows].astype(np.float64), a[rows].astype(np.float64)
    _, g = u_and_g(t, xr, ar, torch.float64)
    h = 1e-6
    fd = np.zeros_like(g)
    for c in range(xr.shape[1]):
        up, dn = xr.copy(), xr.copy()
        up[:, c] += h
        dn[:, c] -= h
        eu = energy(t, torch.tensor(up)).numpy()
        ed = energy(t, torch.tensor(dn)).numpy()
        fd[:, c] = ar * (eu - ed) / (2 * h)
    err = np.max(np.abs(g - fd) / (1.0 + np.abs(g).max(axis=1, keepdims=True)))
    assert err < 1e-6, err
    return err


def main():
    out = {}
    for name in mm.CASES:
        t, _ = mm.case(name)
        inp = mm.inputs(name)
        x, a = inp["x"], inp["a"]
        fd = check_gradient(t, x, a)
        u64, g64 = u_and_g(t, x, a, torch.float64)
        u32, g32 = u_and_g(t, x, a, torch.float32)
        assert np.isfinite(u64).all() and np.isfinite(g64).all() and np.isfinite(u32).all() and np.isfinite(g32).all()
        out[f"{name}_checksum"] = mm.checksum(inp)
        out[f"{name}_u64"], out[f"{name}_g64"] = u64, g64
        line = [f"{name}: n = {int(t['n_atoms'])}, u in [{u64.min():.4g}, {u64.max():.4g}], autograd vs differences {fd:.2g};"]
        for cls, rows in mm.CLASSES:
            out[f"{name}_err_u32_{cls}"] = np.array(mm.err_u(u32[rows], u64[rows]))
            out[f"{name}_err_g32_{cls}"] = np.array(mm.err_g(g32[rows], g64[rows]))
            line.append(f"{cls} u {float(out[f'{name}_err_u32_{cls}']):.2g} g {float(out[f'{name}_err_g32_{cls}']):.2g}")
        print(" ".join(line))
    np.savez(os.path.join(HERE, "molecule.npz"), **out)


if __name__ == "__main__":
    main()
