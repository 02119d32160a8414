"""Writes tests/golden/solvent.npz: the yardstick of the implicit-solvent tests of ``MolecularMechanicsEnergy``.

No evaluator of GBSA-OBC is at hand (OpenMM is not installed), so the formulas are stated HERE in f64 torch with autograd for the
gradient; the vacuum terms are those of make_molecule_goldens.py.  Nothing of bgflow_amd is imported but the topology of alanine
dipeptide, through tests/molecule_common.py.  Per atom i (charge q, radius r, scale s): rho_i = r_i - 0.009, sigma_i = s_i rho_i; for every
ordered pair j != i at distance d, regime by regime:

    (a) rho_i >= d + sigma_j                 H = 0
    (b) d - sigma_j >= rho_i                 L = d - sigma_j
    (c) otherwise                            L = rho_i
    (d) rho_i < sigma_j - d                  L = sigma_j - d, and H gains 2 (1 / rho_i - 1 / L)
    U = d + sigma_j,  H = 1/L - 1/U + (d / 4)(1/U^2 - 1/L^2) + ln(L / U) / (2 d) + sigma_j^2 (1/L^2 - 1/U^2) / (4 d)
    Psi_i = rho_i / 2 sum_j H,   1 / B_i = 1 / rho_i - tanh(Psi_i - 0.8 Psi_i^2 + 4.85 Psi_i^3) / r_i
    E_GB = -138.935458 (1 / eps_solute - 1 / eps_solvent) [sum_i q_i^2 / (2 B_i) + sum_{i<j} q_i q_j / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j)))]
    E_SA = sum_i 4 pi gamma (r_i + 0.14)^2 (r_i / B_i)^6

The autograd gradient is checked once per case against central differences in f64 (printed).  Per case (key prefix ``<case>_``): the
inputs' checksum, the regime counts [4] (a, b, c, d) over all rows, u64 [150] and g64 [150, 3 n] (the gradient of sum_b a_b u_b) in f64,
and per row class the errors ``err_u32_<class>`` / ``err_g32_<class>`` of the SAME formulas run in f32, by the measures of molecule_common.
Condition on the inputs, asserted here: over the cases every regime occurs, row 3 of every case produces (a) and (d), and (b) is never the
only regime of a case.

    python tests/golden/make_solvent_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import molecule_common as mm  # noqa: E402
import solvent_common as sc  # noqa: E402
from make_molecule_goldens import energy as vacuum_energy  # noqa: E402


def solvent_energy(t, x):
    """E_GB + E_SA [B] in kJ/mol of the rows x [B, 3 n] in x's dtype"""
    dt = x.dtype
    n = int(t["n_atoms"])
    p = x.reshape(x.shape[0], n, 3)
    as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64), dtype=dt)       # noqa: E731
    q, rad, scale = as_t(t["solvent_charge"]), as_t(t["solvent_radius"]), as_t(t["solvent_scale"])
    rho = rad - 0.009
    sigma = scale * rho
    born = []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        d = (p[:, others] - p[:, i:i + 1]).pow(2).sum(-1).sqrt()             # [B, n - 1]
        sg = sigma[others]
        inside, engulfed, separate = rho[i] >= d + sg, rho[i] < sg - d, d - sg >= rho[i]
        L = torch.where(separate, d - sg, torch.where(engulfed, sg - d, rho[i].expand_as(d)))
        U = d + sg
        H = 1 / L - 1 / U + d / 4 * (1 / U ** 2 - 1 / L ** 2) + torch.log(L / U) / (2 * d) + sg ** 2 / (4 * d) * (1 / L ** 2 - 1 / U ** 2)
        H = H + torch.where(engulfed, 2 * (1 / rho[i] - 1 / L), torch.zeros_like(H))
        H = torch.where(inside, torch.zeros_like(H), H)
        psi = rho[i] / 2 * H.sum(-1)
        born.append(1 / (1 / rho[i] - torch.tanh(psi - 0.8 * psi ** 2 + 4.85 * psi ** 3) / rad[i]))
    pre = -mm.COULOMB * (1.0 / float(t["solute_dielectric"]) - 1.0 / float(t["solvent_dielectric"]))
    gamma = float(t["surface_area_energy"])
    e = torch.zeros(x.shape[0], dtype=dt)
    for i in range(n):
        for j in range(i + 1, n):
            d2 = (p[:, i] - p[:, j]).pow(2).sum(-1)
            bb = born[i] * born[j]
            e = e + pre * q[i] * q[j] / (d2 + bb * torch.exp(-d2 / (4 * bb))).sqrt()
    for i in range(n):
        e = e + pre * q[i] ** 2 / (2 * born[i]) + 4 * np.pi * gamma * (rad[i] + 0.14) ** 2 * (rad[i] / born[i]) ** 6
    return e


def energy(t, x):
    return vacuum_energy(t, x) + solvent_energy(t, x)


def u_and_g(t, x, a, dtype):
    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    u = energy(t, x)
    g, = torch.autograd.grad((torch.tensor(a, dtype=dtype) * u).sum(), x)
    return u.detach().numpy(), g.numpy()


def check_gradient(t, x, a):
    """the autograd gradient of sum_b a_b u_b against central differences in f64, on rows 0, 1, 2, 7"""
    rows = np.array([0, 1, 2, 7])
    xr, ar = x[rows].astype(np.float64), a[rows].astype(np.float64)
    _, g = u_and_g(t, xr, ar, torch.float64)
    h = 1e-6
    fd = np.zeros_like(g)
    with torch.no_grad():
        for c in range(xr.shape[1]):
            up, dn = xr.copy(), xr.copy()
            up[:, c] += h
            dn[:, c] -= h
            fd[:, c] = ar * (energy(t, torch.tensor(up)).numpy() - energy(t, torch.tensor(dn)).numpy()) / (2 * h)
    err = np.max(np.abs(g - fd) / (1.0 + np.abs(g).max(axis=1, keepdims=True)))
    assert err < 1e-6, err
    return err


def check_regimes(counts, row3):
    total = sum(counts.values())
    assert (total > 0).all(), total
    for name, c in counts.items():
        assert c[0] + c[2] + c[3] > 0, (name, c)                  # (b) is never the only regime
        assert row3[name][0] > 0 and row3[name][3] > 0, (name, row3[name])


def row3_counts(name):
    """the regime counts of row 3 alone"""
    t, _ = sc.case(name)
    n = int(t["n_atoms"])
    p = sc.inputs(name)["x"][3].astype(np.float64).reshape(n, 3)
    r = np.linalg.norm(p[:, None] - p[None, :], axis=-1)
    rho = t["solvent_radius"] - sc.GB_OFFSET
    sigma = (t["solvent_scale"] * rho)[None, :]
    rho = rho[:, None]
    off = ~np.eye(n, dtype=bool)
    a, d = (rho >= r + sigma) & off, (rho < sigma - r) & off
    b = ~a & ~d & (r - sigma >= rho) & off
    return np.array([a.sum(), b.sum(), (off & ~a & ~b & ~d).sum(), d.sum()], np.int64)


def main():
    out, counts, row3 = {}, {}, {}
    for name in sc.CASES + [sc.EXTRA]:
        t, _ = sc.case(name)
        inp = sc.inputs(name)
        x, a = inp["x"], inp["a"]
        fd = check_gradient(t, x, a)
        u64, g64 = u_and_g(t, x, a, torch.float64)
        u32, g32 = u_and_g(t, x, a, torch.float32)
        assert np.isfinite(u64).all() and np.isfinite(g64).all() and np.isfinite(u32).all() and np.isfinite(g32).all()
        counts[name], row3[name] = sc.regime_counts(name), row3_counts(name)
        out[f"{name}_checksum"] = sc.checksum(inp)
        out[f"{name}_regimes"] = counts[name]
        out[f"{name}_u64"], out[f"{name}_g64"] = u64, g64
        line = [f"{name}: n = {int(t['n_atoms'])}, u in [{u64.min():.4g}, {u64.max():.4g}], autograd vs differences {fd:.2g}, "
                f"regimes a b c d {counts[name].tolist()} (row 3: {row3[name].tolist()});"]
        for cls, rows in mm.CLASSES:
            out[f"{name}_err_u32_{cls}"] = np.array(mm.err_u(u32[rows], u64[rows]))
            out[f"{name}_err_g32_{cls}"] = np.array(mm.err_g(g32[rows], g64[rows]))
            line.append(f"{cls} u {float(out[f'{name}_err_u32_{cls}']):.2g} g {float(out[f'{name}_err_g32_{cls}']):.2g}")
        print(" ".join(line), flush=True)
    check_regimes(counts, row3)
    np.savez(os.path.join(HERE, "solvent.npz"), **out)


if __name__ == "__main__":
    main()
