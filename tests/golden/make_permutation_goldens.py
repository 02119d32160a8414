"""Writes tests/golden/permutation.npz: inputs and expected permutations for bgflow_amd.HungarianMapper (tests/permutation_common.py,
test_host_permutation.py, test_gpu_permutation.py).  numpy and scipy only: the reference's module
(distribution/sampling/_mcmc/permutation.py) imports ``deep_boltzmann`` and cannot be imported, so the oracle is what it calls --
``scipy.optimize.linear_sum_assignment`` on the f64 squared-distance matrix -- applied to the f32 inputs stored here.

    python tests/golden/make_permutation_goldens.py

Per case ``<name>``: ``_xref`` [n d] f32, ``_ip`` [m] int32 (ascending), ``_X`` [B, n d] f32, ``_perm`` [B, m] int16 (row i of the problem
= reference particle ip[i] receives sample particle ip[perm[b, i]]), ``_stable`` [B] bool.  A row is STABLE when the solution on the
f32-computed cost matrix (difference, square, sum over k in f32 -- the kernel's costs) equals the one on the f64 matrix; tests demand
the exact permutation on stable rows only.  More than 0.5 % unstable rows in a case is an error here, not something to skip.

Rows: row b of a case is the reference with its identical particles shuffled plus Gaussian noise of NOISE[b % 3] on every coordinate
(3.0 on a +-5 box: most rows need long augmenting paths); rows with b % 8 == 7 are the reference itself (expected: the identity) and
rows with b % 8 == 5 the unshuffled reference plus noise 1e-3 (the identity unless two reference positions are that close).
"""
import json
import os

import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
NOISE = (0.05, 0.5, 3.0)
MAX_UNSTABLE = 0.005
F = np.float32


def layout(kind, m):
    """(n, identical particle indices): the identical set is a strict subset with other particles interleaved"""
    if kind == "box":                # the solvent box: two dimer particles in front
        return m + 2, np.arange(2, m + 2)
    if kind == "ends":               # one other particle at either end
        return m + 2, np.arange(1, m + 1)
    assert kind == "gaps"            # another particle after every third identical one, and one in front
    ip = np.arange(m) + 1 + np.arange(m) // 3
    return int(ip[-1]) + 2, ip


def cases():
    out = []
    kinds = ("ends", "gaps", "box")
    for a, m in enumerate((1, 2, 3, 31, 32, 33, 63, 64)):
        for d in (1, 2, 3):
            out.append((f"m{m}_d{d}_b3", kinds[(a + d) % 3], m, d, 3))
    out += [("m36_d2_b1", "box", 36, 2, 1), ("m64_d3_b1", "gaps", 64, 3, 1), ("m1_d1_b1", "ends", 1, 1, 1),
            ("m36_d2_b3", "box", 36, 2, 3),
            ("m3_d3_b257", "gaps", 3, 3, 257), ("m31_d1_b257", "ends", 31, 1, 257), ("m33_d1_b257", "box", 33, 1, 257)]
    return out


def cost32(ref, pts):
    s = None
    for k in range(ref.shape[1]):
        t = (ref[:, None, k] - pts[None, :, k]).astype(F)
        s = (t * t).astype(F) if s is None else (s + (t * t).astype(F)).astype(F)
    return s


def solve(ref, pts):
    """(f64 solution, stable) of one sample: ref, pts [m, d] f32"""
    C = ((ref.astype(np.float64)[:, None, :] - pts.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    c64 = linear_sum_assignment(C)[1]
    c32 = linear_sum_assignment(cost32(ref, pts).astype(np.float64))[1]
    return c64, bool(np.array_equal(c64, c32))


def main():
    rng = np.random.default_rng(20261019)
    out, meta = {}, []
    for name, kind, m, d, B in cases():
        n, ip = layout(kind, m)
        xref = rng.uniform(-5.0, 5.0, (n, d)).astype(F)
        X = np.empty((B, n, d), dtype=F)
        perm = np.empty((B, m), dtype=np.int16)
        stable = np.empty(B, dtype=bool)
        for b in range(B):
            row = xref.astype(np.float64).copy()
            if b % 8 == 5:
                row += 1e-3 * rng.standard_normal(row.shape)
            elif b % 8 != 7:
                row[ip] = row[ip][rng.permutation(m)]
                row += NOISE[b % 3] * rng.standard_normal(row.shape)
            X[b] = row.astype(F)
            perm[b], stable[b] = solve(xref[ip], X[b][ip])
        unstable = int((~stable).sum())
        if unstable > MAX_UNSTABLE * B:
            raise SystemExit(f"{name}: {unstable} of {B} rows are unstable (more than {MAX_UNSTABLE:.1%})")
        identity = (perm == np.arange(m)[None, :]).all(axis=1)
        if B >= 8:
            assert identity[7::8].all() and identity[5::8].mean() > 0.5, name
        out[name + "_xref"], out[name + "_ip"], out[name + "_X"] = xref.reshape(-1), ip.astype(np.int32), X.reshape(B, n * d)
        out[name + "_perm"], out[name + "_stable"] = perm, stable
        meta.append(dict(name=name, n=n, m=m, d=d, B=B, unstable=unstable, identity_rows=int(identity.sum())))
        print(meta[-1])
    out["cases"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "permutation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 160_000


if __name__ == "__main__":
    main()
