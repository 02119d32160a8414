"""The checkers of the internal-coordinate kernels under the constructors' switches (normalize_angles, enforce_boundaries, eps) and on
branched Z-matrices: the C oracle (oracle.ic_xyz2ic, ic_ic2xyz, ic_ic2xyz_backward, refsys through global_ic_*) and the torch
restatements (oracle/torch_flow.py::ic2xyz_torch, xyz2ic_torch, values and autograd gradients) against the unmodified reference's f64
results in tests/golden/ic_switches.npz -- every molecule, every switch set, per element, on the fixture's recorded samples:

    f64   within 1e-10 of the array's largest entry
    f32   within 4 x dev + 1e-6 x max|want|   (dev = the reference's own largest |f32 - f64| of that array, from the fixture)

No GPU: this pins the branches of the checkers that tests/test_gpu_ic_switches.py relies on."""
import numpy as np
import pytest
import torch

import ic_switches_common as C


@pytest.fixture(scope="module")
def G(golden):
    return golden("ic_switches")


def _check(G, mol, sname, name, got, want, sfx, failures):
    err = C.error(got, want, name, sname)
    big = float(np.abs(want).max())
    bound = 1e-10 * big if sfx == "64" else C.bound32(G, mol, sname, name, want)
    ratio = C.report(f"{mol}.{sname}.{name} (f{sfx})", err, bound)
    if not ratio <= 1.0:
        failures.append((name, sfx, ratio))


def test_fixture_conditions(G):
    """what the generator asserted, re-read from the file: 70 samples, the clamp masks of every case"""
    rec = G["rec"]
    assert len(rec) == 16 and set(range(64, 70)) <= set(rec.tolist())
    for mol, sname in C.CASES:
        key = f"{mol}.{sname}."
        eps, enforce = C.SETS[sname].get("eps", 1e-7), C.SETS[sname].get("enforce_boundaries", True)
        assert G[key + "below_inv"].shape == (70,)
        for d in ("inv", "fwd"):
            below, clamped = G[key + f"below_{d}"], G[key + f"clamped_{d}"]
            assert np.array_equal(clamped, below & enforce)
            assert (4 <= below.sum() <= 35) if eps > 1e-4 else not below.any()
        assert G[key + "xysq_below_fwd"].all() if eps > 1e-4 else not G[key + "xysq_below_fwd"].any()
    for mol in C.MOLS:
        z, f = G[f"{mol}.z_matrix"], G[f"{mol}.fixed"]
        if mol == "ala2":
            continue
        assert sorted(f.tolist()) != f.tolist() and set(f.tolist()) != {0, 1, 2}
        if mol.startswith("hub"):
            from bgflow_amd.ic import _placement_table
            assert not np.array_equal(_placement_table(z, f)[:, 4], np.arange(len(z))), "rows must not sit in placement order"


def test_whitening_equals_the_reference(G):
    """the PCA of the rigid block that every mixed case is built on (sign of the components included)"""
    w = C.make(G, "ala2", "default")._whiten
    for got, k in ((w.X0mean, "wh_mean"), (w.Twhiten, "wh_Twhiten"), (w.Tblacken, "wh_Tblacken")):
        want = G[f"ala2.{k}"]
        assert np.abs(got.numpy() - want).max() <= 1e-9 * np.abs(want).max(), k
    assert abs(float(w.jacobian_xz) - float(G["ala2.wh_jac"])) < 1e-9


@pytest.mark.parametrize("mol,sname", C.CASES)
def test_c_oracle(G, oracle, mol, sname):
    """values and log-dets of both directions in both precisions; the closed-form backward sweep on the samples without a clamped norm
    (where it is valid, see bgo_impl.h)"""
    kw = C.SETS[sname]
    sw = dict(normalize_angles=kw.get("normalize_angles", True), eps=kw.get("eps", 1e-7), enforce_boundaries=kw.get("enforce_boundaries", True))
    key, rec = f"{mol}.{sname}.", G["rec"]
    z, fixed = G[f"{mol}.z_matrix"], G[f"{mol}.fixed"]
    ins = [np.asarray(v)[rec] for v in C.inputs(G, mol, sname)]
    failures = []
    for dt, sfx in ((np.float64, "64"), (np.float32, "32")):
        x_ref, xin = G[key + "x"], G[key + "xin"]
        if C.kind(mol) == "glob":
            x, dli = oracle.global_ic_inverse(*ins, z, dtype=dt, f32_quarter_turn=True, **sw)      # (the reference's f32 pi/2)
            outs = oracle.global_ic_forward(xin.astype(dt), z, dtype=dt, **sw)
        else:
            wh = bl = None
            if C.kind(mol) == "mixed":
                wh = (G["ala2.wh_mean"], G["ala2.wh_Twhiten"], float(G["ala2.wh_jac"]))
                bl = (G["ala2.wh_mean"], G["ala2.wh_Tblacken"], float(G["ala2.wh_jac"]))
            x, dli = oracle.ic_ic2xyz(*ins, z, fixed, blacken=bl, dtype=dt, **sw)
            outs = oracle.ic_xyz2ic(xin.astype(dt), z, fixed, whiten=wh, dtype=dt, **sw)
        _check(G, mol, sname, "x", x, x_ref, sfx, failures)
        _check(G, mol, sname, "dlogp_inv", dli, G[key + "dlogp_inv"], sfx, failures)
        for k, v in zip(C.names(mol) + ["dlogp"], outs):
            _check(G, mol, sname, f"f_{k}", v, G[key + f"f_{k}"], sfx, failures)
        if C.kind(mol) != "glob":
            free = ~G[key + "clamped_inv"][rec]
            assert free.sum() >= 3
            gx = C.weight(G, mol, "x", rec)
            grads = oracle.ic_ic2xyz_backward(*ins[:3], x_ref, gx, G[f"{mol}.wl_inv"][rec], z, fixed,
                                              normalize_angles=sw["normalize_angles"], blacken=bl, dtype=dt)
            for k, g in zip(C.names(mol), grads):
                want = G[key + f"gi_{k}"]
                err = C.error(g, want, k, sname)[free]
                bound = 1e-10 * np.abs(want).max() if sfx == "64" else C.bound32(G, mol, sname, f"gi_{k}", want)
                if not C.report(f"{key}gi_{k} (f{sfx}, C sweep, unclamped rows)", err, bound) <= 1.0:
                    failures.append((f"gi_{k}", sfx))
    assert not failures, failures


@pytest.mark.parametrize("mol,sname", [c for c in C.CASES if C.kind(c[0]) != "glob"])
def test_torch_restatements(G, mol, sname):
    """ic2xyz_torch and xyz2ic_torch: values, log-dets and the autograd gradients of the fixture's loss w.r.t. every input of both
    directions -- clamped samples included (autograd sees clamp's derivative like the reference's)"""
    key, rec = f"{mol}.{sname}.", G["rec"]
    failures = []
    for dt, sfx in ((torch.float64, "64"), (torch.float32, "32")):
        res = C.restated(G, mol, sname, dt, rows=rec, xin=G[key + "xin"])
        res.pop("xin")
        for k, v in res.items():
            _check(G, mol, sname, k, v, G[key + k], sfx, failures)
    assert not failures, failures


def test_torch_restatement_batch_of_one(G):
    res = C.restated(G, "hub12", "default", torch.float64, rows=slice(0, 1), xin=G["hub12.default.b1_xin"])
    res.pop("xin")
    for k, v in res.items():
        want = G[f"hub12.default.b1_{k}"]
        assert C.error(v, want, k, "default").max() <= 1e-10 * np.abs(want).max(), k


@pytest.mark.parametrize("sname", list(C.SETS))
def test_torch_restatements_on_the_relative_part_of_the_global_molecule(G, sname):
    """the global transformation = reference system + relative part; the torch restatements cover the relative part: its values from the
    recorded positions of the three initial atoms (log-dets and gradients pass through the reference system, which only the C oracle restates)"""
    import bgflow_amd as bg
    from oracle import torch_flow as tf
    key, rec = f"glob12.{sname}.", G["rec"]
    rel = C.make(G, "glob12", sname)._rel_ic
    b, a, t, _, _ = [torch.tensor(np.asarray(v)[rec], dtype=torch.float64) for v in C.inputs(G, "glob12", sname)]
    x_ref = torch.tensor(G[key + "x"])
    x_init = x_ref.reshape(len(rec), -1, 3)[:, G["glob12.fixed"].astype(np.int64)].reshape(len(rec), 9)
    x, _ = tf.ic2xyz_torch(rel, b[:, 2:], a[:, 1:], t, x_init)
    assert float((x - x_ref).abs().max()) <= 1e-10 * float(x_ref.abs().max())
    bo, ao, to, _, _ = tf.xyz2ic_torch(rel, torch.tensor(G[key + "xin"], dtype=torch.float64))
    for got, k, cut in ((bo, "f_bonds", 2), (ao, "f_angles", 1), (to, "f_torsions", 0)):
        want = G[key + k][:, cut:]
        assert C.error(got.numpy(), want, k, sname).max() <= 1e-10 * np.abs(want).max(), k
    assert isinstance(rel, bg.RelativeInternalCoordinateTransformation)
