"""Shared by tests/test_host_ic_switches.py and tests/test_gpu_ic_switches.py: the cases of tests/golden/ic_switches.npz (written by
tests/golden/make_ic_switch_goldens.py from the unmodified reference), the transformations of bgflow_amd for them, and the f64
restatements of oracle/torch_flow.py evaluated on all 70 samples."""
import numpy as np
import torch

SETS = {
    "default": {},
    "nonorm": dict(normalize_angles=False),
    "noenf": dict(enforce_boundaries=False),
    "eps3": dict(eps=1e-3),
    "all": dict(normalize_angles=False, enforce_boundaries=False, eps=1e-3),
}
MOLS = ("hub7", "hub12", "hub23", "ala2", "glob12")
CASES = [(m, s) for m in MOLS for s in SETS]
IN_NAMES = {"rel": ["bonds", "angles", "torsions", "fixed"], "glob": ["bonds", "angles", "torsions", "x0", "R"]}


def kind(mol):
    return "glob" if mol.startswith("glob") else "mixed" if mol == "ala2" else "rel"


def names(mol):
    return IN_NAMES["glob" if kind(mol) == "glob" else "rel"]


def make(G, mol, sname, **extra):
    """the transformation of bgflow_amd for a case (host object; ``.to(dev)`` moves the buffers of the mixed one)"""
    import bgflow_amd as bg
    kw = dict(SETS[sname], **extra)
    z, fixed = G[f"{mol}.z_matrix"].astype(np.int64), G[f"{mol}.fixed"].astype(np.int64)
    if kind(mol) == "glob":
        return bg.GlobalInternalCoordinateTransformation(z, **kw)
    if kind(mol) == "mixed":
        from bgflow_amd.configs import ala2_whitening_data
        return bg.MixedCoordinateTransformation(ala2_whitening_data(torch.float64), z, fixed, keepdims=9, **kw)
    return bg.RelativeInternalCoordinateTransformation(z, fixed, **kw)


def inputs(G, mol, sname):
    """the inverse direction's inputs of a case, f32 arrays of 70 rows (radians for the normalize_angles=False sets)"""
    r = "in_" if SETS[sname].get("normalize_angles", True) else "inr_"
    pick = lambda k: G[f"{mol}.{r}{k}"] if f"{mol}.{r}{k}" in G.files else G[f"{mol}.in_{k}"]      # noqa: E731
    return [pick(k) for k in names(mol)]


def weight(G, mol, name, rows=slice(None)):
    """[B, columns] loss weights of an output"""
    return G[f"{mol}.ws"].astype(np.float64)[rows, None] * G[f"{mol}.wc_{name}"].astype(np.float64)[None]


def period(sname):
    return 1.0 if SETS[sname].get("normalize_angles", True) else 2 * np.pi


def periodic_columns(name, width):
    """columns of an output that are compared modulo the period: torsions, the Euler angles alpha and gamma"""
    if name.endswith("torsions"):
        return list(range(width))
    if name.endswith("f_R"):
        return [0, 2]
    return []


def error(got, want, name, sname):
    """|got - want| per element, modulo the period where the output is periodic"""
    got, want = np.asarray(got, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    cols = periodic_columns(name, want.shape[-1]) if want.ndim == 2 else []
    if cols:
        err[:, cols] = np.minimum(err[:, cols], period(sname) - err[:, cols])
    return err


def bound32(G, mol, sname, name, want, cap=None):
    """f32 bound of an array: 4 x the reference's own f32 deviation + 1e-6 of the largest entry, never above ``cap`` x the largest entry"""
    big = float(np.abs(want).max())
    b = 4.0 * float(G[f"{mol}.{sname}.dev_{name}"]) + 1e-6 * big
    return b if cap is None else min(b, cap * big)


def report(label, err, bound):
    """print the worst error / bound and its element; return the ratio"""
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    ratio = float(err[i]) / bound
    print(f"{label:44s} worst error {float(err[i]):.3e} = {ratio:6.3f} x bound {bound:.3e} at {tuple(int(k) for k in i)}")
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# f64 restatements on all rows (relative and mixed: values and autograd gradients of both directions)
# ---------------------------------------------------------------------------------------------------------------------------------
def forward_input(G, mol, sname, x, rows=slice(None)):
    """the forward direction's input: the inverse's f64 positions rounded to f32, the recorded samples exactly as the fixture has them"""
    xin = np.asarray(x).astype(np.float32)
    if isinstance(rows, slice) and rows == slice(None):
        xin[G["rec"]] = G[f"{mol}.{sname}.xin"]
    return xin


def restated(G, mol, sname, dtype=torch.float64, rows=slice(None), xin=None):
    """oracle/torch_flow.py's ic2xyz_torch / xyz2ic_torch for a relative or mixed case, with the fixture's loss: dict of numpy arrays with
    the fixture's keys (x, dlogp_inv, gi_*, xin, f_*, f_dlogp, gf_x); the forward runs on ``xin`` (default: forward_input of x)"""
    from oracle import torch_flow as tf
    assert kind(mol) != "glob"
    tr = make(G, mol, sname)
    ins = [torch.tensor(np.asarray(v)[rows], dtype=dtype).requires_grad_(True) for v in inputs(G, mol, sname)]
    tw = lambda a: torch.tensor(a, dtype=dtype)      # noqa: E731
    x, dli = tf.ic2xyz_torch(tr, *ins)
    loss = (x * tw(weight(G, mol, "x", rows))).sum() + (dli[:, 0] * tw(G[f"{mol}.wl_inv"][rows])).sum()
    gi = torch.autograd.grad(loss, ins)
    res = {"x": x, "dlogp_inv": dli}
    res.update({f"gi_{k}": g for k, g in zip(names(mol), gi)})
    if xin is None:
        xin = forward_input(G, mol, sname, x.detach().numpy(), rows)
    x2 = torch.tensor(xin, dtype=dtype).requires_grad_(True)
    *outs, dlf = tf.xyz2ic_torch(tr, x2)
    loss = sum((v * tw(weight(G, mol, k, rows))).sum() for k, v in zip(names(mol), outs)) + (dlf[:, 0] * tw(G[f"{mol}.wl_fwd"][rows])).sum()
    (gx,) = torch.autograd.grad(loss, x2)
    res.update({f"f_{k}": v for k, v in zip(names(mol), outs)})
    res["f_dlogp"], res["gf_x"] = dlf, gx
    res = {k: v.detach().numpy() for k, v in res.items()}
    res["xin"] = xin
    return res
