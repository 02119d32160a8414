"""The internal-coordinate kernels under the constructors' switches (normalize_angles, enforce_boundaries, eps) and on branched
Z-matrices, per element against the f64 reference of tests/golden/ic_switches.npz (make_ic_switch_goldens.py): scattered atom labels, a
hub of rows on the fixed atoms, rows out of placement order, fixed atoms that are not [0, 1, 2]; 70 samples = one tile + a tail of 6.

References.  The fixture records 16 of the 70 samples (REC) of the unmodified reference's f64 run.  For the relative and mixed
molecules the f64 restatements oracle/torch_flow.py::ic2xyz_torch / xyz2ic_torch -- which tests/test_host_ic_switches.py holds to the
fixture at 1e-10 in every case -- give all 70 samples, values and gradients; the kernels are compared with both.  For the global molecule
the C oracle gives the values of all 70 samples, the fixture the gradients of REC.

Bound per array (the form of tests/test_gpu_box.py):  4 x dev + 1e-6 x max|want|,  dev = the reference's own largest |f32 - f64| of
that array (fixture), and never looser than what tests/test_gpu_parity.py grants these kernels on ala2 (CAPS below).  Each test prints
the worst error / bound and its element per array.  Measured on an MI355X, worst error / bound over all cases: values 0.53 (ala2 x under
normalize_angles=False), IC -> xyz log-det 0.31, its gradients 0.58, xyz -> IC log-det 0.71 (hub7, a sample at the edge of the cos clamp,
where acos near 1 costs f32 its digits: 4.6e-5 of the 6.5e-5 that 1e-5 |log-det| allows), its gradient 0.94 (glob12 without normalisation).
No array needed more than the 4 x bound, so no set is held to a measured ratio.

The forward direction runs on the inverse's f64 positions rounded to f32 -- in the fixture's f64 and f32 runs and here alike, so that
dev and the kernels' errors are those of the forward's arithmetic and not of the rounding of its input.
"""
import warnings

import numpy as np
import pytest
import torch

import ic_switches_common as C

pytestmark = pytest.mark.gpu

# what tests/test_gpu_parity.py grants on ala2: values 3e-6 absolute, log-dets 1e-5 relative, xyz -> IC gradients 5e-4 and global
# gradients 1e-3 of the largest entry
VALUE_CAP, LOGDET_CAP, XGRAD_CAP, GLOBAL_GRAD_CAP = 3e-6, 1e-5, 5e-4, 1e-3


@pytest.fixture(scope="module")
def G(golden):
    return golden("ic_switches")


_REF = {}


def _reference(G, oracle, mol, sname):
    """f64 reference of all 70 samples (computed once per case): the torch restatements, or the C oracle's values for the global molecule"""
    if (mol, sname) in _REF:
        return _REF[(mol, sname)]
    if C.kind(mol) != "glob":
        ref = C.restated(G, mol, sname)
    else:
        kw = C.SETS[sname]
        sw = dict(normalize_angles=kw.get("normalize_angles", True), eps=kw.get("eps", 1e-7), enforce_boundaries=kw.get("enforce_boundaries", True))
        z = G[f"{mol}.z_matrix"]
        x, dli = oracle.global_ic_inverse(*C.inputs(G, mol, sname), z, dtype=np.float64, f32_quarter_turn=True, **sw)
        xin = C.forward_input(G, mol, sname, x)
        outs = oracle.global_ic_forward(xin, z, dtype=np.float64, **sw)
        ref = {"x": x, "dlogp_inv": dli, "xin": xin}
        ref.update({f"f_{k}": v for k, v in zip(C.names(mol) + ["dlogp"], outs)})
    _REF[(mol, sname)] = ref
    return ref


def _bound(G, mol, sname, name, want):
    """4 x dev + 1e-6 x max|want|, capped by what test_gpu_parity.py grants"""
    big = float(np.abs(want).max())
    b = C.bound32(G, mol, sname, name, want)
    if name in ("dlogp_inv", "f_dlogp"):
        return min(b, LOGDET_CAP * big)
    if name.startswith("g"):
        if C.kind(mol) == "glob":
            return min(b, GLOBAL_GRAD_CAP * big)
        return min(b, XGRAD_CAP * big) if name == "gf_x" else b
    if name == "f_fixed" and C.kind(mol) == "mixed":
        return b      # the whitened block: test_gpu_parity.py sets no bound on it (entries of Twhiten reach 1 / the smallest kept std)
    # angles and torsions: the cap in normalised units (what test_gpu_parity.py compares); the same numbers in radians are pi / 2 pi times larger
    unit = 1.0
    if not C.SETS[sname].get("normalize_angles", True):
        unit = np.pi if name == "f_angles" else 2 * np.pi if (name == "f_torsions" or name == "f_R") else 1.0
    return min(b, VALUE_CAP * unit)


def _compare(G, oracle, mol, sname, got, failures, rows=None):
    """every array of ``got`` against the 70-sample reference and against the fixture's recorded samples"""
    ref, key, rec = _reference(G, oracle, mol, sname), f"{mol}.{sname}.", G["rec"]
    for name, v in got.items():
        v = v.detach().cpu().numpy().astype(np.float64)
        fix = G[key + name]
        bound = _bound(G, mol, sname, name, ref[name] if name in ref else fix)
        if name in ref:
            r = C.report(f"{key}{name} (70 samples)", C.error(v, ref[name], name, sname), bound)
            if not r <= 1.0:
                failures.append((name, "restatement", round(r, 3)))
        r = C.report(f"{key}{name} (fixture rows)", C.error(v.reshape(len(v), -1)[rec].reshape(fix.shape), fix, name, sname), bound)
        if not r <= 1.0:
            failures.append((name, "fixture", round(r, 3)))


def _loss(G, mol, outs, out_names, dl, wl, dev):
    tw = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)      # noqa: E731
    return sum((v.reshape(v.shape[0], -1) * tw(C.weight(G, mol, k))).sum() for k, v in zip(out_names, outs)) + (dl[:, 0] * tw(G[f"{mol}.{wl}"])).sum()


def _rel(tr):
    return getattr(tr, "_rel_ic", tr)


def _fixup_samples(rel, dev, B):
    """the samples that the last bgk_ic_ic2xyz_backward of ``rel`` listed for its dual-number launch"""
    buf = rel._fixup_list(dev, B).cpu().numpy()
    assert 0 <= buf[0] <= B
    return np.sort(buf[1:1 + buf[0]])


def _poll(rel, eps):
    """(clamp events since the last poll, the warning's text or None)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        total = rel.check_singularities()
    assert len(w) == (1 if total else 0)
    if total:
        assert f"eps={eps}" in str(w[0].message), str(w[0].message)
    return total


@pytest.mark.parametrize("mol,sname", C.CASES)
def test_values_logdets_and_gradients(hip_lib, oracle, dev, G, mol, sname):
    """both directions of the Relative (hub7 / 12 / 23), Mixed (ala2) and Global (glob12) transformations under every switch set: values,
    log-dets and -- through autograd with the fixture's loss weights -- both backward kernels (bgk_ic_ic2xyz_backward with its dual-number
    fix-up launch on the clamped samples, bgk_ic_xyz2ic_backward, bgk_ic_refsys_backward in both directions), per element.  The fix-up
    list holds exactly the fixture's clamped samples (none under enforce_boundaries=False); check_singularities() is positive exactly
    where the fixture has a quantity below eps (the reference's warning condition; the forward's includes x^2 + y^2 of the torsions,
    which at eps = 1e-3 is below eps in every sample), and its warning names the constructor's eps."""
    key, eps = f"{mol}.{sname}.", C.SETS[sname].get("eps", 1e-7)
    tr = C.make(G, mol, sname).to(dev)
    rel = _rel(tr)
    failures = []
    # IC -> xyz
    ins = [torch.tensor(v, device=dev).requires_grad_(True) for v in C.inputs(G, mol, sname)]
    B = ins[0].shape[0]
    x, dli = tr(*ins, inverse=True)
    _loss(G, mol, [x], ["x"], dli, "wl_inv", dev).backward()
    got = {"x": x, "dlogp_inv": dli}
    got.update({f"gi_{k}": v.grad for k, v in zip(C.names(mol), ins)})
    _compare(G, oracle, mol, sname, got, failures)
    listed, clamped = _fixup_samples(rel, dev, B), np.where(G[key + "clamped_inv"])[0]
    assert np.array_equal(listed, clamped), (listed, clamped)
    assert (len(listed) > 0) == (sname == "eps3")
    assert (_poll(rel, eps) > 0) == bool(G[key + "below_inv"].any())
    # xyz -> IC on the f64 reference's positions rounded to f32 (the input of the reference's forward too)
    x_in = torch.tensor(_reference(G, oracle, mol, sname)["xin"], device=dev).requires_grad_(True)
    *outs, dlf = tr(x_in)
    _loss(G, mol, outs, C.names(mol), dlf, "wl_fwd", dev).backward()
    got = {f"f_{k}": v for k, v in zip(C.names(mol), outs)}
    got.update({"f_dlogp": dlf, "gf_x": x_in.grad})
    _compare(G, oracle, mol, sname, got, failures)
    assert (_poll(rel, eps) > 0) == bool((G[key + "below_fwd"] | G[key + "xysq_below_fwd"]).any())
    assert not failures, failures


def test_batch_of_one(hip_lib, oracle, dev, G):
    """B = 1 against the fixture's own B = 1 record (hub12, defaults), the bounds of the 70-sample case"""
    mol, sname = "hub12", "default"
    tr = C.make(G, mol, sname).to(dev)
    ins = [torch.tensor(v[:1], device=dev).requires_grad_(True) for v in C.inputs(G, mol, sname)]
    x, dli = tr(*ins, inverse=True)
    tw = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)      # noqa: E731
    ((x * tw(C.weight(G, mol, "x", slice(0, 1)))).sum() + (dli[:, 0] * tw(G[f"{mol}.wl_inv"][:1])).sum()).backward()
    got = {"x": x, "dlogp_inv": dli}
    got.update({f"gi_{k}": v.grad for k, v in zip(C.names(mol), ins)})
    x_in = torch.tensor(G[f"{mol}.{sname}.b1_xin"], device=dev).requires_grad_(True)
    *outs, dlf = tr(x_in)
    (sum((v * tw(C.weight(G, mol, k, slice(0, 1)))).sum() for k, v in zip(C.names(mol), outs)) + (dlf[:, 0] * tw(G[f"{mol}.wl_fwd"][:1])).sum()).backward()
    got.update({f"f_{k}": v for k, v in zip(C.names(mol), outs)})
    got.update({"f_dlogp": dlf, "gf_x": x_in.grad})
    for name, v in got.items():
        want = G[f"{mol}.{sname}.b1_{name}"]
        bound = _bound(G, mol, sname, name, G[f"{mol}.{sname}.{name}"])
        assert C.report(f"{mol}.{sname}.b1_{name}", C.error(v.detach().cpu().numpy(), want, name, sname), bound) <= 1.0, name


@pytest.mark.parametrize("sname", ["nonorm", "eps3"])
def test_inputs_that_are_slices_of_wider_tensors(hip_lib, dev, G, sname):
    """hub23 with every input a column slice of a wider tensor that starts 4 bytes past a 16-byte boundary (row stride = width + 5
    floats), at B = 70 and B = 1: outputs and gradients bitwise equal to the contiguous run, the padding columns untouched"""
    mol, PAD = "hub23", 123.0
    tr = C.make(G, mol, sname).to(dev)

    def run(arrs, x_arr, sliced):
        leaves, views = [], []
        for v in list(arrs) + [x_arr]:
            v = torch.tensor(v, device=dev)
            if sliced:
                wide = torch.full((v.shape[0], v.shape[1] + 5), PAD, device=dev)
                assert wide.data_ptr() % 16 == 0
                wide[:, 1:1 + v.shape[1]] = v
                wide.requires_grad_(True)
                view = wide[:, 1:1 + v.shape[1]]
                assert view.data_ptr() % 16 == 4 and view.stride(0) == v.shape[1] + 5
            else:
                wide = view = v.requires_grad_(True)
            leaves.append(wide)
            views.append(view)
        x, dli = tr(*views[:4], inverse=True)
        ((0.5 * x).sum() + dli.sum()).backward()
        *outs, dlf = tr(views[4])
        (sum(o.sum() for o in outs) + 0.1 * dlf.sum()).backward()
        res = [x, dli, *outs, dlf] + [(lf.grad[:, 1:1 + vw.shape[1]] if sliced else lf.grad) for lf, vw in zip(leaves, views)]
        if sliced:
            for lf, vw in zip(leaves, views):
                w = vw.shape[1]
                assert bool((lf.detach()[:, :1] == PAD).all()) and bool((lf.detach()[:, 1 + w:] == PAD).all()), "padding overwritten"
                assert bool((lf.grad[:, :1] == 0).all()) and bool((lf.grad[:, 1 + w:] == 0).all())
        return [r.detach().clone() for r in res]

    arrs = C.inputs(G, mol, sname)
    x_arr = C.restated(G, mol, sname)["xin"]
    for rows in (slice(None), slice(1, 2)):                      # (sample 1 has a clamped placement at eps = 1e-3)
        a = run([v[rows] for v in arrs], x_arr[rows], False)
        b = run([v[rows] for v in arrs], x_arr[rows], True)
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (sname, rows, k, float((u - v).abs().max()))


def _tail_flow(G, mol, sname, dev):
    """[icdf map per field, IC -> xyz] like tests/test_gpu_round3.py::test_tail_and_head_on_other_molecule_sizes, marginals in the units of
    the switch set"""
    import bgflow_amd as bg
    from bgflow_amd import configs
    ic = C.make(G, mol, sname)
    n = len(G[f"{mol}.z_matrix"])
    rad = not C.SETS[sname].get("normalize_angles", True)
    one = lambda v, m: torch.full((m,), float(v))          # noqa: E731
    fixed = (configs._NormalMarginal(torch.zeros(9), one(0.5, 9)) if C.kind(mol) == "mixed"
             else configs._NormalMarginal(torch.tensor([0, 0, 0, 0.15, 0, 0, 0.2, 0.14, 0.0]), one(0.005, 9)))
    a_scale = np.pi if rad else 1.0
    marginals = {
        0: bg.TruncatedNormalDistribution(mu=one(0.15, n), sigma=one(0.01, n), lower_bound=torch.tensor(1e-5), upper_bound=torch.tensor(np.inf)),
        1: bg.TruncatedNormalDistribution(mu=one(0.5 * a_scale, n), sigma=one(0.05 * a_scale, n), lower_bound=torch.tensor(1e-5),
                                          upper_bound=torch.tensor(1.0 * a_scale)),
        2: configs.SloppyUniform(low=one(-np.pi if rad else 0.0, n), high=one(np.pi if rad else 1.0, n)),
        3: fixed,
    }
    return bg.SequentialFlow([bg.WrapFlow(bg.InverseFlow(bg.CDFTransform(marginals[s_])), (s_,)) for s_ in range(4)]
                             + [bg.WrapFlow(bg.InverseFlow(ic), indices=[0, 1, 2, 3], out_indices=(0,))]).to(dev), n


def _tail_runs(flow, xs):
    with torch.no_grad():
        x, dl = flow(*xs)
        *zs, dli = flow(x, inverse=True)
        flow.FUSE_GENERATION_TAIL = False
        x_b, dl_b = flow(*xs)
        *zs_b, dli_b = flow(x, inverse=True)
        flow.FUSE_GENERATION_TAIL = True
    return (x, dl, zs, dli), (x_b, dl_b, zs_b, dli_b)


@pytest.mark.parametrize("sname", ["noenf", "eps3"])
@pytest.mark.parametrize("mol", ["hub23", "ala2"])
def test_fused_tails_take_eps_and_enforce(hip_lib, dev, G, mol, sname):
    """the fused sampling tail and inference head (bgk_tail.hip) receive eps and enforce_boundaries: the four-map + IC flow fused
    against the same flow on its blocks (whose IC stage the tests above hold to the fixture), both directions, with the tolerances of
    test_tail_and_head_on_other_molecule_sizes; the period of the compared torsions is 1 (normalised units)"""
    flow, n = _tail_flow(G, mol, sname, dev)
    assert flow._generation_tail() is not None
    n_atoms = n + len(G[f"{mol}.fixed"])
    g = torch.Generator(device=dev).manual_seed(n_atoms)
    xs = [torch.rand(77, w, device=dev, generator=g).clamp(0.02, 0.98) for w in (n, n, n, 9)]
    (x, dl, zs, dli), (x_b, dl_b, zs_b, dli_b) = _tail_runs(flow, xs)
    print(f"{mol}.{sname}: fused vs blocks  x {float((x - x_b).abs().max()):.2e}  dlogp {float((dl - dl_b).abs().max()):.2e} (|dlogp| {float(dl_b.abs().max()):.0f})  "
          f"inverse dlogp {float((dli - dli_b).abs().max()):.2e}")
    np.testing.assert_allclose(x.cpu().numpy(), x_b.cpu().numpy(), rtol=0, atol=2e-5 * n_atoms)
    np.testing.assert_allclose(dl.cpu().numpy(), dl_b.cpu().numpy(), rtol=2e-5, atol=2e-3)
    for a, b in zip(zs, zs_b):
        da = np.abs(a.cpu().numpy() - b.cpu().numpy())
        assert np.minimum(da, 1.0 - da).max() <= 2e-4
    np.testing.assert_allclose(dli.cpu().numpy(), dli_b.cpu().numpy(), rtol=1e-4, atol=2e-2)
    if sname == "eps3":      # the switch reaches the kernels: clamped placements were met (and counted) in both runs
        assert _poll(_rel(flow._blocks[-1]._flow._delegate), 1e-3) > 0


@pytest.mark.parametrize("mol", ["hub23", "ala2"])
def test_radian_flows_stay_off_the_register_tails(hip_lib, dev, G, mol):
    """normalize_angles=False: ic.py keeps the flow off the kernels of bgk_tail.hip (they take normalised units only).  What runs instead:
    in the sampling direction the first-generation fused kernel bgk_icdf_ic2xyz, which takes the switch -- held to the blocks with the
    tolerances of test_tail_and_head_on_other_molecule_sizes --, in the inference direction the blocks themselves -- bitwise the blocks' result"""
    from test_gpu_round6 import _device_kernel_names
    flow, n = _tail_flow(G, mol, "nonorm", dev)
    n_atoms = n + len(G[f"{mol}.fixed"])
    g = torch.Generator(device=dev).manual_seed(n)
    xs = [torch.rand(77, w, device=dev, generator=g).clamp(0.02, 0.98) for w in (n, n, n, 9)]
    (x, dl, zs, dli), (x_b, dl_b, zs_b, dli_b) = _tail_runs(flow, xs)

    def step():
        with torch.no_grad():
            xx, _ = flow(*xs)
            flow(xx, inverse=True)
    names = _device_kernel_names(step)
    print(sorted(set(names)))
    assert not any(k in nm for nm in names for k in ("icdf_ic2xyz_reg_kernel", "icdf_ic2xyz_uni_kernel", "xyz2ic_cdf_uni_kernel"))
    assert any("icdf_ic2xyz_kernel" in nm for nm in names) and any("ic_xyz2ic_kernel" in nm for nm in names) and any("cdf_kernel" in nm for nm in names)
    print(f"{mol}.nonorm: fused vs blocks  x {float((x - x_b).abs().max()):.2e}  dlogp {float((dl - dl_b).abs().max()):.2e}")
    np.testing.assert_allclose(x.cpu().numpy(), x_b.cpu().numpy(), rtol=0, atol=2e-5 * n_atoms)
    np.testing.assert_allclose(dl.cpu().numpy(), dl_b.cpu().numpy(), rtol=2e-5, atol=2e-3)
    for a, b in zip([*zs, dli], [*zs_b, dli_b]):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_large_molecule_xyz2ic_gradient_per_element(hip_lib, dev):
    """230 atoms (the first shrunken LDS tile) in the style of tests/test_gpu_parity.py::test_relative_ic_large_molecules: the xyz -> IC
    gradient PER ELEMENT against f64 autograd of xyz2ic_torch, for the full loss (bonds, angles, torsions, fixed block, log-det);
    bound (2e-4 + 2e-6 n_atoms) max|want| + 1e-4, which that test uses for the other direction"""
    import bgflow_amd as bg
    from oracle import torch_flow as tf
    n_atoms = 230
    rng = np.random.RandomState(n_atoms)
    z = np.zeros((n_atoms - 3, 4), dtype=np.int64)
    for k, i in enumerate(range(3, n_atoms)):
        z[k] = (i, i - 1, i - 2, i - 3) if i % 4 else (i, i - 2, i - 3, i - 4) if i >= 4 else (i, i - 1, i - 2, i - 3)
    fixed = np.array([0, 1, 2])
    B, n = 37, n_atoms - 3
    bonds = (0.15 + 0.01 * rng.randn(B, n)).astype(np.float32)
    angles = (0.5 + 0.1 * (rng.rand(B, n) - 0.5)).astype(np.float32)
    tors = rng.rand(B, n).astype(np.float32)
    xfix = (np.array([0, 0, 0, 0.15, 0, 0, 0.2, 0.14, 0], dtype=np.float32)[None] + 0.005 * rng.randn(B, 9)).astype(np.float32)
    ws = [rng.randn(B, w) for w in (n, n, n, 9)] + [0.1 * rng.randn(B, 1)]
    ic = bg.RelativeInternalCoordinateTransformation(z, fixed)
    with torch.no_grad():
        x64, _ = tf.ic2xyz_torch(ic, *[torch.tensor(v, dtype=torch.float64) for v in (bonds, angles, tors, xfix)])
    x32 = x64.float()
    xr = x32.double().requires_grad_(True)
    sum((o.reshape(B, -1) * torch.tensor(w)).sum() for o, w in zip(tf.xyz2ic_torch(ic, xr), ws)).backward()
    want = xr.grad.numpy()
    xg = x32.to(dev).requires_grad_(True)
    sum((o.reshape(B, -1) * torch.tensor(w, dtype=torch.float32, device=dev)).sum() for o, w in zip(ic.to(dev)(xg), ws)).backward()
    err = np.abs(xg.grad.cpu().numpy() - want)
    bound = (2e-4 + 2e-6 * n_atoms) * np.abs(want).max() + 1e-4
    assert C.report("230 atoms, xyz -> IC gradient", err, bound) <= 1.0
