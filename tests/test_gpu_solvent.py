"""GPU (-m gpu): the implicit solvent (GBSA-OBC) of ``MolecularMechanicsEnergy`` on the solvent kernels of csrc/bgk_molecule.hip against the
yardstick's f64 run (tests/golden/solvent.npz, written by tests/golden/make_solvent_goldens.py) and bitwise against itself.

Parity bound, the project's bound for every kernel: err <= 4 err_v32 + 1e-6 with err_v32 the error of the yardstick's own f32 run on the
same rows, separately over the 146 bulk rows and each of the four special rows; measures as in tests/molecule_common.py.  B = 150: a
partial last tile and three workgroups at 64 rows per tile; chain64_gb runs 32 rows per tile forward (five workgroups) and 16 backward
(ten).  Every test first asserts that its case takes the kernel."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
import molecule_common as mm
import solvent_common as sc
from bgflow_amd import _lib, molecule
from bgflow_amd.distributions import kl_loss_sums
from test_gpu_molecule import fused_energy, loss_tolerance, numpy_pair, takes_kernel, u_and_gx

pytestmark = pytest.mark.gpu
ALL = sc.CASES + [sc.EXTRA]


@pytest.fixture(scope="module")
def G(golden):
    return golden("solvent")


@pytest.fixture(scope="module")
def cases(hip_lib, dev):
    """name -> (the energy on the device, x [150, 3 n], a [150]), built once"""
    out = {}
    for name in ALL:
        inp = sc.inputs(name)
        out[name] = (bg.MolecularMechanicsEnergy.from_arrays(sc.case(name)[0]).to(dev), torch.from_numpy(inp["x"]).to(dev),
                     torch.from_numpy(inp["a"]).to(dev))
        assert out[name][0].has_solvent
    return out


@pytest.fixture(scope="module")
def results(cases):
    """name -> (u [150], gradient of sum_b a_b u_b [150, 3 n]) from the kernel, computed once"""
    return {name: u_and_gx(energy, x, a) for name, (energy, x, a) in cases.items()}


@pytest.mark.parametrize("name", ALL)                          # (the last: solute dielectric 2, no surface term)
def test_parity_with_the_yardstick(results, G, name):
    u, g = numpy_pair(*results[name])
    assert np.isfinite(u).all() and np.isfinite(g).all()
    mm.assert_within(mm.errors(u, g, G, name), G, name, what="kernel ")


@pytest.mark.parametrize("name", sc.CASES)
def test_force_is_minus_the_gradient(cases, name):
    energy, x, _ = cases[name]
    takes_kernel(energy, x)
    _, gx = u_and_gx(energy, x, torch.ones_like(x[:, 0]))
    f = energy.force(x)
    assert torch.equal(f, -gx) and not x.requires_grad


@pytest.mark.parametrize("name", sc.CASES)
def test_kl_loss_sums(cases, results, G, name):
    energy, x, _ = cases[name]
    takes_kernel(energy, x)
    u_ref, _ = results[name]
    torch.manual_seed(5)
    dlogp = torch.randn(mm.B, 1, device=x.device)
    dl_np = dlogp[:, 0].double().cpu().numpy()
    for drop in (True, False):
        xg, dl = x.detach().clone().requires_grad_(True), dlogp.clone().requires_grad_(True)
        sums, u = kl_loss_sums(energy, (xg,), dl, drop_nonfinite=drop)
        assert sums.dtype == torch.float64 and sums.shape == (2,) and type(sums.grad_fn).__name__ == "_MoleculeKLSumsFnBackward"
        assert torch.equal(u.detach()[:, 0], u_ref) and float(sums.detach()[1]) == mm.B
        want = float((G[f"{name}_u64"] - dl_np).sum())
        tol = loss_tolerance(G, name, dl_np)
        print(f"{name} drop {drop}: loss sum {float(sums[0]):.10g}, f64 {want:.10g}, error {abs(float(sums[0]) - want):.3g}, tolerance {tol:.3g}")
        assert abs(float(sums[0]) - want) <= tol
    # the 146 bulk rows alone (the contact row hides them in the sum over all rows)
    bulk = torch.as_tensor(mm.BULK, device=x.device)
    sums_b, u_b = kl_loss_sums(energy, (x[bulk].contiguous(),), dlogp[bulk].contiguous(), drop_nonfinite=True)
    u64_b = G[f"{name}_u64"][mm.BULK]
    want_b = float((u64_b - dl_np[mm.BULK]).sum())
    tol_b = mm.bound(G, name, "u", "bulk") * (1.0 + np.abs(u64_b)).sum() + 2.0 ** -24 * np.abs(u64_b - dl_np[mm.BULK]).sum()
    print(f"{name}: bulk loss sum {float(sums_b[0]):.10g}, f64 {want_b:.10g}, error {abs(float(sums_b[0]) - want_b):.3g}, tolerance {tol_b:.3g}")
    assert float(sums_b[1]) == len(mm.BULK) and torch.equal(u_b[:, 0], u_ref[bulk]) and abs(float(sums_b[0]) - want_b) <= tol_b
    # gradients (of the last pass, drop_nonfinite=False): d (sums[0] / sums[1]) / d x = (d u / d x) / B, d / d dlogp = -1 / B
    (sums[0] / sums[1]).backward()
    _, g_unit = u_and_gx(energy, x, torch.ones_like(x[:, 0]))
    assert torch.allclose(xg.grad * mm.B, g_unit, rtol=1e-6, atol=0)
    assert torch.equal(dl.grad, torch.full_like(dl, -1.0 / mm.B))
    # one row with two coincident atoms appended (the contact pair): dropped from the sums, +inf, its gradient row exactly zero, the rest
    # unchanged
    i, j = sc.contact_pair(mm.case(sc.base_of(name))[0])
    extra = x[7:8].clone()
    extra[0, 3 * j:3 * j + 3] = extra[0, 3 * i:3 * i + 3]
    x2 = torch.cat([x, extra]).requires_grad_(True)
    dl2 = torch.cat([dlogp, dlogp[:1]]).requires_grad_(True)
    sums2, u2 = kl_loss_sums(energy, (x2,), dl2, drop_nonfinite=True)
    assert float(sums2.detach()[1]) == mm.B and float(u2[-1]) == float("inf") and torch.equal(u2[:-1, 0], u_ref)
    assert float(sums2.detach()[0]) == float(sums.detach()[0])
    (sums2[0] / sums2[1]).backward()
    assert (x2.grad[-1] == 0).all() and float(dl2.grad[-1]) == 0.0
    assert torch.equal(x2.grad[:-1], xg.grad) and torch.equal(dl2.grad[:-1], dl.grad)
    sums3, _ = kl_loss_sums(energy, (x2.detach(),), dl2.detach(), drop_nonfinite=False)
    assert float(sums3[1]) == mm.B + 1 and float(sums3[0]) == float("inf")
    # the energy alone: +inf in that row, and a finite gradient everywhere (the solvent terms contribute none to that row)
    ue, ge = u_and_gx(energy, x2.detach(), torch.ones(mm.B + 1, device=x.device))
    assert float(ue[-1]) == float("inf") and torch.isfinite(ge).all()


@pytest.mark.parametrize("name", sc.CASES)
def test_determinism(cases, results, name):
    energy, x, a = cases[name]
    u, g = results[name]
    u2, g2 = u_and_gx(energy, x, a)
    assert torch.equal(u2, u) and torch.equal(g2, g)
    part = x[37:101].contiguous()
    up, gp = u_and_gx(energy, part, a[37:101].contiguous())
    assert torch.equal(up, u[37:101]) and torch.equal(gp, g[37:101])
    with torch.no_grad():
        assert torch.equal(fused_energy(energy, x)[37:101], fused_energy(energy, part))
    for lo, hi in ((0, 1), (63, 150)):                       # batches of 1 and 87 rows
        ub, gb = u_and_gx(energy, x[lo:hi].contiguous(), a[lo:hi].contiguous())
        assert torch.equal(ub, u[lo:hi]) and torch.equal(gb, g[lo:hi]), (lo, hi)


@pytest.mark.parametrize("name", sc.CASES)
def test_temperature_and_unit_energy(cases, G, name):
    _, x, a = cases[name]
    scaled = bg.MolecularMechanicsEnergy.from_arrays({**sc.case(name)[0], "unit_energy": np.array(2.494)}).to(x.device)
    takes_kernel(scaled, x, 2.5)
    u, g = numpy_pair(*u_and_gx(scaled, x, a, temperature=2.5))
    mm.assert_within(mm.errors(u, g, G, name, scale=1.0 / (2.494 * 2.5)), G, name, what="kernel, T = 2.5, kT = 2.494: ")


@pytest.mark.parametrize("name", ["butane4_gb", "ala2_gb"])
def test_other_inputs_take_the_general_path(cases, results, G, name):
    energy, x, a = cases[name]
    plan = takes_kernel(energy, x)
    # strided rows
    wide = torch.full((mm.B, x.shape[1] + 5), 7.0, device=x.device)
    wide[:, :x.shape[1]] = x
    view = wide[:, :x.shape[1]]
    assert not view.is_contiguous() and molecule._kernel_operands(plan, (view,)) is None
    vg = view.detach().requires_grad_(True)
    u = energy.energy(vg)
    assert "Molecule" not in type(u.grad_fn).__name__
    g, = torch.autograd.grad((a * u[:, 0]).sum(), vg)
    mm.assert_within(mm.errors(*numpy_pair(u.detach()[:, 0], g), G, name), G, name, what="torch ops on the device, strided: ")
    # f64 on the device, and the CPU
    assert molecule._kernel_operands(plan, (x.double(),)) is None and molecule._kernel_operands(plan, (x.cpu(),)) is None
    for where, e in ((x.device, energy), (torch.device("cpu"), bg.MolecularMechanicsEnergy.from_arrays(sc.case(name)[0]))):
        u, g = mm.evaluate(e, x.double().to(where), a.double().to(where))
        assert u.dtype == np.float64
        for key, err in mm.errors(u, g, G, name).items():
            assert err <= 1e-10, (name, where, key, err)
    # create_graph: the forward is the kernel's, the gradient comes from the torch formulas and can be differentiated again
    xg = x.detach().clone().requires_grad_(True)
    u = fused_energy(energy, xg)
    g, = torch.autograd.grad((a * u[:, 0]).sum(), xg, create_graph=True)
    assert g.requires_grad and torch.equal(u.detach()[:, 0], results[name][0])
    mm.assert_within(mm.errors(*numpy_pair(u.detach()[:, 0], g.detach()), G, name), G, name, what="create_graph: ")
    h, = torch.autograd.grad((g[mm.BULK] ** 2).sum(), xg)
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def test_coincident_atoms_of_an_excluded_pair(cases, dev):
    _, x, _ = cases["butane4_gb"]
    t = sc.case("butane4_gb")[0]
    # without the bonded terms that are themselves singular where atoms 0 and 1 (a 1-2 pair, excluded) coincide
    t = {**t, "bond_idx": t["bond_idx"][1:], "bond_r0": t["bond_r0"][1:], "bond_k": t["bond_k"][1:], "angle_idx": t["angle_idx"][:0],
         "angle_theta0": t["angle_theta0"][:0], "angle_k": t["angle_k"][:0], "torsion_idx": t["torsion_idx"][:0],
         "torsion_periodicity": t["torsion_periodicity"][:0], "torsion_phase": t["torsion_phase"][:0], "torsion_k": t["torsion_k"][:0]}
    energy = bg.MolecularMechanicsEnergy.from_arrays(t).to(dev)
    vacuum = bg.MolecularMechanicsEnergy.from_arrays({k: v for k, v in t.items() if k in mm.case("butane4")[0]}).to(dev)
    x = x[:70].clone()
    x[65, 3:6] = x[65, 0:3]
    ones = torch.ones(70, device=dev)
    u, g = u_and_gx(energy, x, ones)
    uv, gv = u_and_gx(vacuum, x, ones)
    assert float(u[65]) == float("inf") and torch.isfinite(uv).all() and torch.isfinite(u[:65]).all() and torch.isfinite(u[66:]).all()
    assert torch.isfinite(g).all() and torch.equal(g[65], gv[65]) and not torch.equal(g[64], gv[64])


class _Recorder:
    """the library with every bgk_molecule_* call's name noted"""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("bgk_molecule"):
            return fn
        return lambda *a: self._names.append(name) or fn(*a)


def test_each_energy_launches_its_own_entries(cases, dev, monkeypatch):
    solvent, x, a = cases["butane4_gb"]
    vacuum = bg.MolecularMechanicsEnergy.from_arrays(mm.case("butane4")[0]).to(dev)
    takes_kernel(solvent, x), takes_kernel(vacuum, x)
    names, real = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _Recorder(real, names))
    dlogp = torch.zeros(mm.B, 1, device=dev)
    want = {vacuum: "bgk_molecule_energy", solvent: "bgk_molecule_solvent_energy"}
    for energy, head in want.items():
        del names[:]
        u_and_gx(energy, x, a)
        energy.force(x)
        sums, _ = kl_loss_sums(energy, (x.detach().clone().requires_grad_(True),), dlogp, drop_nonfinite=True)
        sums[0].backward()
        assert names == [head, head + "_backward", head + "_backward", head + "_kl_sums", head + "_backward"], names


def test_kl_trainer_step_onto_butane(cases, dev, monkeypatch):
    energy, x, _ = cases["butane4_gb"]
    takes_kernel(energy, x)
    dim, half = 12, 6
    layers = [bg.SplitFlow(half),
              bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.ReLU()),
                                                   scale_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.Tanh()))),
              bg.SwapFlow(),
              bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.ReLU()),
                                                   scale_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.Tanh()))),
              bg.InverseFlow(bg.SplitFlow(half))]
    flow = bg.utils.hash_init_(bg.SequentialFlow(layers))
    calls, names, real = [], [], _lib.lib()
    original = molecule.molecule_kl_loss_sums
    monkeypatch.setattr(molecule, "molecule_kl_loss_sums", lambda *a, **k: calls.append(1) or original(*a, **k))
    monkeypatch.setattr(_lib, "lib", lambda: _Recorder(real, names))
    torch.manual_seed(0)
    prior = bg.NormalDistribution(dim, torch.from_numpy(sc.case("butane4_gb")[1].reshape(-1)).float())
    gen = bg.BoltzmannGenerator(prior, flow, energy).to(dev)
    before = [p.detach().clone() for p in gen.flow.parameters()]
    trainer = bg.KLTrainer(gen, optim=torch.optim.Adam(gen.flow.parameters(), lr=1e-3), train_likelihood=False)
    trainer.train(1, batchsize=256)
    assert calls, "the KL step must take the fused loss path"
    assert names == ["bgk_molecule_solvent_energy_kl_sums", "bgk_molecule_solvent_energy_backward"], names
    assert np.isfinite(trainer.losses()[2][0]).all()
    after = list(gen.flow.parameters())
    assert all(torch.isfinite(p).all() for p in after) and any(not torch.equal(p.detach(), q) for p, q in zip(after, before))
