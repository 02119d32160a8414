"""GPU (-m gpu): ``MolecularMechanicsEnergy`` on csrc/bgk_molecule.hip against the yardstick's f64 run (tests/golden/molecule.npz, written
by tests/golden/make_molecule_goldens.py) and bitwise against itself.

Parity bound, the project's bound for every kernel: err <= 4 err_v32 + 1e-6 with err_v32 the error of the yardstick's own f32 run on the
same rows, separately over the 146 bulk rows and each of the four special rows (a 0.01 nm contact, an angle and a torsion within 5e-4 rad of
pi, the molecule at +50 nm); the energy by |u - u64| / (1 + |u64|), the gradient of sum_b a_b u_b scaled by the row,
|g - g64| / (1 + max_row |g64|) (tests/molecule_common.py).  All 150 rows are compared.  B = 150: a partial last tile and three workgroups
(five in the backward of chain64, whose tiles have 32 rows).  Every test first asserts that its case takes the kernel."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
import molecule_common as mm
from bgflow_amd import molecule
from bgflow_amd.distributions import MoleculePlan, _kernel_plan, kl_loss_sums

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("molecule")


@pytest.fixture(scope="module")
def cases(hip_lib, dev):
    """name -> (the energy on the device, x [150, 3 n], a [150]), built once"""
    out = {}
    for name in mm.CASES:
        inp = mm.inputs(name)
        out[name] = (bg.MolecularMechanicsEnergy.from_arrays(mm.case(name)[0]).to(dev), torch.from_numpy(inp["x"]).to(dev),
                     torch.from_numpy(inp["a"]).to(dev))
    return out


@pytest.fixture(scope="module")
def results(cases):
    """name -> (u [150], gradient of sum_b a_b u_b [150, 3 n]) from the kernel, computed once (torch tensors on the device)"""
    out = {}
    for name, (energy, x, a) in cases.items():
        out[name] = u_and_gx(energy, x, a)
    return out


def takes_kernel(energy, x, temperature=1.0):
    plan = _kernel_plan(energy, temperature)
    assert isinstance(plan, MoleculePlan), "the case must describe itself to the kernel"
    assert molecule._kernel_operands(plan, (x,)) is not None, "the case must take the fused path"
    return plan


def fused_energy(energy, x, temperature=1.0):
    takes_kernel(energy, x, temperature)
    u = energy.energy(x, temperature=temperature)
    if u.requires_grad:
        assert type(u.grad_fn).__name__ == "_MoleculeEnergyFnBackward"
    return u


def u_and_gx(energy, x, a, temperature=1.0):
    x = x.detach().clone().requires_grad_(True)
    u = fused_energy(energy, x, temperature)
    assert u.shape == (x.shape[0], 1) and u.dtype == torch.float32
    gx, = torch.autograd.grad((a * u[:, 0]).sum(), x)
    return u.detach()[:, 0], gx


def numpy_pair(u, g):
    return u.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("name", mm.CASES)
def test_parity_with_the_yardstick(results, G, name):
    u, g = numpy_pair(*results[name])
    assert np.isfinite(u).all() and np.isfinite(g).all()
    mm.assert_within(mm.errors(u, g, G, name), G, name, what="kernel ")


@pytest.mark.parametrize("name", mm.CASES)
def test_force_is_minus_the_gradient(cases, name):
    energy, x, _ = cases[name]
    takes_kernel(energy, x)
    _, gx = u_and_gx(energy, x, torch.ones_like(x[:, 0]))
    f = energy.force(x)
    assert torch.equal(f, -gx) and not x.requires_grad


def loss_tolerance(G, name, rows_dlogp, scale=1.0):
    """what the sum over the rows of (u_b - dlogp_b) may miss the f64 sum by: every row's own bound on u, plus an f32 rounding of the row's
    difference (the kernel forms u - dlogp in f32; the sum itself is in f64)"""
    u64 = G[f"{name}_u64"] * scale
    tol = 0.0
    for cls, rows in mm.CLASSES:
        tol += mm.bound(G, name, "u", cls) * (1.0 + np.abs(u64[rows])).sum()
    return tol + 2.0 ** -24 * np.abs(u64 - rows_dlogp).sum()


@pytest.mark.parametrize("name", mm.CASES)
def test_kl_loss_sums(cases, results, G, name):
    energy, x, _ = cases[name]
    takes_kernel(energy, x)
    u_ref, _ = results[name]
    torch.manual_seed(5)
    dlogp = torch.randn(mm.B, 1, device=x.device)
    xg, dl = x.detach().clone().requires_grad_(True), dlogp.clone().requires_grad_(True)
    out = kl_loss_sums(energy, (xg,), dl, drop_nonfinite=True)
    assert out is not None
    sums, u = out
    assert sums.dtype == torch.float64 and sums.shape == (2,) and type(sums.grad_fn).__name__ == "_MoleculeKLSumsFnBackward"
    assert torch.equal(u.detach()[:, 0], u_ref) and float(sums.detach()[1]) == mm.B
    sums_v = sums.detach()
    want = float((G[f"{name}_u64"] - dlogp[:, 0].double().cpu().numpy()).sum())
    tol = loss_tolerance(G, name, dlogp[:, 0].double().cpu().numpy())
    print(f"{name}: loss sum {float(sums_v[0]):.10g}, f64 {want:.10g}, error {abs(float(sums_v[0]) - want):.3g}, tolerance {tol:.3g}")
    assert abs(float(sums_v[0]) - want) <= tol
    # the 146 bulk rows alone (the contact row's 1e15..1e17 hides them in the sum over all rows)
    bulk = torch.as_tensor(mm.BULK, device=x.device)
    sums_b, u_b = kl_loss_sums(energy, (x[bulk].contiguous(),), dlogp[bulk].contiguous(), drop_nonfinite=True)
    dl_b = dlogp[bulk, 0].double().cpu().numpy()
    want_b = float((G[f"{name}_u64"][mm.BULK] - dl_b).sum())
    tol_b = mm.bound(G, name, "u", "bulk") * (1.0 + np.abs(G[f"{name}_u64"][mm.BULK])).sum() + 2.0 ** -24 * np.abs(G[f"{name}_u64"][mm.BULK] - dl_b).sum()
    print(f"{name}: bulk loss sum {float(sums_b[0]):.10g}, f64 {want_b:.10g}, error {abs(float(sums_b[0]) - want_b):.3g}, tolerance {tol_b:.3g}")
    assert float(sums_b[1]) == len(mm.BULK) and torch.equal(u_b[:, 0], u_ref[bulk]) and abs(float(sums_b[0]) - want_b) <= tol_b
    # gradients: d (sums[0] / sums[1]) / d x = (d u / d x) / B, d / d dlogp = -1 / B
    (sums[0] / sums[1]).backward()
    _, g_unit = u_and_gx(energy, x, torch.ones_like(x[:, 0]))
    assert torch.allclose(xg.grad * mm.B, g_unit, rtol=1e-6, atol=0)
    assert torch.equal(dl.grad, torch.full_like(dl, -1.0 / mm.B))
    if energy.n_pairs == 0:
        return
    # one row with two coincident atoms that interact, appended: dropped from the sums, +inf, gradient row exactly zero, the rest unchanged
    li, lj = mm.live_pairs(mm.case(name)[0])[:2]
    i, j = int(li[0]), int(lj[0])
    extra = x[7:8].clone()
    extra[0, 3 * j:3 * j + 3] = extra[0, 3 * i:3 * i + 3]
    x2 = torch.cat([x, extra]).requires_grad_(True)
    dl2 = torch.cat([dlogp, dlogp[:1]]).requires_grad_(True)
    sums2, u2 = kl_loss_sums(energy, (x2,), dl2, drop_nonfinite=True)
    assert float(sums2.detach()[1]) == mm.B and float(u2[-1]) == float("inf") and torch.equal(u2[:-1, 0], u_ref)
    assert float(sums2.detach()[0]) == float(sums_v[0])
    (sums2[0] / sums2[1]).backward()
    assert (x2.grad[-1] == 0).all() and float(dl2.grad[-1]) == 0.0
    assert torch.equal(x2.grad[:-1], xg.grad) and torch.equal(dl2.grad[:-1], dl.grad)
    # without drop_nonfinite the row counts and the sum is +inf
    sums3, _ = kl_loss_sums(energy, (x2.detach(),), dl2.detach(), drop_nonfinite=False)
    assert float(sums3[1]) == mm.B + 1 and float(sums3[0]) == float("inf")
    # the energy alone: +inf in that row, and a finite gradient everywhere (the pair contributes none)
    ue, ge = u_and_gx(energy, x2.detach(), torch.ones(mm.B + 1, device=x.device))
    assert float(ue[-1]) == float("inf") and torch.isfinite(ge).all()


@pytest.mark.parametrize("name", mm.CASES)
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


@pytest.mark.parametrize("name", mm.CASES)
def test_temperature_and_unit_energy(cases, G, name):
    _, x, a = cases[name]
    scaled = bg.MolecularMechanicsEnergy.from_arrays({**mm.case(name)[0], "unit_energy": np.array(2.494)}).to(x.device)
    takes_kernel(scaled, x, 2.5)
    u, g = numpy_pair(*u_and_gx(scaled, x, a, temperature=2.5))
    mm.assert_within(mm.errors(u, g, G, name, scale=1.0 / (2.494 * 2.5)), G, name, what="kernel, T = 2.5, kT = 2.494: ")


@pytest.mark.parametrize("name", ["butane4", "ala2"])
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
    # f64
    assert molecule._kernel_operands(plan, (x.double(),)) is None
    u, g = mm.evaluate(energy, x.double(), a.double())
    assert u.dtype == np.float64
    for key, err in mm.errors(u, g, G, name).items():
        assert err <= 1e-10, (name, key, err)
    # create_graph: the forward is the kernel's, the gradient comes from the torch formulas and can be differentiated again
    xg = x.detach().clone().requires_grad_(True)
    u = fused_energy(energy, xg)
    g, = torch.autograd.grad((a * u[:, 0]).sum(), xg, create_graph=True)
    assert g.requires_grad and torch.equal(u.detach()[:, 0], results[name][0])
    mm.assert_within(mm.errors(*numpy_pair(u.detach()[:, 0], g.detach()), G, name), G, name, what="create_graph: ")
    h, = torch.autograd.grad((g[mm.BULK] ** 2).sum(), xg)
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def test_wrappers_work_around_the_energy(cases, results):
    energy, x, _ = cases["butane4"]
    takes_kernel(energy, x)
    u = results["butane4"][0]
    cut = bg.LinLogCutEnergy(energy, 100.0, 1e9)
    assert torch.isfinite(cut.energy(x)).all() and torch.equal(cut.energy(x)[u < 100.0, 0], u[u < 100.0])


def test_kl_trainer_step_onto_butane(cases, dev, monkeypatch):
    energy, x, _ = cases["butane4"]
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
    calls = []
    original = molecule.molecule_kl_loss_sums
    monkeypatch.setattr(molecule, "molecule_kl_loss_sums", lambda *a, **k: calls.append(1) or original(*a, **k))
    torch.manual_seed(0)
    prior = bg.NormalDistribution(dim, torch.from_numpy(mm.case("butane4")[1].reshape(-1)).float())
    gen = bg.BoltzmannGenerator(prior, flow, energy).to(dev)
    before = [p.detach().clone() for p in gen.flow.parameters()]
    trainer = bg.KLTrainer(gen, optim=torch.optim.Adam(gen.flow.parameters(), lr=1e-3), train_likelihood=False)
    trainer.train(1, batchsize=256)
    assert calls, "the KL step must take the fused loss path"
    assert np.isfinite(trainer.losses()[2][0]).all()
    after = list(gen.flow.parameters())
    assert all(torch.isfinite(p).all() for p in after) and any(not torch.equal(p.detach(), q) for p, q in zip(after, before))
