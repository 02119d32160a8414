"""Host: ``MolecularMechanicsEnergy`` -- the general path (torch ops) against the yardstick's f64 run (tests/golden/molecule.npz, written
by tests/golden/make_molecule_goldens.py), the constructor's checks, the array round trips, the host-side packing of the kernel's
tables, the plan rules and the C entries' prototypes and argument checks.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bgflow_amd as bg
import molecule_common as mm
from bgflow_amd import _lib, configs, molecule
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols
from bgflow_amd.distributions import MoleculePlan, _kernel_plan, kernel_energy, kl_loss_sums


@pytest.fixture(scope="module")
def G(golden):
    return golden("molecule")


@pytest.fixture(scope="module")
def cases():
    """name -> (energy object, x f64 [150, 3 n], a f64 [150]), built once"""
    out = {}
    for name in mm.CASES:
        inp = mm.inputs(name)
        out[name] = (bg.MolecularMechanicsEnergy.from_arrays(mm.case(name)[0]), torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["a"]).double())
    return out


@pytest.mark.parametrize("name", mm.CASES)
def test_inputs_are_the_fixtures(G, name):
    np.testing.assert_allclose(mm.checksum(mm.inputs(name)), G[f"{name}_checksum"], rtol=1e-12)


def test_case_sizes():
    sizes = {name: bg.MolecularMechanicsEnergy.from_arrays(mm.case(name)[0]) for name in mm.CASES}
    counts = {name: (e.n_atoms, e.n_bonds, e.n_angles, e.n_torsions, e.n_pairs) for name, e in sizes.items()}
    assert counts == {"pair2": (2, 1, 0, 0, 0), "ions3": (3, 0, 0, 0, 3), "butane4": (4, 3, 2, 2, 6), "ala2": (22, 21, 20, 21, 231),
                      "chain64": (64, 63, 62, 61, 2016)}
    table = sizes["ala2"].pair_table()
    excluded = (table[:, 0] == 0) & (table[:, 2] == 0)
    assert excluded.sum() == 57 and len(sizes["ala2"].exception_idx) - 57 == 41
    assert sizes["ala2"].dim == 66 and sizes["ala2"].event_shape == torch.Size([66])


@pytest.mark.parametrize("name", mm.CASES)
def test_general_path_f64_is_the_yardstick(cases, G, name):
    energy, x, a = cases[name]
    u, g = mm.evaluate(energy, x, a)
    for key, err in mm.errors(u, g, G, name).items():
        print(name, key, err)
        assert err <= 1e-10, (name, key, err)


@pytest.mark.parametrize("name", mm.CASES)
def test_general_path_f32_within_the_bound(cases, G, name):
    energy, x, a = cases[name]
    u, g = mm.evaluate(energy, x.float(), a.float())
    assert u.dtype == np.float32 and g.dtype == np.float32
    mm.assert_within(mm.errors(u, g, G, name), G, name, what="torch f32 ")


@pytest.mark.parametrize("name", ["butane4", "ala2"])
def test_second_derivative_exists(cases, name):
    energy, x, _ = cases[name]
    x = x[:5].clone().requires_grad_(True)
    g, = torch.autograd.grad(energy.energy(x).sum(), x, create_graph=True)
    h, = torch.autograd.grad((g * g).sum(), x)
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def test_temperature_and_unit_energy(cases):
    energy, x, _ = cases["butane4"]
    u = energy.energy(x)
    assert torch.equal(energy.energy(x, temperature=2.5), u / 2.5)
    scaled = bg.MolecularMechanicsEnergy.from_arrays({**mm.case("butane4")[0], "unit_energy": np.array(2.494)})
    assert torch.allclose(scaled.energy(x), u / 2.494, rtol=1e-14, atol=0)
    assert u.shape == (mm.B, 1) and energy.energy(x.reshape(3, 50, 12)).shape == (3, 50, 1)
    f = energy.force(x)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(f, -torch.autograd.grad(energy.energy(xg).sum(), xg)[0]) and not x.requires_grad


def test_coincident_atoms_give_plus_infinity():
    energy = bg.MolecularMechanicsEnergy.from_arrays(mm.case("ions3")[0])
    x = torch.from_numpy(mm.inputs("ions3")["x"][:4]).double()
    x[1, 3:6] = x[1, 0:3]                                    # atoms 0 and 1 (charges +1, -1): -inf + inf would be NaN
    x = x.requires_grad_(True)
    u = energy.energy(x)
    assert float(u.detach()[1]) == float("inf") and torch.isfinite(u[[0, 2, 3]]).all()
    g, = torch.autograd.grad(u[[0, 2, 3]].sum(), x)
    assert torch.isfinite(g).all() and (g[1] == 0).all()
    # an excluded pair may coincide
    t = mm.case("butane4")[0]
    energy = bg.MolecularMechanicsEnergy.from_arrays({**t, "bond_idx": t["bond_idx"][1:], "bond_r0": t["bond_r0"][1:], "bond_k": t["bond_k"][1:],
                                                      "angle_idx": t["angle_idx"][:0], "angle_theta0": t["angle_theta0"][:0],
                                                      "angle_k": t["angle_k"][:0], "torsion_idx": t["torsion_idx"][:0],
                                                      "torsion_periodicity": t["torsion_periodicity"][:0], "torsion_phase": t["torsion_phase"][:0],
                                                      "torsion_k": t["torsion_k"][:0]})
    x = torch.from_numpy(mm.inputs("butane4")["x"][:2]).double()
    x[0, 3:6] = x[0, 0:3]                                    # atoms 0 and 1: a 1-2 pair
    assert torch.isfinite(energy.energy(x)).all()


def _args(**over):
    kw = dict(n_atoms=4, bonds=(np.array([[0, 1], [1, 2]]), np.array([0.1, 0.15]), np.array([1.0, 2.0])),
              angles=(np.array([[0, 1, 2]]), np.array([1.9]), np.array([3.0])),
              torsions=(np.array([[0, 1, 2, 3]]), np.array([3]), np.array([0.5]), np.array([2.0])),
              nonbonded=(np.zeros(4), np.full(4, 0.3), np.full(4, 0.2)),
              exceptions=(np.array([[0, 1], [0, 2]]), np.zeros(2), np.full(2, 0.3), np.zeros(2)))
    kw.update(over)
    return kw


def test_constructor_validation_names_the_term():
    bg.MolecularMechanicsEnergy(**_args())
    bg.MolecularMechanicsEnergy(3)                                         # every term group is optional
    bad = [
        (dict(bonds=(np.array([[0, 1], [1, 4]]), np.array([0.1, 0.15]), np.array([1.0, 2.0]))), "bond term 1"),              # index range
        (dict(bonds=(np.array([[0, 1], [-1, 2]]), np.array([0.1, 0.15]), np.array([1.0, 2.0]))), "bond term 1"),
        (dict(angles=(np.array([[0, 1, 0]]), np.array([1.9]), np.array([3.0]))), "angle term 0"),                            # an atom twice
        (dict(torsions=(np.array([[0, 1, 2, 1]]), np.array([3]), np.array([0.5]), np.array([2.0]))), "torsion term 0"),
        (dict(bonds=(np.array([[0, 1], [1, 2]]), np.array([0.1, 0.0]), np.array([1.0, 2.0]))), "bond term 1"),               # r0 > 0
        (dict(nonbonded=(np.zeros(4), np.array([0.3, 0.3, -0.1, 0.3]), np.full(4, 0.2))), "nonbonded atom 2"),               # sigma > 0
        (dict(exceptions=(np.array([[0, 1], [0, 2]]), np.zeros(2), np.array([0.3, 0.0]), np.zeros(2))), "exception term 1"),
        (dict(torsions=(np.array([[0, 1, 2, 3]]), np.array([0]), np.array([0.5]), np.array([2.0]))), "torsion term 0"),      # periodicity 1..6
        (dict(torsions=(np.array([[0, 1, 2, 3]]), np.array([7]), np.array([0.5]), np.array([2.0]))), "torsion term 0"),
        (dict(exceptions=(np.array([[0, 1], [1, 0]]), np.zeros(2), np.full(2, 0.3), np.zeros(2))), "exception term 1"),      # one per pair
        (dict(exceptions=(np.array([[0, 0]]), np.zeros(1), np.full(1, 0.3), np.zeros(1))), "exception term 0"),
        (dict(nonbonded=None), "exceptions need"),
        (dict(bonds=(np.array([[0, 1]]), np.array([0.1, 0.2]), np.array([1.0]))), "r0 has 2 entries"),
    ]
    for over, text in bad:
        with pytest.raises(ValueError, match=text):
            bg.MolecularMechanicsEnergy(**_args(**over))
    # several torsion terms on the same four atoms are allowed
    two = bg.MolecularMechanicsEnergy(**_args(torsions=(np.array([[0, 1, 2, 3], [0, 1, 2, 3]]), np.array([1, 3]), np.zeros(2), np.ones(2))))
    assert two.n_torsions == 2


def test_array_round_trips_are_bitwise(cases, tmp_path):
    energy, x, _ = cases["ala2"]
    arrays = energy.to_arrays()
    assert all(isinstance(v, np.ndarray) and v.dtype.kind in "if" for v in arrays.values())
    for k, v in mm.case("ala2")[0].items():
        assert arrays[k].dtype == v.dtype and np.array_equal(arrays[k], v), k
    path = tmp_path / "ala2.npz"
    energy.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(arrays) and all(z[k].dtype.kind in "if" for k in z.files)
    for other in (bg.MolecularMechanicsEnergy.from_arrays(arrays), bg.MolecularMechanicsEnergy.load(path)):
        back = other.to_arrays()
        assert set(back) == set(arrays) and all(np.array_equal(back[k], arrays[k]) and back[k].dtype == arrays[k].dtype for k in arrays)
        assert torch.equal(other.energy(x), energy.energy(x))


def test_state_dict_and_dtype(cases):
    energy, x, _ = cases["butane4"]
    state = energy.state_dict()
    assert set(state) == {f"{g}_{n}" for g, names in (("bond", ("idx", "r0", "k")), ("angle", ("idx", "theta0", "k")),
                                                     ("torsion", ("idx", "periodicity", "phase", "k")),
                                                     ("exception", ("idx", "chargeprod", "sigma", "epsilon")),
                                                     ("nonbonded", ("charge", "sigma", "epsilon"))) for n in names}
    # the tables follow the buffers: a state dict loaded into an object of the same sizes replaces them
    t = mm.case("butane4")[0]
    other = bg.MolecularMechanicsEnergy.from_arrays({**t, "bond_k": 2 * t["bond_k"], "nonbonded_charge": 0 * t["nonbonded_charge"]})
    before = other._packed_tables()
    assert other._packed_tables() is before                                   # cached while nothing changes
    assert not torch.equal(other.energy(x), energy.energy(x))
    other.load_state_dict(state)
    assert torch.equal(other.energy(x), energy.energy(x)) and np.array_equal(other._packed_tables(), energy._packed_tables())
    assert other._packed_tables() is not before
    with torch.no_grad():
        other.bond_k.mul_(2.0)                                                # a parameter change in place
    assert not np.array_equal(other._packed_tables(), energy._packed_tables())
    # .to(dtype): the float tables are rounded, the index tables stay int64, the energy of an f64 input stays f64
    low = bg.MolecularMechanicsEnergy.from_arrays(t).to(torch.float32)
    assert low.bond_r0.dtype == torch.float32 and low.bond_idx.dtype == torch.int64 and low.torsion_periodicity.dtype == torch.int64
    u = low.energy(x)
    assert u.dtype == torch.float64 and torch.allclose(u, energy.energy(x), rtol=1e-5)
    assert isinstance(_kernel_plan(low, 1.0), MoleculePlan)


@pytest.mark.parametrize("name", ["ions3", "butane4", "ala2", "chain64"])
def test_pair_table_packing(cases, name):
    energy, _, _ = cases[name]
    t = mm.case(name)[0]
    n = energy.n_atoms
    brute = mm.pair_table(t)                                                  # a loop over i < j, ascending
    table = energy.pair_table()
    assert table.shape == (n * (n - 1) // 2, 3) and np.array_equal(table, brute)
    packed = energy._packed_tables()
    n_terms = energy.n_bonds + energy.n_angles + energy.n_torsions
    assert packed.dtype == np.int32 and len(packed) == 4 * n_terms + 3 * len(table) + 4
    pairs = packed[4 * n_terms:4 * n_terms + 3 * len(table)].view(np.float32).reshape(-1, 3)
    assert np.array_equal(pairs, brute.astype(np.float32))                    # products formed in double, rounded once
    row = {(i, j): r for r, (i, j) in enumerate((i, j) for i in range(n) for j in range(i + 1, n))}
    for m, (i, j) in enumerate(t["exception_idx"].tolist()):
        want = (mm.COULOMB * t["exception_chargeprod"][m], t["exception_sigma"][m], 4 * t["exception_epsilon"][m])
        assert tuple(table[row[(min(i, j), max(i, j))]]) == want              # an exception overrides the combination rule
        if t["exception_chargeprod"][m] == 0 and t["exception_epsilon"][m] == 0:
            assert pairs[row[(min(i, j), max(i, j))], 0] == 0 and pairs[row[(min(i, j), max(i, j))], 2] == 0     # an exclusion is zero
    # the term records: atoms in 6-bit fields, the periodicity above them
    words = packed[:4 * n_terms].reshape(-1, 4)
    if energy.n_torsions:
        tors = words[energy.n_bonds + energy.n_angles:]
        idx = np.stack([(tors[:, 0] >> s) & 63 for s in (0, 6, 12, 18)], axis=1)
        assert np.array_equal(idx, t["torsion_idx"]) and np.array_equal((tors[:, 0] >> 24) & 7, t["torsion_periodicity"])
        k, phase = t["torsion_k"], t["torsion_phase"]
        assert np.array_equal(tors[:, 1:].view(np.float32), np.stack([k, k * np.cos(phase), k * np.sin(phase)], axis=1).astype(np.float32))
    if energy.n_bonds:
        bonds = words[:energy.n_bonds]
        assert np.array_equal(np.stack([bonds[:, 0] & 63, (bonds[:, 0] >> 6) & 63], axis=1), t["bond_idx"])
        assert np.array_equal(bonds[:, 1:3].view(np.float32), np.stack([t["bond_r0"], t["bond_k"]], axis=1).astype(np.float32))


def test_synthetic_forcefield_is_the_recipe():
    z, xyz = mm.ala2_topology()
    assert np.array_equal(z, configs.ala2_global_z_matrix())
    made = configs.synthetic_forcefield(z, xyz, seed=0).to_arrays()
    want = mm.forcefield_arrays(z, xyz, seed=0)
    assert set(made) == set(want) and all(np.array_equal(made[k], want[k]) for k in want)
    assert (made["bond_idx"].shape, made["angle_idx"].shape, made["torsion_idx"].shape) == ((21, 2), (20, 3), (19, 4))
    gen = configs.make_ala2_mm_generator()
    assert isinstance(gen._target, bg.MolecularMechanicsEnergy) and gen._target.unit_energy == 2.494 and gen._target.dim == 66
    assert isinstance(_kernel_plan(gen._target, 1.0), MoleculePlan)


def test_plan_rules(cases):
    energy, x, _ = cases["butane4"]
    plan = _kernel_plan(energy, 2.0)
    assert isinstance(plan, MoleculePlan) and len(plan) not in (5, 6, 9) and plan.dist is energy
    assert (plan.n_atoms, plan.unit_energy, plan.temperature) == (4, 1.0, 2.0)
    assert _kernel_plan(energy, torch.tensor(1.0)) is None and _kernel_plan(energy, 0.0) is None

    class Shifted(bg.MolecularMechanicsEnergy):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    shifted = Shifted.from_arrays(mm.case("butane4")[0])
    assert _kernel_plan(shifted, 1.0) is None and torch.equal(shifted.energy(x), energy.energy(x) + 1.0)
    off = bg.MolecularMechanicsEnergy.from_arrays(mm.case("butane4")[0])
    off.fused = False
    assert _kernel_plan(off, 1.0) is None
    # no caller that folds field plans mistakes it for one: the wrappers, a product, the training tail
    from bgflow_amd.distributions import _wrapper_plan
    assert _wrapper_plan(bg.LinLogCutEnergy(energy, 1e3, 1e9), 1.0) is None
    assert _kernel_plan(bg.GradientClippedEnergy(energy, bg.ClipGradient(1e3, 3)), 1.0) is None
    prod = bg.ProductDistribution([bg.NormalDistribution(4), energy])
    assert prod._kernel_fields(1.0) is None and _kernel_plan(prod, 1.0) is None
    x0 = torch.randn(6, 4, dtype=torch.float64)
    assert torch.allclose(prod.energy(x0, x[:6]), bg.NormalDistribution(4).energy(x0) + energy.energy(x[:6]))
    # a CPU tensor is not the kernel's: the dispatchers decline, the energy runs the torch formulas
    assert kernel_energy(energy, (x.float(),)) is None and kl_loss_sums(energy, (x.float(),), torch.zeros(mm.B, 1)) is None
    cut = bg.LinLogCutEnergy(energy, 1e3, 1e9).energy(x)
    assert cut.shape == (mm.B, 1) and torch.isfinite(cut).all()


def test_outside_the_envelope_is_the_general_path():
    n = 65
    xyz = mm.chain_xyz(n)
    big = bg.MolecularMechanicsEnergy.from_arrays(mm.forcefield_arrays(mm.chain_z_matrix(n), xyz, seed=1))
    assert _kernel_plan(big, 1.0) is None
    assert torch.isfinite(big.energy(torch.from_numpy(xyz.reshape(1, -1)))).all()
    idx = np.array([[i, j] for i in range(64) for j in range(i + 1, 64)][:257])
    many = bg.MolecularMechanicsEnergy(64, bonds=(idx, np.full(257, 0.2), np.ones(257)))
    assert _kernel_plan(many, 1.0) is None and torch.isfinite(many.energy(torch.randn(3, 192))).all()
    assert isinstance(_kernel_plan(bg.MolecularMechanicsEnergy(64, bonds=(idx[:256], np.full(256, 0.2), np.ones(256))), 1.0), MoleculePlan)
    assert _kernel_plan(bg.MolecularMechanicsEnergy(1), 1.0) is None
    energy = bg.MolecularMechanicsEnergy.from_arrays(mm.case("butane4")[0])
    plan = _kernel_plan(energy, 1.0)
    x = torch.from_numpy(mm.inputs("butane4")["x"])
    for bad in (x, x.double(), x[:, :11]):                                  # (the device, dtype and layout checks run on every input)
        assert molecule._kernel_operands(plan, (bad,)) is None


def test_abi_entries_and_argument_checks(hip_lib):
    sigs = abi_signatures()
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    head = [p, i64, i32, i32, i32, i32, i32, p, f64, f64]
    want = {
        "bgk_molecule_energy": head + [p, p],
        "bgk_molecule_energy_kl_sums": head + [p, p, i32, p, i32, p, p],
        "bgk_molecule_energy_backward": head + [p, p, p, p, i32, p, p, p],
    }
    for name, args in want.items():
        assert name in abi_symbols() and sigs[name] == (ctypes.c_int, args), name
        assert list(getattr(hip_lib, name).argtypes) == args
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), name), ctypes.c_void_p).value, f"{name} is not exported"
    assert (molecule.MOLECULE_MAX_ATOMS, molecule.MOLECULE_MAX_BONDS, molecule.MOLECULE_MAX_ANGLES, molecule.MOLECULE_MAX_TORSIONS) == (64, 256, 512, 1024)
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def energy(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, u=fake):
        return hip_lib.bgk_molecule_energy(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, u, None)

    def sums(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, u=fake, dlogp=fake, partial=fake, out=fake):
        return hip_lib.bgk_molecule_energy_kl_sums(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, u, dlogp, 0, partial, 4, out, None)

    def backward(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, g_u=fake, g_x=fake):
        return hip_lib.bgk_molecule_energy_backward(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, g_u, None, None, None, 0, None,
                                                    g_x, None)

    for call in (energy, sums, backward):
        if call is not sums:                                        # (an empty batch zeroes the loss sums: device work)
            assert call(batch=0) == 0
        for over in (dict(n=1, npairs=0), dict(n=65, npairs=0), dict(nb=257), dict(na=513), dict(nt=1025)):
            assert call(**over) == -2 and b"envelope" in hip_lib.bgk_last_error(), over
        assert call(batch=-1) == -1 and call(temperature=0.0) == -1 and call(unit=0.0) == -1
        assert call(npairs=5) == -1 and call(nb=-1) == -1
        assert call(x=None) == -1 and call(tables=None) == -1 and call(tables=ctypes.c_void_p(68)) == -1
    assert energy(u=None) == -1
    assert sums(out=None) == -1 and sums(dlogp=None) == -1 and sums(partial=None) == -1
    assert backward(g_u=None) == -1 and backward(g_x=None) == -1    # neither g_u nor the loss form


def test_samplers_accept_the_energy():
    torch.manual_seed(0)
    energy = bg.MolecularMechanicsEnergy.from_arrays(mm.case("butane4")[0])
    x = torch.from_numpy(mm.inputs("butane4")["x"][8:16]).double()
    proposal = bg.HamiltonianProposal(energy, 1e-4, n_leapfrog=3)
    new, dlp = proposal(bg.SamplerState(samples=x))
    x1 = new.as_dict()["samples"][0]
    assert x1.shape == x.shape and torch.isfinite(x1).all() and torch.isfinite(dlp).all() and not torch.equal(x1, x)
    for prop in (bg.GaussianProposal(1e-3), bg.HamiltonianProposal(energy, 1e-4, n_leapfrog=2)):
        step = bg.MCMCStep(energy, proposal=prop, n_steps=3)
        assert step._fused_setup(bg.SamplerState(samples=x)) is None
        out = step(bg.SamplerState(samples=x)).as_dict()["samples"][0]
        assert out.shape == x.shape and torch.isfinite(out).all()
