"""Host: the implicit solvent (GBSA-OBC) of ``MolecularMechanicsEnergy`` -- the general path (torch ops) against the yardstick's f64 run
(tests/golden/solvent.npz, written by tests/golden/make_solvent_goldens.py), the constructor's checks, the array round trips, the packed
solvent table, the unchanged vacuum object and the new C entries' prototypes and argument checks.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bgflow_amd as bg
import molecule_common as mm
import solvent_common as sc
from bgflow_amd import _lib, configs, molecule
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols
from bgflow_amd.distributions import MoleculePlan, _kernel_plan

ALL = sc.CASES + [sc.EXTRA]


@pytest.fixture(scope="module")
def G(golden):
    return golden("solvent")


@pytest.fixture(scope="module")
def cases():
    """name -> (energy object, x f64 [150, 3 n], a f64 [150]), built once"""
    out = {}
    for name in ALL:
        inp = sc.inputs(name)
        out[name] = (bg.MolecularMechanicsEnergy.from_arrays(sc.case(name)[0]), torch.from_numpy(inp["x"]).double(),
                     torch.from_numpy(inp["a"]).double())
    return out


@pytest.mark.parametrize("name", ALL)
def test_inputs_are_the_fixtures(G, name):
    np.testing.assert_allclose(sc.checksum(sc.inputs(name)), G[f"{name}_checksum"], rtol=1e-12)


def test_every_regime_of_h_is_taken(G):
    counts = {name: sc.regime_counts(name) for name in sc.CASES}
    for name, c in counts.items():
        print(name, "regimes a b c d:", c.tolist())
        n = int(sc.case(name)[0]["n_atoms"])
        assert np.array_equal(c, G[f"{name}_regimes"]) and c.sum() == mm.B * n * (n - 1)
        assert c[0] > 0 and c[3] > 0, name                         # the contact row: (a) and (d)
        assert c[0] + c[2] + c[3] > 0, name                        # (b) is never the only regime
    assert (sum(counts.values()) > 0).all()


@pytest.mark.parametrize("name", ALL)
def test_general_path_f64_is_the_yardstick(cases, G, name):
    energy, x, a = cases[name]
    u, g = mm.evaluate(energy, x, a)
    for key, err in mm.errors(u, g, G, name).items():
        print(name, key, err)
        assert err <= 1e-12, (name, key, err)


@pytest.mark.parametrize("name", ALL)
def test_general_path_f32_within_the_bound(cases, G, name):
    energy, x, a = cases[name]
    u, g = mm.evaluate(energy, x.float(), a.float())
    assert u.dtype == np.float32 and g.dtype == np.float32
    mm.assert_within(mm.errors(u, g, G, name), G, name, what="torch f32 ")


@pytest.mark.parametrize("name", ["butane4_gb", "ala2_gb"])
def test_second_derivative_exists(cases, name):
    energy, x, _ = cases[name]
    x = x[:5].clone().requires_grad_(True)
    g, = torch.autograd.grad(energy.energy(x).sum(), x, create_graph=True)
    h, = torch.autograd.grad((g * g).sum(), x)
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def test_coincident_atoms_of_an_excluded_pair_give_plus_infinity(cases):
    _, x, _ = cases["butane4_gb"]
    t = sc.case("butane4_gb")[0]
    # without the bonded terms that are themselves singular where atoms 0 and 1 coincide
    t = {**t, "bond_idx": t["bond_idx"][1:], "bond_r0": t["bond_r0"][1:], "bond_k": t["bond_k"][1:], "angle_idx": t["angle_idx"][:0],
         "angle_theta0": t["angle_theta0"][:0], "angle_k": t["angle_k"][:0], "torsion_idx": t["torsion_idx"][:0],
         "torsion_periodicity": t["torsion_periodicity"][:0], "torsion_phase": t["torsion_phase"][:0], "torsion_k": t["torsion_k"][:0]}
    energy = bg.MolecularMechanicsEnergy.from_arrays(t)
    vacuum = bg.MolecularMechanicsEnergy.from_arrays({k: v for k, v in t.items() if k in mm.case("butane4")[0]})
    table = energy.pair_table()
    assert table[0, 0] == 0 and table[0, 2] == 0                   # atoms 0 and 1: a 1-2 pair, excluded
    x = x[:4].clone()
    x[1, 3:6] = x[1, 0:3]
    assert torch.isfinite(vacuum.energy(x)).all()                  # the vacuum terms do not mind
    xg = x.clone().requires_grad_(True)
    u = energy.energy(xg)
    assert float(u.detach()[1]) == float("inf") and torch.isfinite(u[[0, 2, 3]]).all()
    g, = torch.autograd.grad(u.sum(), xg)
    xv = x.clone().requires_grad_(True)
    gv, = torch.autograd.grad(vacuum.energy(xv).sum(), xv)
    assert torch.isfinite(g).all() and torch.equal(g[1], gv[1])    # the solvent terms add nothing to that row's gradient
    assert not torch.equal(g[0], gv[0])
    # in f32 as well
    u32 = energy.energy(x.float())
    assert float(u32[1]) == float("inf") and torch.isfinite(u32[[0, 2, 3]]).all()


def _solvent(**over):
    kw = dict(n_atoms=3, implicit_solvent=(np.array([0.1, -0.2, 0.1]), np.array([0.15, 0.12, 0.2]), np.array([0.8, 0.85, 0.7])))
    kw.update(over)
    return kw


def test_constructor_validation_names_the_atom():
    e = bg.MolecularMechanicsEnergy(**_solvent())
    assert e.has_solvent and not e.has_nonbonded and (e.solute_dielectric, e.solvent_dielectric, e.surface_area_energy) == (1.0, 78.5, 2.25936)
    q, r, s = _solvent()["implicit_solvent"]
    bad = [
        (dict(implicit_solvent=(q[:2], r, s)), "charge has 2 entries for 3 atoms"),
        (dict(implicit_solvent=(q, r, np.append(s, 0.8))), "scale has 4 entries for 3 atoms"),
        (dict(implicit_solvent=(q, r)), "must be \\(charge, radius, scale\\)"),
        (dict(implicit_solvent=(np.array([0.1, np.nan, 0.1]), r, s)), "atom 1 has a non-finite charge"),
        (dict(implicit_solvent=(q, np.array([0.15, 0.12, np.inf]), s)), "atom 2 has a non-finite radius"),
        (dict(implicit_solvent=(q, np.array([0.009, 0.12, 0.2]), s)), "atom 0 has radius <= 0.009"),
        (dict(implicit_solvent=(q, np.array([0.15, -1.0, 0.2]), s)), "atom 1 has radius <= 0.009"),
        (dict(implicit_solvent=(q, r, np.array([0.8, 0.85, 0.0]))), "atom 2 has scale <= 0"),
        (dict(solute_dielectric=0.0), "solute_dielectric"),
        (dict(solvent_dielectric=-78.5), "solvent_dielectric"),
        (dict(surface_area_energy=-1.0), "surface_area_energy"),
    ]
    for over, text in bad:
        with pytest.raises(ValueError, match=text):
            bg.MolecularMechanicsEnergy(**_solvent(**over))
    bg.MolecularMechanicsEnergy(**_solvent(surface_area_energy=0))      # 0 switches the surface term off


def test_array_round_trips_are_bitwise(cases, tmp_path):
    for name in ("ala2_gb", sc.EXTRA):
        energy, x, _ = cases[name]
        arrays = energy.to_arrays()
        assert all(isinstance(v, np.ndarray) and v.dtype.kind in "if" for v in arrays.values())
        want = sc.case(name)[0]
        assert set(arrays) == set(want)
        for k, v in want.items():
            assert arrays[k].dtype == v.dtype and np.array_equal(arrays[k], v), k
        path = tmp_path / f"{name}.npz"
        energy.save(path)
        for other in (bg.MolecularMechanicsEnergy.from_arrays(arrays), bg.MolecularMechanicsEnergy.load(path)):
            back = other.to_arrays()
            assert set(back) == set(arrays) and all(np.array_equal(back[k], arrays[k]) and back[k].dtype == arrays[k].dtype for k in arrays)
            assert torch.equal(other.energy(x), energy.energy(x))
    # a state dict carries the three arrays into an object of the same sizes
    energy, x, _ = cases["butane4_gb"]
    t = sc.case("butane4_gb")[0]
    other = bg.MolecularMechanicsEnergy.from_arrays({**t, "solvent_radius": t["solvent_radius"] + 0.01})
    assert not torch.equal(other.energy(x), energy.energy(x))
    state = energy.state_dict()
    assert {"solvent_charge", "solvent_radius", "solvent_scale"} <= set(state)
    other.load_state_dict(state)
    assert torch.equal(other.energy(x), energy.energy(x)) and np.array_equal(other._packed_solvent(), energy._packed_solvent())


def test_without_the_keyword_nothing_changes():
    t = mm.case("butane4")[0]
    vacuum = bg.MolecularMechanicsEnergy.from_arrays(t)
    solvent = bg.MolecularMechanicsEnergy.from_arrays(sc.case("butane4_gb")[0])
    assert not vacuum.has_solvent and set(vacuum.to_arrays()) == set(t)
    names = {f"{g}_{n}" for g, ns in (("bond", ("idx", "r0", "k")), ("angle", ("idx", "theta0", "k")), ("torsion", ("idx", "periodicity", "phase", "k")),
                                      ("exception", ("idx", "chargeprod", "sigma", "epsilon")), ("nonbonded", ("charge", "sigma", "epsilon"))) for n in ns}
    assert set(vacuum.state_dict()) == names
    assert set(solvent.state_dict()) == names | {"solvent_charge", "solvent_radius", "solvent_scale"}
    assert set(solvent.to_arrays()) == set(t) | {"has_solvent", "solvent_charge", "solvent_radius", "solvent_scale", "solute_dielectric",
                                                  "solvent_dielectric", "surface_area_energy"}
    # the packed vacuum table is the same with and without a solvent: the solvent has a table of its own
    assert np.array_equal(vacuum._packed_tables(), solvent._packed_tables())
    assert len(vacuum._packed_tables()) == 4 * (3 + 2 + 2) + 3 * 6 + 4
    for e in (vacuum, solvent):
        plan = _kernel_plan(e, 1.0)
        assert isinstance(plan, MoleculePlan) and len(plan) == 4 and plan.dist is e


def test_packed_solvent_table(cases):
    for name in ALL:
        energy, _, _ = cases[name]
        t = sc.case(name)[0]
        n = energy.n_atoms
        packed = energy._packed_solvent()
        assert packed.dtype == np.float32 and len(packed) == 4 * n + 4 * ((n + 3) // 4)
        gamma = float(t["surface_area_energy"])
        for i in range(n):                                          # products formed in double, rounded once
            q, r, s = (float(t[f"solvent_{k}"][i]) for k in ("charge", "radius", "scale"))
            rho = r - 0.009
            assert np.array_equal(packed[4 * i:4 * i + 4], np.array([q, rho, s * rho, r]).astype(np.float32)), (name, i)
            assert packed[4 * n + i] == np.float32(4.0 * np.pi * gamma * (r + 0.14) ** 2 * r ** 6), (name, i)
        assert (packed[5 * n:] == 0).all()
        want = -mm.COULOMB * (1.0 / float(t["solute_dielectric"]) - 1.0 / float(t["solvent_dielectric"]))
        assert energy.gb_prefactor() == want and want < 0


def test_in_place_edits_invalidate_the_tables(cases):
    energy = bg.MolecularMechanicsEnergy.from_arrays(sc.case("butane4_gb")[0])
    _, x, _ = cases["butane4_gb"]
    before, packed, u = energy._packed_solvent(), energy._packed_tables(), energy.energy(x)
    assert energy._packed_solvent() is before                       # cached while nothing changes
    with torch.no_grad():
        energy.solvent_radius.add_(0.01)
    after = energy._packed_solvent()
    assert after is not before and not np.array_equal(after, before) and np.array_equal(energy._packed_tables(), packed)
    assert not torch.equal(energy.energy(x), u)


def test_synthetic_forcefield_is_the_recipe():
    z, xyz = mm.ala2_topology()
    plain = configs.synthetic_forcefield(z, xyz, seed=0).to_arrays()
    made = configs.synthetic_forcefield(z, xyz, seed=0, implicit_solvent=True).to_arrays()
    assert all(np.array_equal(made[k], plain[k]) for k in plain)    # the vacuum tables are those of the default call
    rng = np.random.RandomState(0)
    n = len(xyz)
    charge = rng.uniform(-0.5, 0.5, n)
    charge -= charge.mean()
    rng.uniform(0.15, 0.35, n), rng.uniform(0.05, 0.5, n)
    assert np.array_equal(made["solvent_charge"], charge) and np.array_equal(made["solvent_charge"], made["nonbonded_charge"])
    assert np.array_equal(made["solvent_radius"], rng.uniform(0.11, 0.20, n)) and np.array_equal(made["solvent_scale"], rng.uniform(0.70, 0.90, n))
    assert (float(made["solute_dielectric"]), float(made["solvent_dielectric"]), float(made["surface_area_energy"])) == (1.0, 78.5, 2.25936)
    gen = configs.make_ala2_mm_generator(implicit_solvent=True)
    assert gen._target.has_solvent and gen._target.unit_energy == 2.494 and not configs.make_ala2_mm_generator()._target.has_solvent


def test_more_than_64_atoms_run_the_general_path():
    n = 65
    xyz = mm.chain_xyz(n)
    big = configs.synthetic_forcefield(mm.chain_z_matrix(n), xyz, seed=1, implicit_solvent=True)
    assert _kernel_plan(big, 1.0) is None and torch.isfinite(big.energy(torch.from_numpy(xyz.reshape(1, -1)))).all()


def test_abi_entries_and_argument_checks(hip_lib):
    sigs = abi_signatures()
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    head = [p, i64, i32, i32, i32, i32, i32, p, f64, f64, p, f64]
    want = {
        "bgk_molecule_solvent_energy": head + [p, p],
        "bgk_molecule_solvent_energy_kl_sums": head + [p, p, i32, p, i32, p, p],
        "bgk_molecule_solvent_energy_backward": head + [p, p, p, p, i32, p, p, p],
    }
    for name, args in want.items():
        assert name in abi_symbols() and sigs[name] == (ctypes.c_int, args), name
        assert list(getattr(hip_lib, name).argtypes) == args
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), name), ctypes.c_void_p).value, f"{name} is not exported"
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def energy(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, solvent=fake, pre=-137.0, u=fake):
        return hip_lib.bgk_molecule_solvent_energy(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, solvent, pre, u, None)

    def sums(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, solvent=fake, pre=-137.0, u=fake,
             dlogp=fake, partial=fake, out=fake):
        return hip_lib.bgk_molecule_solvent_energy_kl_sums(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, solvent, pre, u, dlogp,
                                                           0, partial, 4, out, None)

    def backward(x=fake, batch=8, n=4, nb=3, na=2, nt=2, npairs=6, tables=fake, unit=1.0, temperature=1.0, solvent=fake, pre=-137.0,
                 g_u=fake, g_x=fake):
        return hip_lib.bgk_molecule_solvent_energy_backward(x, batch, n, nb, na, nt, npairs, tables, unit, temperature, solvent, pre, g_u,
                                                            None, None, None, 0, None, g_x, None)

    for call in (energy, sums, backward):
        if call is not sums:                                        # (an empty batch zeroes the loss sums: device work)
            assert call(batch=0) == 0
        for over in (dict(n=1, npairs=0), dict(n=65, npairs=0), dict(nb=257), dict(na=513), dict(nt=1025)):
            assert call(**over) == -2 and b"envelope" in hip_lib.bgk_last_error(), over
        assert call(batch=-1) == -1 and call(temperature=0.0) == -1 and call(unit=0.0) == -1
        assert call(npairs=5) == -1 and call(nb=-1) == -1
        assert call(x=None) == -1 and call(tables=None) == -1 and call(tables=ctypes.c_void_p(68)) == -1
        assert call(solvent=None) == -1 and b"solvent" in hip_lib.bgk_last_error()
        assert call(solvent=ctypes.c_void_p(68)) == -1 and b"solvent" in hip_lib.bgk_last_error()
        assert call(pre=float("nan")) == -1
    assert energy(u=None) == -1
    assert sums(out=None) == -1 and sums(dlogp=None) == -1 and sums(partial=None) == -1
    assert backward(g_u=None) == -1 and backward(g_x=None) == -1    # neither g_u nor the loss form
