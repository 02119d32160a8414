"""Cases, inputs and regime counts of the implicit-solvent tests of ``MolecularMechanicsEnergy`` (GBSA-OBC).  Everything is regenerated
from seeds with numpy alone on top of tests/molecule_common.py (tests/golden/solvent.npz stores the inputs' checksums, the regime counts
and the yardstick's OUTPUTS, written by tests/golden/make_solvent_goldens.py, which states the formulas itself).

Cases: ``<base>_gb`` is the case ``<base>`` of molecule_common (same tables, same rows, same ``a``) plus a solvent with seeded charges
(uniform in [-0.5, 0.5]), radii (uniform in [0.11, 0.20] nm) and scales (uniform in [0.70, 0.90]) and the default dielectrics and surface
energy:

  pair2_gb    2 atoms, one bond, no nonbonded tables: the contact row tests the solvent terms alone
  ions3_gb    3 atoms, nonbonded only
  butane4_gb  4 atoms
  ala2_gb     22 atoms, row stride 67
  chain64_gb  64 atoms: the forward tile has 32 rows, the backward tile 16

``ala2_gb_nosa`` is ``ala2_gb`` on the same rows with ``surface_area_energy = 0`` and ``solute_dielectric = 2``.

Rows: those of ``molecule_common.inputs``; row 3 is the 0.01 nm contact of the first pair that interacts (pair2 has none: there the row
is made HERE by the same recipe for atoms 0 and 1, since under Generalised Born every pair interacts).  The contact pair (i, j) gets the
radii (0.11, 0.20) nm and atom j the scale 0.85, so that at 0.01 nm atom i lies inside j's scaled sphere (regime (d) of H for the ordered
pair (i, j)) and i's scaled sphere lies inside j's (regime (a) for (j, i)).

Regimes of H(r, rho_i, sigma_j) for an ordered pair: (a) rho_i >= r + sigma_j; (d) rho_i < sigma_j - r; (b) r - sigma_j >= rho_i
(separate spheres); (c) everything else (overlapping spheres).  ``regime_counts`` counts them over all rows.
"""
import numpy as np

import molecule_common as mm

CASES = [f"{base}_gb" for base in mm.CASES]
EXTRA = "ala2_gb_nosa"
GB_OFFSET, GB_PROBE = 0.009, 0.14
SOLUTE, SOLVENT, SURFACE = 1.0, 78.5, 2.25936


def base_of(name):
    return name.split("_gb")[0]


def contact_pair(t):
    """the atoms of row 3's contact: the first pair that interacts, or (0, 1) without one"""
    li, lj = mm.live_pairs(t)[:2]
    return (int(li[0]), int(lj[0])) if len(li) else (0, 1)


def case(name):
    """(tables dict for ``MolecularMechanicsEnergy.from_arrays``, reference geometry f64 [n, 3])"""
    base = base_of(name)
    t, xyz = mm.case(base)
    n = int(t["n_atoms"])
    rng = np.random.RandomState(mm.SEED + 100 + mm.CASES.index(base))
    charge, radius, scale = rng.uniform(-0.5, 0.5, n), rng.uniform(0.11, 0.20, n), rng.uniform(0.70, 0.90, n)
    i, j = contact_pair(t)
    radius[i], radius[j], scale[j] = 0.11, 0.20, 0.85
    t = dict(t)
    t.update(has_solvent=np.array(1, np.int64), solvent_charge=charge, solvent_radius=radius, solvent_scale=scale,
             solute_dielectric=np.array(2.0 if name == EXTRA else SOLUTE), solvent_dielectric=np.array(SOLVENT),
             surface_area_energy=np.array(0.0 if name == EXTRA else SURFACE))
    return t, xyz


def inputs(name):
    """dict: x f32 [150, 3 n], a f32 [150]"""
    base = base_of(name)
    inp = mm.inputs(base)
    t = mm.case(base)[0]
    if not len(mm.live_pairs(t)[0]):                              # row 3: the contact, made here for a case without nonbonded tables
        i, j = contact_pair(t)
        p = inp["x"][3].astype(np.float64).reshape(-1, 3)
        d = p[j] - p[i]
        p[j] = p[i] + 0.01 * d / np.linalg.norm(d)
        inp["x"][3] = p.reshape(-1).astype(np.float32)
    return inp


checksum = mm.checksum


def regime_counts(name):
    """int64 [4]: how many ordered pairs (i, j != i) over all rows fall into the regimes (a), (b), (c), (d) of H"""
    t, _ = case(name)
    n = int(t["n_atoms"])
    p = inputs(name)["x"].astype(np.float64).reshape(mm.B, n, 3)
    r = np.linalg.norm(p[:, :, None] - p[:, None, :], axis=-1)
    rho = (t["solvent_radius"] - GB_OFFSET)
    sigma = (t["solvent_scale"] * rho)[None, None, :]
    rho = rho[None, :, None]
    off = ~np.eye(n, dtype=bool)[None]
    a = rho >= r + sigma
    d = rho < sigma - r
    b = ~a & ~d & (r - sigma >= rho)
    c = ~a & ~b & ~d
    assert ((a & d).sum(), (a | b | c | d)[np.broadcast_to(off, a.shape)].all()) == (0, True)
    return np.array([(m & off).sum() for m in (a, b, c, d)], np.int64)
