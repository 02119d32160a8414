"""``MolecularMechanicsEnergy``: a classical force-field energy over the Cartesian coordinates of one molecule -- harmonic bonds and
angles, periodic torsions, Lennard-Jones and Coulomb pairs with exclusions and exceptions.  The functional forms and units (nm,
kJ/mol, rad) are those of OpenMM's ``HarmonicBondForce``, ``HarmonicAngleForce``, ``PeriodicTorsionForce`` and ``NonbondedForce`` with
``NoCutoff``, so the tables can be read off an OpenMM ``System`` (INTEGRATION.md has the recipe); OpenMM itself is never imported.

The general path is the formulas in torch ops -- any device, dtype and layout, twice differentiable.  A contiguous f32 HIP tensor
[B, 3 n] of 2..64 atoms (at most ``MOLECULE_MAX_BONDS`` bonds, ``MOLECULE_MAX_ANGLES`` angles, ``MOLECULE_MAX_TORSIONS`` torsion terms) at
a scalar temperature runs on csrc/bgk_molecule.hip instead: one launch for the energy (optionally with the KL integrand's sums, so
``KLTrainer`` keeps its fused loss path), one for the gradient.  The kernel's arithmetic is defined in csrc/bgk_molecule_terms.h.

``implicit_solvent=(charge, radius, scale)`` adds a GBSA-OBC solvent (Generalised Born, OBC2, plus the surface-area term: the arithmetic
of OpenMM's ``GBSAOBCForce``, csrc/bgk_solvent_terms.h) to both paths; on the kernel path the vacuum and solvent terms are one launch.
"""
import numpy as np
import torch

from .distributions import Energy, MoleculePlan, _kernel_plan, kernel_energy

__all__ = ["MolecularMechanicsEnergy"]

COULOMB = 138.935458                                  # 1 / (4 pi eps0) in kJ nm / (mol e^2) (OpenMM's ONE_4PI_EPS0)
MOLECULE_MAX_ATOMS = 64                               # the envelope of csrc/bgk_molecule.hip (BGK_MOLECULE_MAX_* of include/bgflow_amd.h)
MOLECULE_MAX_BONDS, MOLECULE_MAX_ANGLES, MOLECULE_MAX_TORSIONS = 256, 512, 1024
_MAX_BLOCKS = 2048                                    # block partials of the loss sums
GB_OFFSET, GB_PROBE = 0.009, 0.14                     # GBSAOBCForce (OBC2): dielectric offset and probe radius in nm
GB_ALPHA, GB_BETA, GB_GAMMA = 1.0, 0.8, 4.85          # 1 / B = 1 / rho - tanh(alpha Psi - beta Psi^2 + gamma Psi^3) / r

# the term groups: name -> (atoms per term, the float tables, the integer tables)
_GROUPS = {"bond": (2, ("r0", "k"), ()), "angle": (3, ("theta0", "k"), ()), "torsion": (4, ("phase", "k"), ("periodicity",)),
           "exception": (2, ("chargeprod", "sigma", "epsilon"), ())}
_ARGS = {"bond": "bonds", "angle": "angles", "torsion": "torsions", "exception": "exceptions"}


def _is_number(t):
    return isinstance(t, (int, float)) and not isinstance(t, bool)


def _f64(a, what):
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64).reshape(-1)
    if not np.isfinite(a).all():
        raise ValueError(f"MolecularMechanicsEnergy: {what} has a non-finite entry (term {int(np.flatnonzero(~np.isfinite(a))[0])})")
    return a


def _index(a, width, n_atoms, what):
    """int64 [N, width] with every atom in 0..n_atoms-1 and distinct atoms within a term"""
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    if a.size == 0:
        return np.zeros((0, width), np.int64)
    if a.ndim != 2 or a.shape[1] != width or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"MolecularMechanicsEnergy: {what} indices must be an integer array [N, {width}], got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    for t, row in enumerate(a):
        if (row < 0).any() or (row >= n_atoms).any():
            raise ValueError(f"MolecularMechanicsEnergy: {what} term {t} {tuple(row)} names an atom outside 0..{n_atoms - 1}")
        if len(set(row.tolist())) != width:
            raise ValueError(f"MolecularMechanicsEnergy: {what} term {t} {tuple(row)} names an atom twice")
    return a


def _pair_index(n):
    """(i, j) of the pairs i < j in ascending (i, j) order"""
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int64), j.astype(np.int64)


# ---- launches ----------------------------------------------------------------------------------------------------------------------
def _counts(plan):
    d = plan.dist
    return (plan.n_atoms, d.n_bonds, d.n_angles, d.n_torsions, d.n_pairs)


def _scale(plan):
    return (float(plan.unit_energy), float(plan.temperature))


def _solvent(plan, device):
    """the extra arguments of the bgk_molecule_solvent_* entries: (the solvent table's pointer, the prefactor), or () for a vacuum energy"""
    from . import _lib
    d = plan.dist
    return (_lib.ptr(d._device_solvent(device)), d.gb_prefactor()) if d.has_solvent else ()


def _launch_energy(plan, tables, x2, dlogp=None, drop_nonfinite=False, want_sums=False):
    """one launch of bgk_molecule_energy / bgk_molecule_energy_kl_sums (with solvent tables: bgk_molecule_solvent_energy / _kl_sums) on the
    contiguous rows x2: u [B] (and the f64 loss sums [2])"""
    from . import _lib
    B, dev = x2.shape[0], x2.device
    u = torch.empty(B, dtype=torch.float32, device=dev)
    sums = None
    head = "bgk_molecule_solvent_energy" if plan.dist.has_solvent else "bgk_molecule_energy"
    with torch.cuda.device(dev):
        common = (_lib.ptr(x2), B, *_counts(plan), _lib.ptr(tables), *_scale(plan), *_solvent(plan, dev), _lib.ptr(u))
        if want_sums:
            partial = torch.empty((_MAX_BLOCKS, 2), dtype=torch.float64, device=dev)
            sums = torch.empty(2, dtype=torch.float64, device=dev)
            name = head + "_kl_sums"
            st = getattr(_lib.lib(), name)(*common, _lib.ptr(dlogp), int(bool(drop_nonfinite)), _lib.ptr(partial), _MAX_BLOCKS,
                                           _lib.ptr(sums), _lib.stream_ptr(dev))
        else:
            name = head
            st = getattr(_lib.lib(), name)(*common, _lib.stream_ptr(dev))
    _lib.check(st, name)
    return u, sums


def _launch_backward(plan, tables, x2, g_u=None, g_scalar=None, u=None, dlogp=None, drop_nonfinite=False, want_gdl=False):
    """one launch of bgk_molecule_energy_backward (with solvent tables: bgk_molecule_solvent_energy_backward): (g_x [B, 3 n], g_dlogp [B]
    or None)"""
    from . import _lib
    B, dev = x2.shape[0], x2.device
    gx = torch.empty_like(x2)
    g_dl = torch.empty(B, dtype=torch.float32, device=dev) if want_gdl else None
    name = "bgk_molecule_solvent_energy_backward" if plan.dist.has_solvent else "bgk_molecule_energy_backward"
    with torch.cuda.device(dev):
        st = getattr(_lib.lib(), name)(_lib.ptr(x2), B, *_counts(plan), _lib.ptr(tables), *_scale(plan), *_solvent(plan, dev), _lib.ptr(g_u),
                                       _lib.ptr(g_scalar), _lib.ptr(u), _lib.ptr(dlogp), int(bool(drop_nonfinite)),
                                       _lib.ptr(g_dl), _lib.ptr(gx), _lib.stream_ptr(dev))
    _lib.check(st, name)
    return gx, g_dl


class _MoleculeEnergyFn(torch.autograd.Function):
    """u = E(x) / unit_energy / T on bgk_molecule_energy; the gradient is one launch of bgk_molecule_energy_backward.  A backward under
    ``create_graph=True`` forms the gradient from the torch formulas instead, whose graph can be differentiated again."""

    @staticmethod
    def forward(ctx, plan, tables, x2):
        u, _ = _launch_energy(plan, tables, x2)
        ctx.save_for_backward(x2)
        ctx.cfg = (plan, tables)
        return u[:, None]

    @staticmethod
    def backward(ctx, g_u):
        (x2,) = ctx.saved_tensors
        plan = ctx.cfg[0]
        if torch.is_grad_enabled():
            xg = x2 if x2.requires_grad else x2.detach().requires_grad_(True)
            u = plan.dist._energy(xg) / plan.temperature
            return None, None, torch.autograd.grad(u, xg, g_u, create_graph=True)[0]
        gx, _ = _launch_backward(*ctx.cfg, x2, g_u=g_u.reshape(-1).to(torch.float32).contiguous())
        return None, None, gx


class _MoleculeKLSumsFn(torch.autograd.Function):
    """[sum_b (u(x_b) - dlogp_b), number of samples kept] (f64 [2]) with the partial sums formed by the molecule kernel itself;
    backward: one launch for the gradients of x and dlogp"""

    @staticmethod
    def forward(ctx, plan, tables, drop_nonfinite, dlogp, x2):
        dl = dlogp.detach().reshape(-1).to(torch.float32).contiguous()
        u, sums = _launch_energy(plan, tables, x2, dlogp=dl, drop_nonfinite=drop_nonfinite, want_sums=True)
        ctx.save_for_backward(u, dl, x2)
        ctx.cfg = (plan, tables, bool(drop_nonfinite), dlogp.shape)
        u2 = u[:, None]
        ctx.mark_non_differentiable(u2)
        return sums, u2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sums, _g_u):
        plan, tables, drop, dl_shape = ctx.cfg
        u, dl, x2 = ctx.saved_tensors
        gs = g_sums[0:1].to(torch.float32).contiguous()
        gx, g_dl = _launch_backward(plan, tables, x2, g_scalar=gs, u=u, dlogp=dl, drop_nonfinite=drop, want_gdl=ctx.needs_input_grad[3])
        return None, None, None, None if g_dl is None else g_dl.reshape(dl_shape), gx


def _kernel_operands(plan, xs):
    """(x [B, 3 n], the packed device tables) if the molecule kernel takes this input, else None"""
    if len(xs) != 1 or not torch.is_tensor(xs[0]):
        return None
    x = xs[0]
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3 * plan.n_atoms and x.shape[0] > 0
            and x.is_contiguous()):
        return None
    return x, plan.dist._device_tables(x.device)


def molecule_energy(plan, xs):
    """the [B, 1] energy of a MoleculePlan on bgk_molecule_energy, or None if the input is not the kernel's"""
    ops = _kernel_operands(plan, xs)
    return None if ops is None else _MoleculeEnergyFn.apply(plan, ops[1], ops[0])


def molecule_kl_loss_sums(plan, xs, dlogp, drop_nonfinite=False):
    """(sums, u) of distributions.kl_loss_sums for a MoleculePlan, or None"""
    ops = _kernel_operands(plan, xs)
    if ops is None or not (torch.is_tensor(dlogp) and dlogp.is_cuda and dlogp.numel() == xs[0].shape[0]):
        return None
    return _MoleculeKLSumsFn.apply(plan, ops[1], bool(drop_nonfinite), dlogp, ops[0])


class MolecularMechanicsEnergy(Energy):
    """Force-field energy of one molecule of ``n_atoms`` atoms over its Cartesian coordinates, a row [x0, y0, z0, x1, ...] of
    ``dim = 3 n_atoms`` numbers in nm; energies in kJ/mol, angles in rad.  Every term group is optional:

        bonds       (idx int[Nb, 2], r0[Nb], k[Nb])                 k / 2 (r - r0)^2                    HarmonicBondForce
        angles      (idx int[Na, 3], theta0[Na], k[Na])             k / 2 (theta - theta0)^2, vertex idx[:, 1]    HarmonicAngleForce
        torsions    (idx int[Nt, 4], periodicity int[Nt] in 1..6, phase[Nt], k[Nt])
                                                                    k (1 + cos(n phi - phase))          PeriodicTorsionForce
        nonbonded   (charge[n], sigma[n], epsilon[n])               every pair i < j with sigma_ij = (s_i + s_j) / 2,
                                                                    eps_ij = sqrt(e_i e_j), qq_ij = q_i q_j (Lorentz-Berthelot):
                    4 eps_ij ((sigma_ij / r)^12 - (sigma_ij / r)^6) + 138.935458 qq_ij / r            NonbondedForce, NoCutoff
        exceptions  (idx int[Ne, 2], chargeprod[Ne], sigma[Ne], epsilon[Ne])   replaces that pair's (qq, sigma, eps); (0, ., 0) excludes it
        implicit_solvent  (charge[n], radius[n], scale[n])          Generalised Born (OBC2) + surface area over ALL pairs        GBSAOBCForce
                    with ``solute_dielectric``, ``solvent_dielectric`` and ``surface_area_energy`` (kJ/mol/nm^2; 0: no surface term); the
                    charges are the solvent force's own, so no nonbonded tables are needed (formulas: csrc/bgk_solvent_terms.h)

    phi is the IUPAC dihedral of atoms (i, j, k, l) (trans = pi), the sign OpenMM uses; several torsion terms may name the same four
    atoms (Fourier series, impropers).  ``energy(x, temperature)`` is the reduced energy ``E / unit_energy / temperature`` of shape
    [B, 1] (``unit_energy``: kT in kJ/mol), ``force(x)`` minus its gradient.  Two coincident atoms of a pair that is not excluded give
    the energy +inf (never NaN) and contribute no gradient; with an implicit solvent ANY two coincident atoms do, and the solvent terms
    then add nothing to that row's gradient.

    The constructor raises ``ValueError``, naming the term, for an atom outside ``0..n_atoms-1``, an atom twice within a term, a
    non-positive ``r0`` or ``sigma``, a periodicity outside 1..6 and two exceptions for one pair; naming the atom, for a solvent array of the
    wrong length, a non-finite entry, a ``radius <= 0.009`` and a ``scale <= 0``; and for a dielectric ``<= 0`` or a negative surface energy.  ``to_arrays`` / ``from_arrays`` /
    ``save`` / ``load`` carry the tables through a dict / an ``.npz`` of numbers only.

    A contiguous f32 HIP tensor [B, 3 n] of 2..64 atoms at a scalar temperature runs on csrc/bgk_molecule.hip (energy, gradient, KL loss
    sums; ``force`` is then the backward launch alone); ``fused``: True or "always" (the kernel wherever it applies, DESIGN.md
    "Molecular mechanics energy"), False (the torch formulas).  Everything else -- CPU, f64, strided rows, second derivatives, more
    atoms or terms than the kernel's envelope -- runs the torch formulas, which form angles and dihedrals with ``atan2``.

    Out of scope: periodic boxes and cutoffs, constraints, other Generalised Born models, CMAP and other torsion forms, chain kernels for MCMC /
    HMC on this target (the samplers run their torch path on it), and folding ``LinLogCutEnergy`` / ``GradientClippedEnergy`` into the
    launch (the wrappers evaluate this energy and apply their own stand-alone kernels)."""
    fused = True

    def __init__(self, n_atoms, bonds=None, angles=None, torsions=None, nonbonded=None, exceptions=None, unit_energy=1.0,
                 implicit_solvent=None, solute_dielectric=1.0, solvent_dielectric=78.5, surface_area_energy=2.25936):
        if not (isinstance(n_atoms, (int, np.integer)) and n_atoms >= 1):
            raise ValueError(f"MolecularMechanicsEnergy: n_atoms must be a positive integer, got {n_atoms!r}")
        n_atoms = int(n_atoms)
        super().__init__(3 * n_atoms)
        if not (_is_number(unit_energy) and unit_energy > 0):
            raise ValueError(f"MolecularMechanicsEnergy: unit_energy must be a positive number, got {unit_energy!r}")
        self.n_atoms, self.unit_energy = n_atoms, float(unit_energy)
        given = {"bond": bonds, "angle": angles, "torsion": torsions, "exception": exceptions}
        for group, (width, floats, ints) in _GROUPS.items():
            arg, parts = _ARGS[group], given[group]
            if parts is None:
                parts = (np.zeros((0, width), np.int64),) + tuple(np.zeros(0) for _ in floats + ints)
            if len(parts) != 1 + len(floats) + len(ints):
                raise ValueError(f"MolecularMechanicsEnergy: {arg} must be (idx, {', '.join(ints + floats)})")
            idx = _index(parts[0], width, n_atoms, group)
            self.register_buffer(f"{group}_idx", torch.from_numpy(idx))
            named = dict(zip(ints + floats, parts[1:]))
            for name in ints:
                v = np.asarray(named[name].detach().cpu().numpy() if torch.is_tensor(named[name]) else named[name]).reshape(-1)
                if len(v) != len(idx) or (len(v) and not np.issubdtype(v.dtype, np.integer)):
                    raise ValueError(f"MolecularMechanicsEnergy: {arg}: {name} must be {len(idx)} integers")
                self.register_buffer(f"{group}_{name}", torch.from_numpy(v.astype(np.int64)))
            for name in floats:
                v = _f64(named[name], f"{group} {name}")
                if len(v) != len(idx):
                    raise ValueError(f"MolecularMechanicsEnergy: {arg}: {name} has {len(v)} entries for {len(idx)} terms")
                self.register_buffer(f"{group}_{name}", torch.from_numpy(v.copy()))
        for t in np.flatnonzero(~(self.bond_r0.numpy() > 0)):
            raise ValueError(f"MolecularMechanicsEnergy: bond term {int(t)} {tuple(self.bond_idx[t].tolist())} has r0 <= 0")
        for t in np.flatnonzero((self.torsion_periodicity.numpy() < 1) | (self.torsion_periodicity.numpy() > 6)):
            raise ValueError(f"MolecularMechanicsEnergy: torsion term {int(t)} {tuple(self.torsion_idx[t].tolist())} has periodicity "
                             f"{int(self.torsion_periodicity[t])} outside 1..6")
        for t in np.flatnonzero(~(self.exception_sigma.numpy() > 0)):
            raise ValueError(f"MolecularMechanicsEnergy: exception term {int(t)} {tuple(self.exception_idx[t].tolist())} has sigma <= 0")
        seen = {}
        for t, (i, j) in enumerate(self.exception_idx.tolist()):
            pair = (min(i, j), max(i, j))
            if pair in seen:
                raise ValueError(f"MolecularMechanicsEnergy: exception term {t} {(i, j)} names the pair of exception term {seen[pair]}")
            seen[pair] = t
        self.has_nonbonded = nonbonded is not None
        if nonbonded is None:
            if len(self.exception_idx):
                raise ValueError("MolecularMechanicsEnergy: exceptions need the nonbonded tables")
            nonbonded = (np.zeros(0), np.zeros(0), np.zeros(0))
        if len(nonbonded) != 3:
            raise ValueError("MolecularMechanicsEnergy: nonbonded must be (charge, sigma, epsilon)")
        for name, v in zip(("charge", "sigma", "epsilon"), nonbonded):
            v = _f64(v, f"nonbonded {name}")
            if self.has_nonbonded and len(v) != n_atoms:
                raise ValueError(f"MolecularMechanicsEnergy: nonbonded {name} has {len(v)} entries for {n_atoms} atoms")
            self.register_buffer(f"nonbonded_{name}", torch.from_numpy(v.copy()))
        for t in np.flatnonzero(~(self.nonbonded_sigma.numpy() > 0)):
            raise ValueError(f"MolecularMechanicsEnergy: nonbonded atom {int(t)} has sigma <= 0")
        for t in np.flatnonzero(self.nonbonded_epsilon.numpy() < 0):
            raise ValueError(f"MolecularMechanicsEnergy: nonbonded atom {int(t)} has epsilon < 0")
        self.has_solvent = implicit_solvent is not None
        for name, v in (("solute_dielectric", solute_dielectric), ("solvent_dielectric", solvent_dielectric)):
            if not (_is_number(v) and np.isfinite(v) and v > 0):
                raise ValueError(f"MolecularMechanicsEnergy: {name} must be a positive number, got {v!r}")
        if not (_is_number(surface_area_energy) and np.isfinite(surface_area_energy) and surface_area_energy >= 0):
            raise ValueError(f"MolecularMechanicsEnergy: surface_area_energy must be a non-negative number, got {surface_area_energy!r}")
        self.solute_dielectric, self.solvent_dielectric = float(solute_dielectric), float(solvent_dielectric)
        self.surface_area_energy = float(surface_area_energy)
        if self.has_solvent:
            if len(implicit_solvent) != 3:
                raise ValueError("MolecularMechanicsEnergy: implicit_solvent must be (charge, radius, scale)")
            for name, v in zip(("charge", "radius", "scale"), implicit_solvent):
                v = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
                if len(v) != n_atoms:
                    raise ValueError(f"MolecularMechanicsEnergy: implicit_solvent {name} has {len(v)} entries for {n_atoms} atoms")
                for t in np.flatnonzero(~np.isfinite(v)):
                    raise ValueError(f"MolecularMechanicsEnergy: implicit_solvent atom {int(t)} has a non-finite {name}")
                self.register_buffer(f"solvent_{name}", torch.from_numpy(v.copy()))
            for t in np.flatnonzero(~(self.solvent_radius.numpy() > GB_OFFSET)):
                raise ValueError(f"MolecularMechanicsEnergy: implicit_solvent atom {int(t)} has radius <= {GB_OFFSET}")
            for t in np.flatnonzero(~(self.solvent_scale.numpy() > 0)):
                raise ValueError(f"MolecularMechanicsEnergy: implicit_solvent atom {int(t)} has scale <= 0")

    n_bonds = property(lambda self: len(self.bond_idx))
    n_angles = property(lambda self: len(self.angle_idx))
    n_torsions = property(lambda self: len(self.torsion_idx))
    n_pairs = property(lambda self: self.n_atoms * (self.n_atoms - 1) // 2 if self.has_nonbonded else 0)

    # ---- the tables as arrays ----
    def to_arrays(self):
        """the tables as a dict of numpy arrays (numbers only): ``n_atoms``, ``unit_energy``, ``has_nonbonded`` and every buffer"""
        out = {"n_atoms": np.array(self.n_atoms, np.int64), "unit_energy": np.array(self.unit_energy, np.float64),
               "has_nonbonded": np.array(int(self.has_nonbonded), np.int64)}
        out.update({name: buf.detach().cpu().numpy().copy() for name, buf in self.named_buffers()})
        if self.has_solvent:                # (the three solvent arrays are buffers)
            out.update(has_solvent=np.array(1, np.int64), solute_dielectric=np.array(self.solute_dielectric, np.float64),
                       solvent_dielectric=np.array(self.solvent_dielectric, np.float64),
                       surface_area_energy=np.array(self.surface_area_energy, np.float64))
        return out

    @classmethod
    def from_arrays(cls, arrays):
        a = {k: np.asarray(v) for k, v in dict(arrays).items()}

        def group(g):
            _, floats, ints = _GROUPS[g]
            return (a[f"{g}_idx"].astype(np.int64),) + tuple(a[f"{g}_{name}"] for name in ints + floats)

        nonbonded = tuple(a[f"nonbonded_{name}"] for name in ("charge", "sigma", "epsilon")) if int(a["has_nonbonded"]) else None
        solvent = {}
        if int(a.get("has_solvent", 0)):
            solvent = dict(implicit_solvent=tuple(a[f"solvent_{name}"] for name in ("charge", "radius", "scale")),
                           **{name: float(a[name]) for name in ("solute_dielectric", "solvent_dielectric", "surface_area_energy")})
        return cls(int(a["n_atoms"]), group("bond"), group("angle"), group("torsion"), nonbonded, group("exception"),
                   unit_energy=float(a["unit_energy"]), **solvent)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **self.to_arrays())

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_arrays({k: z[k] for k in z.files})

    # ---- host tables, rebuilt when a buffer changes (its storage, version, dtype or device: ``.to()``, ``load_state_dict``) ----
    def _tables(self):
        key = tuple((b.data_ptr(), b._version, b.dtype, b.device) for _, b in self.named_buffers())
        hit = self.__dict__.get("_mm_tables")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_mm_tables"] = (key, {}, {})
        return hit

    def _host(self, name):
        """a buffer as an f64 (int64) host array"""
        b = getattr(self, name).detach().cpu()
        return b.numpy().astype(np.float64 if b.is_floating_point() else np.int64)

    def pair_table(self):
        """the dense pair table over i < j in ascending (i, j) order, f64 [n (n - 1) / 2, 3]: (138.935458 qq_ij, sigma_ij, 4 eps_ij) with the
        combination rules, exclusions and exceptions applied (an excluded pair: qq = 0 and eps = 0); None without nonbonded tables"""
        if not self.has_nonbonded:
            return None
        host = self._tables()[1]
        if "pairs" not in host:
            n = self.n_atoms
            i, j = _pair_index(n)
            q, s, e = (self._host(f"nonbonded_{name}") for name in ("charge", "sigma", "epsilon"))
            t = np.stack([COULOMB * (q[i] * q[j]), 0.5 * (s[i] + s[j]), 4.0 * np.sqrt(e[i] * e[j])], axis=1)
            ex = self._host("exception_idx")
            if len(ex):
                lo, hi = ex.min(axis=1), ex.max(axis=1)
                row = lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)
                t[row] = np.stack([COULOMB * self._host("exception_chargeprod"), self._host("exception_sigma"),
                                   4.0 * self._host("exception_epsilon")], axis=1)
            host["pairs"] = t
        return host["pairs"]

    def _packed_tables(self):
        """the kernel's one table (csrc/bgk_molecule_terms.h), int32 words: bonds [Nb, 4] (i | j << 6, r0, k, 0), angles [Na, 4]
        (i | j << 6 | k << 12, theta0, k, 0), torsions [Nt, 4] (i | j << 6 | k << 12 | l << 18 | n << 24, k, k cos(phase), k sin(phase)),
        pairs [n (n - 1) / 2, 3] (qq, sigma, 4 eps); the floats as their f32 bits, products formed in double and rounded once"""
        host = self._tables()[1]
        if "packed" not in host:
            def block(idx, cols):
                shifts = np.array([0, 6, 12, 18][:idx.shape[1]], np.int64)
                out = np.zeros((len(idx), 4), np.int32)
                out[:, 0] = (idx << shifts).sum(axis=1).astype(np.int32)
                for c, v in enumerate(cols, start=1):
                    out[:, c] = np.asarray(v, np.float64).astype(np.float32).view(np.int32)
                return out

            bonds = block(self._host("bond_idx"), [self._host("bond_r0"), self._host("bond_k")])
            angles = block(self._host("angle_idx"), [self._host("angle_theta0"), self._host("angle_k")])
            k, phase = self._host("torsion_k"), self._host("torsion_phase")
            tors = block(self._host("torsion_idx"), [k, k * np.cos(phase), k * np.sin(phase)])
            tors[:, 0] |= (self._host("torsion_periodicity") << 24).astype(np.int32)
            pairs = self.pair_table()
            pairs = np.zeros((0, 3), np.int32) if pairs is None else pairs.astype(np.float32).view(np.int32)
            words = np.concatenate([t.reshape(-1) for t in (bonds, angles, tors, pairs)] + [np.zeros(4, np.int32)])
            host["packed"] = np.ascontiguousarray(words)
        return host["packed"]

    def gb_prefactor(self):
        """-138.935458 (1 / solute_dielectric - 1 / solvent_dielectric), in double"""
        return -COULOMB * (1.0 / self.solute_dielectric - 1.0 / self.solvent_dielectric)

    def _packed_solvent(self):
        """the kernel's solvent table (csrc/bgk_solvent_terms.h), f32: [n, 4] (q_i, rho_i = r_i - 0.009, sigma_i = s_i rho_i, r_i), then [n]
        sa_i = 4 pi surface_area_energy (r_i + 0.14)^2 r_i^6, padded to a multiple of four words; formed in double and rounded once"""
        host = self._tables()[1]
        if "solvent" not in host:
            q, r, sc = (self._host(f"solvent_{name}") for name in ("charge", "radius", "scale"))
            rho = r - GB_OFFSET
            atoms = np.stack([q, rho, sc * rho, r], axis=1)
            sa = 4.0 * np.pi * self.surface_area_energy * (r + GB_PROBE) ** 2 * r ** 6
            words = np.concatenate([atoms.reshape(-1), sa, np.zeros(-len(sa) % 4)])
            host["solvent"] = np.ascontiguousarray(words.astype(np.float32))
        return host["solvent"]

    def _device_solvent(self, device):
        packed = self._packed_solvent()
        cache = self._tables()[2]
        key = ("solvent", str(device))
        if key not in cache:
            cache[key] = torch.from_numpy(packed).to(device)
        return cache[key]

    def _device_tables(self, device):
        packed = self._packed_tables()
        cache = self._tables()[2]
        key = ("packed", str(device))
        if key not in cache:
            cache[key] = torch.from_numpy(packed).to(device)
        return cache[key]

    def _torch_tables(self, device, dtype):
        """the float tables of the torch formulas on ``device`` in ``dtype`` (the pairs: only those that interact)"""
        cache = self._tables()[2]
        key = ("torch", str(device), dtype)
        if key not in cache:
            t = {}
            for group, (_, floats, ints) in _GROUPS.items():
                if group == "exception":
                    continue
                t[f"{group}_idx"] = getattr(self, f"{group}_idx").to(device)
                for name in floats:
                    t[f"{group}_{name}"] = getattr(self, f"{group}_{name}").to(device=device, dtype=dtype)
            t["torsion_n"] = self.torsion_periodicity.to(device=device, dtype=dtype)
            pairs = self.pair_table()
            if pairs is not None:
                i, j = _pair_index(self.n_atoms)
                live = (pairs[:, 0] != 0) | (pairs[:, 2] != 0)
                t["pair_i"], t["pair_j"] = torch.from_numpy(i[live]).to(device), torch.from_numpy(j[live]).to(device)
                t["pair_qq"], t["pair_sigma"], t["pair_eps4"] = (torch.from_numpy(pairs[live, c]).to(device=device, dtype=dtype) for c in range(3))
            if self.has_solvent:
                n = self.n_atoms
                q, r, sc = (getattr(self, f"solvent_{name}").to(device=device, dtype=dtype) for name in ("charge", "radius", "scale"))
                i, j = _pair_index(n)
                t.update(gb_q=q, gb_r=r, gb_rho=r - GB_OFFSET, gb_sigma=sc * (r - GB_OFFSET), gb_i=torch.from_numpy(i).to(device),
                         gb_j=torch.from_numpy(j).to(device), gb_eye=torch.eye(n, dtype=torch.bool, device=device))
            cache[key] = t
        return cache[key]

    # ---- general path ----
    def _energy(self, x):
        """E / unit_energy of x [..., 3 n] in torch ops: [..., 1]"""
        t = self._torch_tables(x.device, x.dtype)
        lead = x.shape[:-1]
        p = x.reshape(-1, self.n_atoms, 3)
        e = torch.zeros(p.shape[0], dtype=x.dtype, device=x.device)
        if self.n_bonds:
            i, j = t["bond_idx"].unbind(1)
            r = (p[:, i] - p[:, j]).pow(2).sum(-1).sqrt()
            e = e + (0.5 * t["bond_k"] * (r - t["bond_r0"]) ** 2).sum(-1)
        if self.n_angles:
            i, j, k = t["angle_idx"].unbind(1)
            a, b = p[:, i] - p[:, j], p[:, k] - p[:, j]
            theta = torch.atan2(torch.linalg.cross(a, b).pow(2).sum(-1).sqrt(), (a * b).sum(-1))
            e = e + (0.5 * t["angle_k"] * (theta - t["angle_theta0"]) ** 2).sum(-1)
        if self.n_torsions:
            i, j, k, l = t["torsion_idx"].unbind(1)
            b1, b2, b3 = p[:, j] - p[:, i], p[:, k] - p[:, j], p[:, l] - p[:, k]
            n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
            phi = torch.atan2(b2.pow(2).sum(-1).sqrt() * (b1 * n2).sum(-1), (n1 * n2).sum(-1))
            e = e + (t["torsion_k"] * (1 + torch.cos(t["torsion_n"] * phi - t["torsion_phase"]))).sum(-1)
        if "pair_i" in t and len(t["pair_i"]):
            d2 = (p[:, t["pair_i"]] - p[:, t["pair_j"]]).pow(2).sum(-1)
            apart = d2 > 0
            d2s = torch.where(apart, d2, torch.ones_like(d2))
            s6 = (t["pair_sigma"] ** 2 / d2s) ** 3
            pair = t["pair_eps4"] * (s6 * s6 - s6) + t["pair_qq"] * d2s.rsqrt()
            e = e + torch.where(apart, pair, torch.full_like(pair, float("inf"))).sum(-1)
        if self.has_solvent:
            e = e + self._solvent_energy(p, t)
        return (e / self.unit_energy).reshape(*lead, 1)

    def _solvent_energy(self, p, t):
        """E_GB + E_SA [B] of the positions p [B, n, 3] (GBSAOBCForce's arithmetic, OBC2) in torch ops; +inf where two atoms coincide.  Every
        branch is a ``torch.where`` over values formed from safe arguments, so no NaN reaches a gradient."""
        eye = t["gb_eye"]
        d2 = (p[:, :, None] - p[:, None, :]).pow(2).sum(-1)                   # [B, n, n]: atom i along dim 1, atom j along dim 2
        apart = (d2 > 0) | eye
        d2s = torch.where((d2 > 0) & ~eye, d2, torch.ones_like(d2))
        r = d2s.sqrt()
        rho, sigma = t["gb_rho"][:, None], t["gb_sigma"][None, :]
        l = 1.0 / torch.maximum(rho.expand_as(r), (r - sigma).abs())
        u = 1.0 / (r + sigma)
        l2u2 = l * l - u * u
        h = l - u - 0.25 * r * l2u2 + 0.5 * torch.log(u / l) / r + 0.25 * sigma ** 2 * l2u2 / r
        h = h + torch.where(rho < sigma - r, 2.0 * (1.0 / rho - l), torch.zeros_like(h))
        h = torch.where((rho >= r + sigma) | eye, torch.zeros_like(h), h)
        psi = 0.5 * t["gb_rho"] * h.sum(-1)                                   # [B, n]
        inv_b = 1.0 / t["gb_rho"] - torch.tanh(GB_ALPHA * psi - GB_BETA * psi ** 2 + GB_GAMMA * psi ** 3) / t["gb_r"]
        born = 1.0 / inv_b
        i, j = t["gb_i"], t["gb_j"]
        r2, bb = d2s[:, i, j], born[:, i] * born[:, j]
        f = (r2 + bb * torch.exp(-r2 / (4.0 * bb))).sqrt()
        q = t["gb_q"]
        e_gb = self.gb_prefactor() * ((q[i] * q[j] / f).sum(-1) + (0.5 * q * q * inv_b).sum(-1))
        e_sa = (4.0 * np.pi * self.surface_area_energy * (t["gb_r"] + GB_PROBE) ** 2 * (t["gb_r"] * inv_b) ** 6).sum(-1)
        return torch.where(apart.all(-1).all(-1), e_gb + e_sa, torch.full_like(e_gb, float("inf")))

    # ---- the kernel path ----
    def _molecule_kernel(self, temperature=1.0):
        """the MoleculePlan of this energy at ``temperature``, or None (then the torch formulas run)"""
        if self.fused is False or not (_is_number(temperature) and temperature > 0):
            return None
        if not (2 <= self.n_atoms <= MOLECULE_MAX_ATOMS and self.n_bonds <= MOLECULE_MAX_BONDS and self.n_angles <= MOLECULE_MAX_ANGLES
                and self.n_torsions <= MOLECULE_MAX_TORSIONS):
            return None
        return MoleculePlan(self, self.n_atoms, self.unit_energy, float(temperature))

    def energy(self, x, temperature=1.0):
        if torch.is_tensor(x) and x.dim() == 2:
            fast = kernel_energy(self, (x,), temperature)
            if fast is not None:
                return fast
        return super().energy(x, temperature=temperature)

    def _kernel_force(self, x):
        """-d u / d x of a kernel input as ONE launch of bgk_molecule_energy_backward (g_u = -1), else None"""
        plan = _kernel_plan(self, 1.0)
        if not isinstance(plan, MoleculePlan) or not torch.is_tensor(x):
            return None
        ops = _kernel_operands(plan, (x.detach(),))
        if ops is None:
            return None
        g = torch.full((x.shape[0],), -1.0, dtype=torch.float32, device=x.device)
        return _launch_backward(plan, ops[1], ops[0], g_u=g)[0]

    def force(self, x, temperature=1.0):
        """``-d energy(x, temperature) / d x``; on the fused path the backward launch alone"""
        fast = self._kernel_force(x) if _is_number(temperature) and temperature == 1.0 else None
        if fast is not None:
            return fast
        with torch.enable_grad():
            xg = x.detach().requires_grad_(True)
            return -torch.autograd.grad(self.energy(xg, temperature=temperature).sum(), xg)[0]
