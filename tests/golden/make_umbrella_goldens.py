#!/usr/bin/env python
"""Generate tests/golden/umbrella.npz by IMPORTING the reference (CPU only, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_umbrella_goldens.py

It does not import bgflow_amd.  The fixture holds DATA only; it is written with fixed zip time stamps, so the script regenerates it bit
for bit.  The toy system, the cases and their seeds are in tests/umbrella_common.py.

(a) The UNMODIFIED ``bgflow/distribution/sampling/_mcmc/umbrella_sampling.py`` and ``metropolis.py``, loaded by path, on a 1-d double
    well given as a numpy callable, rc = x[:, 0]: 4 umbrellas, k = 10, centres -1 .. 1, 200 steps each, noise 0.2, for both values of
    ``forward_backward``, under ``np.random.seed``.  Stored: ``umbrella_positions``, ``rc_trajs``, ``bias_energies`` and
    ``umbrella_free_energies()``, each in the dtype the reference returns.  Two things the reference needs to get that far:
      * its loop assigns the ``UmbrellaModel`` itself to ``sampler.energy_function`` and its ``MetropolisGauss`` calls that attribute,
        but the model has no ``__call__``.  The sampler used here is a subclass of the reference's whose ``energy_function`` property
        stores ``model.energy`` when it is handed a model -- no arithmetic and no random call changes;
      * ``umbrella_free_energies`` imports ``bar`` from ``deep_boltzmann.sampling.analysis``, a package that does not exist.  A stand-in
        module of that name is put into ``sys.modules`` whose ``bar`` is the reference's own ``_mcmc/analysis.py::bar`` (as
        nflows_stub.py stands in for nflows).
(b) MBAR cases with the window free energies f from an INDEPENDENT method.  The reference's own ``mbar`` cannot make these numbers: it
    imports pyemma, which is not installed here (nor is pymbar).  Expected values: ``scipy.optimize.minimize`` (BFGS, analytic gradient)
    of the convex MBAR objective  sum_n D_n(f) - sum_k N_k f_k,  D_n = log sum_l N_l exp(f_l - kappa_l (r_n - m_l)^2),  in f64 with f_0
    fixed at 0, whose gradient S_k - N_k vanishes exactly at the fixed point of the self-consistent iteration.  The samples are stored
    as float32 and the expected values are computed on their exact widening to f64.  Beside BFGS the script runs its own numpy
    restatement of the iteration (f64, tolerance 1e-12) and records, per case, its iteration count and its largest disagreement with
    BFGS; ``b_agreement`` is the largest over all cases, and ten times that is the bound the tests assert for any path (BFGS stops on
    its own gradient tolerance).
"""
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import umbrella_common as uc       # noqa: E402


def load_reference(name):
    path = os.path.join(os.environ["BGFLOW_REFERENCE"], "bgflow", "distribution", "sampling", "_mcmc", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (a zip archive of .npy members)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def part_a(out):
    ref_us, ref_mc, ref_an = load_reference("umbrella_sampling"), load_reference("metropolis"), load_reference("analysis")
    stand_in = types.ModuleType("deep_boltzmann.sampling.analysis")
    stand_in.bar = ref_an.bar
    for name in ("deep_boltzmann", "deep_boltzmann.sampling"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["deep_boltzmann.sampling.analysis"] = stand_in

    class Sampler(ref_mc.MetropolisGauss):
        @property
        def energy_function(self):
            return self._energy_function

        @energy_function.setter
        def energy_function(self, value):
            self._energy_function = value.energy if isinstance(value, ref_us.UmbrellaModel) else value

    for fb in (False, True):
        np.random.seed(uc.A_SEED)
        sampler = Sampler(uc.double_well, uc.A_X0, noise=uc.A_NOISE)
        us = ref_us.UmbrellaSampling(uc.double_well, sampler, uc.first_coordinate, uc.A_X0, uc.A_N_UMBRELLA, uc.A_K, uc.A_M_MIN, uc.A_M_MAX,
                                     forward_backward=fb)
        us.run(nsteps=uc.A_NSTEPS, verbose=False)
        key = uc.a_key(fb)
        out[key + "_positions"] = us.umbrella_positions
        out[key + "_rc_trajs"] = np.stack(us.rc_trajs)
        out[key + "_bias_energies"] = np.stack(us.bias_energies)
        out[key + "_free_energies"] = us.umbrella_free_energies()
        n = uc.A_N_UMBRELLA * (2 if fb else 1)
        assert out[key + "_rc_trajs"].shape == (n, uc.A_NSTEPS + 1) and out[key + "_rc_trajs"].dtype == np.float32
        assert np.isfinite(out[key + "_free_energies"]).all() and out[key + "_free_energies"].shape == (n,)
        moved = [np.unique(t).size for t in us.rc_trajs]
        assert min(moved) > 20, moved                                   # the chains accept


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def log_denominators(r, N, m, kappa, f):
    a = (np.log(N) + f)[None, :] - kappa[None, :] * (r[:, None] - m[None, :]) ** 2
    mx = a.max(1)
    D = mx + np.log(np.exp(a - mx[:, None]).sum(1))
    return D, a


def iterate(r, N, m, kappa, tolerance, maximum_iterations=100000):
    """the self-consistent iteration, restated in numpy f64"""
    f = np.zeros(N.size)
    for it in range(1, maximum_iterations + 1):
        D, a = log_denominators(r, N, m, kappa, f)
        S = np.exp(a - D[:, None]).sum(0)
        new = f - (np.log(S) - np.log(N))
        new -= new[0]
        err = np.abs(new - f).max()
        f = new
        if err <= tolerance:
            return f, it
    raise AssertionError("the restatement did not converge")


def bfgs(r, N, m, kappa):
    n = float(N.sum())

    def objective(free):
        f = np.concatenate([[0.0], free])
        D, a = log_denominators(r, N, m, kappa, f)
        S = np.exp(a - D[:, None]).sum(0)
        return (D.sum() - (N * f).sum()) / n, (S - N)[1:] / n

    # BFGS gives up ("precision loss") once its line search no longer resolves the objective; a restart from where it stopped, with a
    # fresh inverse Hessian, gets further.  Restarts go on while they lower the gradient
    x, grad = np.zeros(N.size - 1), np.inf
    for _ in range(20):
        res = minimize(objective, x, jac=True, method="BFGS", options={"gtol": 1e-14, "maxiter": 20000})
        g = float(np.abs(res.jac).max())
        if not g < grad:
            break
        x, grad = res.x, g
    return np.concatenate([[0.0], x]), grad


def part_b(out):
    rng = np.random.default_rng(uc.B_SEED)
    meta, worst = {}, 0.0
    for case, (counts, centres, k) in uc.B_CASES.items():
        N = np.array(counts, np.float64)
        kappa = np.full(N.size, k)
        mean, sd = k * centres / (0.5 + k), np.sqrt(0.5 / (0.5 + k))
        rc = np.concatenate([mu + sd * rng.standard_normal(c) for mu, c in zip(mean, counts)]).astype(np.float32)
        r = rc.astype(np.float64)
        f_it, iterations = iterate(r, N, centres, kappa, uc.B_TOLERANCE)
        if N.size == 1:
            f_ref, grad = np.zeros(1), 0.0
        else:
            f_ref, grad = bfgs(r, N, centres, kappa)
        agreement = float(np.abs(f_it - f_ref).max())
        worst = max(worst, agreement)
        out[f"{case}_rc"] = rc
        out[f"{case}_f"] = f_ref
        meta[case] = {"iterations": iterations, "agreement": agreement, "bfgs_gradient": grad, "f_range": float(np.ptp(f_ref))}
        print(f"{case}: K {N.size} N {int(N.sum())}  iterations {iterations}  |f_iter - f_bfgs| {agreement:.2e}  BFGS |grad| / n {grad:.1e}  "
              f"f range {np.ptp(f_ref):.3f}")
        assert iterations < 100, "the case does not overlap well"
    out["b_agreement"] = np.float64(worst)
    out["b_meta"] = np.array(json.dumps(meta))
    print(f"largest disagreement with BFGS: {worst:.2e}; the tests assert {10 * worst:.2e}")


def main():
    out = {}
    part_a(out)
    part_b(out)
    path = os.path.join(HERE, "umbrella.npz")
    save_npz(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
