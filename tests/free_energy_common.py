"""Shared by the host and GPU tests of bgflow_amd.free_energy: the cases of tests/golden/free_energy.npz (written by
tests/golden/make_free_energy_goldens.py from the reference), the bounds and the check of one solver record against the fixture.

Bounds, and where they come from:

* delta_f against ``delta64`` (the reference run through all 500 iterations in f64; |f(delta64)| <= 1e-12 is asserted when the
  fixture is written): |d - delta64| <= 1e-10 max(1, |delta64|).  The stop rule is 1e-12 relative; a numpy restatement of the solver
  differed from the reference's value by at most 5.5e-13 over 4000 random small cases and seven shapes up to 2^20 / 2^19; the factor of
  about 200 on top covers another summation order.
* uncertainty against ``unc64``: relative 1e-8 where unc64 is finite and positive, PLUS the rounding error of the reference's own
  value.  The reference forms var = A + B - nrat (A + B = var + nrat) from a handful of rounded f64 terms, so its var carries up to
  about 8 eps (var + 2 nrat) of noise, i.e. unc64 is only known to sqrt(unc64^2 + that) - unc64.  At the usual cases this term is below
  1e-14; it matters for ``single`` alone: one sample a side has var = 1 + 1 - 2 = 0 exactly, this package returns 0, and the
  reference's 2.1e-8 is the square root of its rounding noise (4.4e-16).
* the public function on f32 inputs: |d - delta64| <= 2^-23 |delta64| + 1e-10, one rounding to f32.
* the residual f(delta_f): the fixture's cases are roots to 1e-12 in the reference; |residual| <= 1e-9 asked here.
* at most 100 evaluations of f on every finite case (the restatement needed at most 25): a solver that runs to its budget of 500
  iterations still returns the right number, so the count is a condition of its own."""
import json
import math

import torch

from bgflow_amd import free_energy as fe

DELTA_RTOL = 1e-10
UNC_RTOL = 1e-8
RESIDUAL_ATOL = 1e-9
MAX_EVALUATIONS = 100
EPS64 = 2.0 ** -52


def cases(G):
    return json.loads(str(G["cases"]))


def finite_cases(G):
    return [c for c in cases(G) if c != "nooverlap"]


def works(G, case, dtype=torch.float32, device="cpu"):
    """the stored f32 work values of a case, converted (exactly) to ``dtype``"""
    return tuple(torch.from_numpy(G[f"{case}_{k}"]).to(dtype).to(device) for k in ("wf", "wr"))


def delta_bound(ref):
    return DELTA_RTOL * max(1.0, abs(ref))


def uncertainty_bound(unc64, nf, nr):
    nrat = (nf + nr) / (nf * nr)
    reference_noise = math.sqrt(unc64 * unc64 + 8.0 * EPS64 * (unc64 * unc64 + 2.0 * nrat)) - unc64
    return UNC_RTOL * unc64 + reference_noise


def check_record(G, case, r, label=""):
    """one BARResult against the fixture: delta_f, uncertainty, residual, status, the evaluation count; prints every figure first"""
    nf, nr = G[f"{case}_wf"].size, G[f"{case}_wr"].size
    d64, u64 = float(G[f"{case}_delta64"]), float(G[f"{case}_unc64"])
    d, u, res = float(r.delta_f), float(r.uncertainty), float(r.residual)
    print(f"{label}{case}: delta {d:.16g} (err {abs(d - d64):.2e} / {delta_bound(d64):.1e})  unc {u:.10g} (err {abs(u - u64):.2e})  "
          f"residual {res:.2e}  status {r.status}  evaluations {r.n_evaluations}  expansions {r.n_expansions}  iterations {r.n_iterations}")
    for t in (r.delta_f, r.uncertainty, r.residual):
        assert t.dtype == torch.float64 and t.dim() == 0
    if case == "nooverlap":
        assert math.isnan(d) and math.isnan(u) and r.status in (fe.NO_ROOT, fe.NOT_A_NUMBER)
        return
    assert r.status == fe.CONVERGED, fe.STATUS_NAMES[r.status]
    assert abs(d - d64) <= delta_bound(d64)
    if math.isfinite(u64) and u64 > 0:
        assert abs(u - u64) <= uncertainty_bound(u64, nf, nr)
    assert abs(res) <= RESIDUAL_ATOL
    assert r.n_evaluations <= MAX_EVALUATIONS
    assert r.n_evaluations == 2 + 2 * r.n_expansions + r.n_iterations
    if case.startswith("expand"):
        assert r.n_expansions >= 3 and r.n_expansions == int(G[f"{case}_n_expand"])
