"""No GPU: bgflow_amd.free_energy on the CPU (the torch path of the solver) against tests/golden/free_energy.npz, the public function's
interface and import paths, and what csrc/bgk_bar.hip shows without a device: its prototype in the header, in ``abi_signatures`` and in
the built library, with the argument checks.  Bounds: free_energy_common.py."""
import ctypes
import inspect
import json
import math
import sys
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib
from bgflow_amd import free_energy as fe
from bgflow_amd._abi import HEADER, abi_signatures
from bgflow_amd.build import abi_symbols

from free_energy_common import check_record, delta_bound, finite_cases, works

CASES = ["pos", "neg", "far", "scales", "ragged", "tiny", "single", "expand_a", "expand_b", "nooverlap"]
f64, i32, i64, p = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
WANT = [p, i64, p, i64, i32, i32, i32, p, p, i32, f64, i32, p]


def test_the_fixture_lists_the_cases(golden):
    G = golden("free_energy")
    assert json.loads(str(G["cases"])) == CASES and finite_cases(G) == CASES[:-1]
    assert sum(G[f"{c}_{k}"].nbytes for c in CASES for k in ("wf", "wr")) < 70000
    assert all(G[f"{c}_{k}"].dtype == np.float32 for c in CASES for k in ("wf", "wr"))
    assert abs(float(G["neg_delta_default"]) - float(G["neg_delta64"])) > 1e-8        # the reference's early exit, DESIGN.md


def test_signature_is_the_references(golden):
    meta = json.loads(str(golden("free_energy")["meta"]))["bennett_acceptance_ratio"]
    got = [[q.name, "<required>" if q.default is inspect.Parameter.empty else q.default]
           for q in inspect.signature(bg.bennett_acceptance_ratio).parameters.values()]
    assert got == meta
    got = [[q.name, q.default] for q in inspect.signature(bg.bar_solve).parameters.values()][2:]
    assert got == [["maximum_iterations", 500], ["relative_tolerance", 1e-12], ["path", None]]


def test_import_paths():
    import bgflow_amd.utils.free_energy as alias
    assert alias.bennett_acceptance_ratio is bg.bennett_acceptance_ratio
    assert bg.utils.bennett_acceptance_ratio is bg.bennett_acceptance_ratio
    assert sys.modules["bgflow_amd.utils.free_energy"] is alias and bg.utils.free_energy is alias


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", CASES)
def test_torch_path_meets_the_fixture(golden, case, dtype):
    G = golden("free_energy")
    wf, wr = works(G, case, dtype)
    r = bg.bar_solve(wf, wr)
    check_record(G, case, r, label=f"torch {dtype} ")
    assert r.delta_f.device.type == "cpu"
    assert bg.bar_solve(wf, wr, path="torch").delta_f.equal(r.delta_f) or case == "nooverlap"
    with pytest.raises(ValueError):
        bg.bar_solve(wf, wr, path="kernel")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", CASES[:-1])
def test_public_function_returns_the_inputs_dtype(golden, case, dtype):
    G = golden("free_energy")
    wf, wr = works(G, case, dtype)
    d, u = bg.bennett_acceptance_ratio(wf, wr)
    d64 = float(G[f"{case}_delta64"])
    assert d.dtype == dtype and u.dtype == dtype and d.dim() == 0 and u.dim() == 0
    bound = 2.0 ** -23 * abs(d64) + 1e-10 if dtype == torch.float32 else delta_bound(d64)
    print(f"{case} {dtype}: {float(d):.10g} err {abs(float(d) - d64):.2e} / {bound:.2e}")
    assert abs(float(d) - d64) <= bound


def test_single_meets_the_closed_form(golden):
    G = golden("free_energy")
    wf, wr = works(G, "single", torch.float64)
    r = bg.bar_solve(wf, wr)
    assert abs(float(r.delta_f) - (float(wf) - float(wr)) / 2) <= 1e-12
    assert abs(float(r.delta_f) - 0.45) < 1e-7 and float(r.uncertainty) == 0.0


def test_far_with_two_iterations_is_the_references_second_iterate(golden):
    G = golden("free_energy")
    r = bg.bar_solve(*works(G, "far", torch.float64), maximum_iterations=2)
    ref = float(G["far_it2"])
    assert r.status == fe.BUDGET and fe.STATUS_NAMES[r.status] == "budget exhausted" and r.n_iterations == 2
    assert abs(float(r.delta_f) - ref) <= delta_bound(ref)
    assert abs(ref - float(G["far_delta64"])) > 100 * delta_bound(ref)       # (the second iterate is not yet the root: 5.4e-7 off)


def test_negative_estimate_is_a_root(golden):
    """the reference leaves its loop after one secant step when the estimate is negative (``neg``: off the root by 2.2e-7)"""
    G = golden("free_energy")
    r = bg.bar_solve(*works(G, "neg", torch.float64))
    assert float(r.delta_f) < 0 and abs(float(r.residual)) <= 1e-9 and r.n_iterations > 1


def test_no_overlap_gives_the_nan_pair_and_the_warning(golden):
    wf, wr = works(golden("free_energy"), "nooverlap")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d, u = bg.bennett_acceptance_ratio(wf, wr)                    # warn=False: silent
        assert math.isnan(float(d)) and math.isnan(float(u)) and d.dtype == torch.float32
        d, u = bg.bennett_acceptance_ratio(wf, wr, compute_uncertainty=False)
        assert math.isnan(float(d)) and math.isnan(float(u))          # the reference's NaN pair (:160)
    with pytest.warns(UserWarning, match="BAR could not compute free energy differences"):
        bg.bennett_acceptance_ratio(wf, wr, warn=True)


def test_expansions_beyond_the_budget_end_with_no_root(golden):
    """the reference's expansion loop has no end of its own; here ``maximum_iterations`` bounds it too (``expand_a`` needs 3)"""
    G = golden("free_energy")
    r = bg.bar_solve(*works(G, "expand_a", torch.float64), maximum_iterations=2)
    assert r.status == fe.NO_ROOT and fe.STATUS_NAMES[r.status] == "no root" and r.n_expansions == 2 and r.n_evaluations == 6
    assert math.isnan(float(r.delta_f)) and math.isnan(float(r.uncertainty)) and r.n_iterations == 0
    d, u = bg.bennett_acceptance_ratio(*works(G, "expand_a"), maximum_iterations=2)
    assert math.isnan(float(d)) and math.isnan(float(u))


def test_interface(golden):
    G = golden("free_energy")
    wf, wr = works(G, "pos", torch.float64)
    d, u = bg.bennett_acceptance_ratio(wf, wr, compute_uncertainty=False)
    assert u is None and d.dim() == 0
    d2, _ = bg.bennett_acceptance_ratio(wf[:, None], wr.reshape(-1, 2, 1))            # [N, 1] energies and any other shape
    wide_f, wide_r = torch.zeros(wf.numel(), 3, dtype=wf.dtype), torch.zeros(wr.numel(), 2, dtype=wr.dtype)
    wide_f[:, 1], wide_r[:, 0] = wf, wr
    d3, _ = bg.bennett_acceptance_ratio(wide_f[:, 1], wide_r[:, :1])                  # strided
    assert d2.equal(d) and d3.equal(d)
    for a, b in ((wf[:0], wr), (wf, wr[:0])):
        with pytest.raises(ValueError):
            bg.bennett_acceptance_ratio(a, b)
        with pytest.raises(ValueError):
            bg.bar_solve(a, b)
    with pytest.raises(ValueError):
        bg.bar_solve(wf, wr, path="fastest")
    with pytest.raises(ImportError):
        bg.bennett_acceptance_ratio(wf, wr, implementation="pymbar")                  # pymbar is not a dependency
    with pytest.raises(KeyError):
        bg.bennett_acceptance_ratio(wf, wr, implementation="other")


def test_inputs_that_require_grad_take_the_torch_path(golden):
    G = golden("free_energy")
    wf, wr = works(G, "pos", torch.float64)
    plain = bg.bar_solve(wf, wr)
    wf, wr = wf.clone().requires_grad_(True), wr.clone().requires_grad_(True)
    r = bg.bar_solve(wf, wr)
    assert r.delta_f.grad_fn is not None and r.uncertainty.grad_fn is not None
    assert r.delta_f.detach().equal(plain.delta_f)                   # the value is the solver's
    gf, gr = torch.autograd.grad(r.delta_f, (wf, wr))
    # a shift of every work value moves the root with it: d delta / d wF sums with -d delta / d wR to one
    assert abs(float(gf.sum()) - float(gr.sum()) - 1.0) <= 1e-9
    # ... and the derivative by finite differences on one forward work value
    h = 1e-4
    with torch.no_grad():
        up, down = wf.detach().clone(), wf.detach().clone()
        up[3] += h
        down[3] -= h
        fd = (float(bg.bar_solve(up, wr.detach()).delta_f) - float(bg.bar_solve(down, wr.detach()).delta_f)) / (2 * h)
        assert bg.bar_solve(wf, wr).delta_f.grad_fn is None
    assert abs(float(gf[3]) - fd) <= 1e-6 * max(1.0, abs(fd)) + 1e-8
    d, u = bg.bennett_acceptance_ratio(wf.float(), wr.float())
    assert d.grad_fn is not None and u.grad_fn is not None and d.dtype == torch.float32


def test_the_prototype_is_declared_parsed_and_exported(hip_lib):
    sigs = abi_signatures()
    assert sigs["bgk_bar_solve_steps"] == (ctypes.c_int, WANT)
    assert "bgk_bar_solve_steps" in abi_symbols()
    assert list(hip_lib.bgk_bar_solve_steps.argtypes) == WANT
    assert ctypes.cast(ctypes.CDLL(_lib.LIB_PATH).bgk_bar_solve_steps, ctypes.c_void_p).value, "bgk_bar_solve_steps is not exported"
    with open(HEADER) as f:
        header = f.read()
    assert f"#define BGK_BAR_RECORD_DOUBLES {fe.RECORD_DOUBLES}\n" in header
    assert "#define BGK_BAR_F32 0\n" in header and "#define BGK_BAR_F64 1\n" in header and fe._DTYPE_CODES == {torch.float32: 0, torch.float64: 1}


def test_argument_checks_of_the_entry(hip_lib):
    fake = ctypes.c_void_p(64)              # never dereferenced: every check comes before the first launch

    def call(wf=fake, nf=8, wr=fake, nr=8, dtype=0, nbf=1, nbr=1, partial=fake, record=fake, max_iter=500, rtol=1e-12, n_steps=0):
        return hip_lib.bgk_bar_solve_steps(wf, nf, wr, nr, dtype, nbf, nbr, partial, record, max_iter, rtol, n_steps, None)

    assert call() == 0                                               # n_steps == 0: nothing is launched
    for bad in (dict(wf=None), dict(wr=None), dict(partial=None), dict(record=None)):
        assert call(**bad) == -1 and b"null pointer" in hip_lib.bgk_last_error()
    assert call(nf=-1) == -1 and call(nr=-1) == -1 and call(nf=0) == -1 and b"sizes" in hip_lib.bgk_last_error()
    assert call(dtype=2) == -1 and b"dtype" in hip_lib.bgk_last_error() and call(dtype=-1) == -1
    assert call(dtype=1) == 0 and call(wf=ctypes.c_void_p(68)) == 0                  # a 4-byte aligned f32 pointer is fine
    assert call(wf=ctypes.c_void_p(68), dtype=1) == -1 and call(wr=ctypes.c_void_p(66)) == -1 and b"aligned" in hip_lib.bgk_last_error()
    assert call(nbf=0) == -1 and call(nbr=513) == -1 and call(nbr=512) == 0
    assert call(max_iter=0) == -1 and b"maximum_iterations" in hip_lib.bgk_last_error() and call(max_iter=-3) == -1
    assert call(n_steps=-1) == -1
