"""Free-energy differences from two sets of work values: the Bennett acceptance ratio (utils/free_energy.py).

    f(D) = log sum_i fermi(M + wF_i - D) - log sum_j fermi(wR_j + D - M),   fermi(a) = 1 / (1 + e^a),   M = log(nF / nR)

``bennett_acceptance_ratio`` keeps the reference's signature; ``bar_solve`` returns the whole solver record.  Two paths run ONE state
machine (DESIGN.md "Bennett acceptance ratio"):

* kernel (csrc/bgk_bar.hip): contiguous f32 / f64 work values on one HIP device.  One evaluation of f is two launches (block partials,
  then merge + solver step on the device); the host enqueues ``BAR_CHUNK`` evaluations per call and reads the 18-double record back once
  per chunk.
* torch: the same steps as torch ops in f64 with the solver's scalars on the host (one read of four log-sums per evaluation): CPU
  tensors, other dtypes, inputs that require grad.

The solver: bounds from one-sided exponential averaging (:125-138), the reference's bracket expansion (:142-147) -- stopped with status
``NO_ROOT`` after ``maximum_iterations`` expansions, where the reference would loop on --, then false position with the reference's update
and sign tests (:151-161).  Stop rule: |D - D_old| <= relative_tolerance |D|, D == D_old, f(D) == 0, or ``maximum_iterations`` iterations
(status ``BUDGET``, the last iterate is returned as in the reference).  The reference's own stop test compares with a D_old that is never
reassigned (:149, :163): it runs all iterations for D > 0 and leaves after one for D < 0.  The uncertainty (:170-195) is written with the
log-sums of the last evaluation, var = exp(L2F - 2 L1F) + exp(L2R - 2 L1R) - (nF + nR) / (nF nR), which stays finite where the reference's
exp(...) underflows to 0 / 0.  All arithmetic is f64 whatever the input dtype."""
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import _driver, _lib
from ._driver import BUDGET, CONVERGED, NO_ROOT, NOT_A_NUMBER, R_STATUS, STATUS_NAMES      # NOT_A_NUMBER: neither sign test fired (f is NaN)
from ._driver import DTYPE_CODES as _DTYPE_CODES

__all__ = ["bennett_acceptance_ratio", "bar_solve", "BARResult"]

BARResult = namedtuple("BARResult", ["delta_f", "uncertainty", "residual", "status", "n_evaluations", "n_expansions", "n_iterations",
                                     "n_readbacks"])

BAR_CHUNK = 16                 # evaluations enqueued per host read-back of the record (kernel path)
MAX_BLOCKS = 512               # stage-1 blocks per work array (2 per CU)
MIN_ELEMENTS_PER_BLOCK = 4096  # 16 elements per thread

# the device record (f64), csrc/bgk_bar.hip / include/bgflow_amd.h
RECORD_DOUBLES = 18
(R_UPPER, R_LOWER, R_F_UPPER, R_F_LOWER, R_DELTA, R_DELTA_OLD, R_N_EVAL, R_N_EXPAND, R_N_ITER,
 R_L1F, R_L2F, R_L1R, R_L2R, R_RESIDUAL, R_RESULT, R_UNCERTAINTY) = range(2, RECORD_DOUBLES)      # after R_PHASE, R_STATUS
PHASE_DONE = 4


def _clamp(x, lo=0.1, hi=1e10):
    return lo if x < lo else (hi if x > hi else x)      # (a NaN stays a NaN, as torch.clamp)


def _variance(L, n_forward, n_reverse, exp=torch.exp):
    nrat = float(n_forward + n_reverse) / (float(n_forward) * float(n_reverse))
    return exp(L[1] - 2.0 * L[0]) + exp(L[3] - 2.0 * L[2]) - nrat


def _log_sums(wf, wr, delta, M):
    """[log sum fermi(aF), log sum fermi(aF)^2, log sum fermi(aR), log sum fermi(aR)^2] at ``delta`` (f64 tensor [4])"""
    out = []
    for w, c in ((wf, M - delta), (wr, delta - M)):
        a = w + c
        lf = -(a.clamp(min=0.0) + torch.log1p(torch.exp(-a.abs())))
        out += [torch.logsumexp(lf, 0), torch.logsumexp(2.0 * lf, 0)]
    return torch.stack(out)


def _solve_torch(wf, wr, maximum_iterations, relative_tolerance, stop=True):
    """the state machine of csrc/bgk_bar.hip, scalars on the host in f64; ``stop=False`` keeps iterating to the budget (the
    reference's behaviour for a positive estimate; tools/bar_time.py)"""
    f64 = np.float64
    nf, nr = wf.numel(), wr.numel()
    M = f64(np.log(float(nf) / float(nr)))
    n_eval = n_expand = n_iter = reads = 0
    nan = f64(np.nan)
    with torch.no_grad(), np.errstate(all="ignore"):
        one_sided = torch.stack([torch.logsumexp(-wf, 0), torch.logsumexp(-wr, 0)]).tolist()
        reads += 1
        upper = -(f64(one_sided[0]) - f64(np.log(float(nf))))
        lower = f64(one_sided[1]) - f64(np.log(float(nr)))

        def evaluate(delta):
            nonlocal n_eval, reads
            n_eval += 1
            reads += 1
            L = [f64(v) for v in _log_sums(wf, wr, float(delta), float(M)).tolist()]
            return L[0] - L[2], L

        f_upper, L = evaluate(upper)
        f_lower, L = evaluate(lower)
        while f_upper * f_lower > 0:
            if n_expand >= maximum_iterations:
                return nan, nan, nan, NO_ROOT, n_eval, n_expand, n_iter, reads
            average = (upper + lower) / 2
            upper = upper - _clamp(abs(upper - average))
            lower = lower + _clamp(abs(lower - average))
            n_expand += 1
            f_upper, L = evaluate(upper)
            f_lower, L = evaluate(lower)
        delta_old = f64(np.inf)
        while True:
            delta = upper - f_upper * (upper - lower) / (f_upper - f_lower)
            f_new, L = evaluate(delta)
            if f_upper * f_new < 0.0:
                lower, f_lower = delta, f_new
            elif f_lower * f_new <= 0:
                upper, f_upper = delta, f_new
            else:
                return nan, nan, nan, NOT_A_NUMBER, n_eval, n_expand, n_iter, reads
            n_iter += 1
            status = BUDGET if n_iter >= maximum_iterations else None
            if stop and (f_new == 0 or delta == delta_old or abs(delta - delta_old) <= relative_tolerance * abs(delta)):
                status = CONVERGED
            if status is not None:
                break
            delta_old = delta
        variance = _variance(L, nf, nr, exp=np.exp)
        return delta, np.sqrt(variance), f_new, status, n_eval, n_expand, n_iter, reads


def _bar_torch(forward_work, reverse_work, maximum_iterations, relative_tolerance, stop=True):
    dev = forward_work.device
    wf, wr = forward_work.double(), reverse_work.double()
    delta, unc, resid, status, n_eval, n_expand, n_iter, reads = _solve_torch(wf.detach(), wr.detach(), maximum_iterations,
                                                                                relative_tolerance, stop)
    delta_t, unc_t, resid_t = (torch.tensor(float(v), dtype=torch.float64, device=dev) for v in (delta, unc, resid))
    if torch.is_grad_enabled() and (wf.requires_grad or wr.requires_grad) and status in (CONVERGED, BUDGET):
        # the derivative of the root by the implicit-function theorem, d delta = -(df/dw) / (df/d delta): (f - f.detach()) is exactly
        # zero, so the value is the solver's; the uncertainty is re-evaluated at the differentiable delta
        nf, nr = wf.numel(), wr.numel()
        M = float(np.log(float(nf) / float(nr)))
        d = delta_t.clone().requires_grad_(True)
        L = _log_sums(wf, wr, d, M)
        f = L[0] - L[2]
        (slope,) = torch.autograd.grad(f, d, retain_graph=True)
        delta_t = delta_t - (f - f.detach()) / slope
        unc_t = _variance(_log_sums(wf, wr, delta_t, M), nf, nr).sqrt()
    return BARResult(delta_t, unc_t, resid_t, status, n_eval, n_expand, n_iter, reads)


def _blocks(n):
    return max(1, min(MAX_BLOCKS, (n + MIN_ELEMENTS_PER_BLOCK - 1) // MIN_ELEMENTS_PER_BLOCK))


def _bar_kernel(wf, wr, maximum_iterations, relative_tolerance, chunk=None):
    chunk = BAR_CHUNK if chunk is None else int(chunk)
    dev = wf.device
    wf, wr = wf.detach().contiguous(), wr.detach().contiguous()
    nbf, nbr = _blocks(wf.numel()), _blocks(wr.numel())
    partial = torch.empty(3 * (nbf + nbr), dtype=torch.float64, device=dev)

    def enqueue(record, n_steps):
        return _lib.lib().bgk_bar_solve_steps(_lib.ptr(wf), wf.numel(), _lib.ptr(wr), wr.numel(), _DTYPE_CODES[wf.dtype], nbf, nbr,
                                              _lib.ptr(partial), _lib.ptr(record), maximum_iterations, relative_tolerance, n_steps,
                                              _lib.stream_ptr(dev))

    # one pass for the bounds, two evaluations per expansion (and the first two), one per iteration
    budget = 3 + 2 * maximum_iterations + maximum_iterations
    record, host, reads = _driver.solve_record(enqueue, RECORD_DOUBLES, PHASE_DONE, budget, chunk, dev, "bgk_bar_solve_steps")
    return BARResult(record[R_RESULT].clone(), record[R_UNCERTAINTY].clone(), record[R_RESIDUAL].clone(), int(host[R_STATUS]),
                     int(host[R_N_EVAL]), int(host[R_N_EXPAND]), int(host[R_N_ITER]), reads)


def _kernel_eligible(wf, wr):
    grad = torch.is_grad_enabled()              # without it nothing is recorded, so inputs that require grad are taken too
    return all(_driver.kernel_takes(w, any_layout=True, requires_grad_ok=not grad) for w in (wf, wr)) and _driver.same_kind((wf, wr))


def bar_solve(forward_work, reverse_work, maximum_iterations=500, relative_tolerance=1e-12, path=None):
    """Solve the BAR equation; returns a ``BARResult``: f64 0-dim tensors ``delta_f``, ``uncertainty``, ``residual`` (f at the returned
    delta_f) on the inputs' device and host ints ``status`` (``CONVERGED``, ``BUDGET``, ``NO_ROOT``, ``NOT_A_NUMBER``; the last two
    return NaN), ``n_evaluations`` of f, ``n_expansions`` of the bracket, ``n_iterations`` of false position, ``n_readbacks``.

    ``path``: None picks the kernel for work values of one dtype in {f32, f64} on one HIP device that do not require grad (while grad
    is enabled), the torch ops otherwise; "kernel" / "torch" force one ("kernel" raises ValueError for inputs it does not take)."""
    if forward_work.device != reverse_work.device:
        raise ValueError(f"bar_solve: forward work on {forward_work.device}, reverse work on {reverse_work.device}")
    wf, wr = forward_work.reshape(-1), reverse_work.reshape(-1)
    if wf.numel() == 0 or wr.numel() == 0:
        raise ValueError("bar_solve: empty work array")
    maximum_iterations = int(maximum_iterations)
    if maximum_iterations <= 0:
        raise ValueError("bar_solve: maximum_iterations must be positive")
    if _driver.use_kernel(path, _kernel_eligible(wf, wr), "bar_solve",
                          "f32 or f64 work values of one dtype on one HIP device that do not require grad"):
        return _bar_kernel(wf, wr, maximum_iterations, float(relative_tolerance))
    return _bar_torch(wf, wr, maximum_iterations, float(relative_tolerance))


def _bennett_acceptance_ratio_pymbar(forward_work, reverse_work, compute_uncertainty=True, maximum_iterations=500,
                                     relative_tolerance=1e-12):
    """pymbar's BAR on host copies (:69-89)"""
    import io
    from contextlib import redirect_stdout

    import pymbar

    from .utils import as_numpy
    ctx = {"device": forward_work.device, "dtype": forward_work.dtype}
    out = io.StringIO()
    with redirect_stdout(out):
        result = pymbar.BAR(w_F=as_numpy(forward_work), w_R=as_numpy(reverse_work), return_dict=False,
                            compute_uncertainty=compute_uncertainty, maximum_iterations=maximum_iterations,
                            relative_tolerance=relative_tolerance)
    if "poor overlap" in out.getvalue() or (compute_uncertainty and np.isnan(result[1])):
        return torch.tensor(np.nan, **ctx), torch.tensor(np.nan, **ctx)
    if compute_uncertainty:
        return torch.tensor(result[0], **ctx), torch.tensor(result[1], **ctx)
    return torch.tensor(result, **ctx), None


def _bennett_acceptance_ratio_torch(forward_work, reverse_work, compute_uncertainty=True, maximum_iterations=500,
                                    relative_tolerance=1e-12):
    r = bar_solve(forward_work, reverse_work, maximum_iterations=maximum_iterations, relative_tolerance=relative_tolerance)
    dtype = forward_work.dtype if forward_work.dtype.is_floating_point else torch.get_default_dtype()
    if r.status in (NO_ROOT, NOT_A_NUMBER):         # the reference's NaN pair (:160), whatever compute_uncertainty says
        return r.delta_f.to(dtype), r.uncertainty.to(dtype)
    return r.delta_f.to(dtype), (r.uncertainty.to(dtype) if compute_uncertainty else None)


def bennett_acceptance_ratio(forward_work, reverse_work, compute_uncertainty=True, implementation="torch", maximum_iterations=500,
                             relative_tolerance=1e-12, warn=False):
    """Free energy difference DF_{0 -> 1} between two ensembles by the Bennett acceptance ratio (utils/free_energy.py:13-66).

    forward_work: u1(x) - u0(x) on samples x ~ e^-u0; reverse_work: u0(x) - u1(x) on samples x ~ e^-u1 (dimensionless, any shape).
    implementation: "torch" (this package's solver: ``bar_solve``) or "pymbar".  Returns ``(delta_f, uncertainty)``, 0-dim tensors of
    ``forward_work``'s dtype and device; ``uncertainty`` is None when not asked for.  Without a root (no overlap) both are NaN, and
    ``warn`` issues a UserWarning."""
    implementations = {"torch": _bennett_acceptance_ratio_torch, "pymbar": _bennett_acceptance_ratio_pymbar}
    delta_f, uncertainty = implementations[implementation](forward_work, reverse_work, compute_uncertainty=compute_uncertainty,
                                                           maximum_iterations=maximum_iterations,
                                                           relative_tolerance=relative_tolerance)
    if warn and bool(torch.isnan(delta_f)):
        warnings.warn("BAR could not compute free energy differences due to poor overlap. Returns nan.", UserWarning)
    return delta_f, uncertainty
