"""What the host sides of the free-energy and statistics kernels share (free_energy.py, umbrella.py, analysis.py; csrc/bgk_reduce.h;
DESIGN.md "Shared plumbing of the free-energy kernels")."""
import contextlib

import torch

from . import _lib

DTYPE_CODES = {torch.float32: 0, torch.float64: 1}      # BGK_BAR_F32 / _F64, BGK_MBAR_*, BGK_HIST_* (include/bgflow_amd.h)
# a solver's status: BUDGET = iterations exhausted (the last iterate is returned), NO_ROOT = bracket expansions exhausted (BAR only),
# NOT_A_NUMBER = the residual or the error is NaN
CONVERGED, BUDGET, NO_ROOT, NOT_A_NUMBER = 0, 1, 2, 3
STATUS_NAMES = ("converged", "budget exhausted", "no root", "nan")
R_PHASE, R_STATUS = 0, 1       # the two record slots every solver shares


def kernel_takes(t, any_layout=False, requires_grad_ok=False):
    """the per-tensor rule of every kernel path: an f32 / f64 tensor on a HIP device that does not require grad, contiguous and 1-d
    unless ``any_layout`` (the caller flattens and copies)"""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in DTYPE_CODES and (requires_grad_ok or not t.requires_grad)
            and (any_layout or (t.dim() == 1 and t.is_contiguous())))


def same_kind(tensors):
    return all(t.dtype == tensors[0].dtype and t.device == tensors[0].device for t in tensors)


def use_kernel(path, eligible, who, takes):
    """``path``: None picks the kernel for inputs it takes (``eligible``), "kernel" / "torch" force one; True for the kernel"""
    if path not in (None, "kernel", "torch"):
        raise ValueError(f"{who}: unknown path {path!r}")
    if path == "kernel" and not eligible:
        raise ValueError(f"{who}: the kernel path takes {takes}")
    return path == "kernel" or (path is None and eligible)


def solve_record(enqueue, record_doubles, phase_done, budget, chunk, device, who, unit="steps"):
    """Drive a two-stage solver through its record: ``record_doubles`` zeros on ``device`` (the start state), then
    ``enqueue(record, chunk)`` -- ``chunk`` steps in stream order, returns the entry's status; steps past the end are empty launches --
    and one read-back, until the phase is ``phase_done``.  Returns (record, its host copy, read-backs); RuntimeError if the record is
    not done ``chunk`` steps past ``budget``, the most steps the solver can need."""
    record = torch.zeros(record_doubles, dtype=torch.float64, device=device)
    reads = enqueued = 0
    while True:
        with torch.cuda.device(device) if record.is_cuda else contextlib.nullcontext():
            _lib.check(enqueue(record, chunk), who)
        enqueued += chunk
        host = record.cpu()
        reads += 1
        if int(host[R_PHASE]) == phase_done:
            return record, host, reads
        if enqueued > budget + chunk:
            raise RuntimeError(f"{who}: the record is not done after {enqueued} {unit} (budget {budget})")
