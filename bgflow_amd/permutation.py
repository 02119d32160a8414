"""Permutation reduction: ``HungarianMapper`` (distribution/sampling/_mcmc/permutation.py) relabels the identical particles of every
sample so that each sits next to "its" position of a reference configuration -- the step that makes MCMC data of a solvent box usable
for a flow that is not permutation equivariant.

Kernel path (csrc/bgk_assign.hip, entry bgk_assign_particles): f32 tensors on a HIP device with at most 64 identical particles in at
most 3 dimensions and rows of at most 4096 values -- one launch per call, one wavefront per sample, no cost matrix in memory.
General path (everything else: numpy arrays, CPU tensors, f64, more particles or dimensions): the reference's method, an f64 cost matrix
per sample and ``scipy.optimize.linear_sum_assignment`` on the host.  The two agree wherever the assignment does not hinge on the
rounding of the f32 costs (DESIGN.md "Permutation reduction").
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib

__all__ = ["HungarianMapper"]

KERNEL_MAX_PARTICLES = 64
KERNEL_MAX_DIM = 3
KERNEL_MAX_ROW = 4096


class HungarianMapper:
    """Permutes identical particles to minimize the distance to a reference structure: for every configuration the permutation of the
    identical particles that minimizes the sum of squared distances to ``xref`` (a linear sum assignment per configuration).

    Parameters
    ----------
    xref : array or tensor
        reference structure, ``n * dim`` values ([x1, y1, x2, y2, ...] for ``dim=2``; any shape)
    dim : int
        number of dimensions of the particle system
    identical_particles : None or array of int
        indices of the particles subject to permutation, a set: used in ascending order (the reference sorts the coordinate indices it
        derives from them, which amounts to the same).  ``None``: all ``xref.size // dim`` particles.

    ``map`` / ``is_permuted`` are the reference's; ``assignment`` is new.  A numpy input gives numpy output, a tensor a tensor on its
    device and of its dtype; a single configuration ``[n * dim]`` is one sample, ``[B, n, dim]`` is accepted and returned in that shape.
    Outputs carry no autograd graph.

    Deviation from the reference: its ``identical_particles=None`` stands for ``np.arange(xref.size)`` -- coordinate, not particle,
    count -- and so indexes past the end of the coordinate vector; here it means every particle.  (The reference's module also imports
    ``deep_boltzmann`` and cannot be imported at all, so scipy's solution of the f64 problem is what this class is tested against.)

    Samples with a non-finite coordinate among their identical particles (or a non-finite reference) keep their order (identity
    permutation) on either path; ``map`` warns once with their count and never raises for them.
    """

    def __init__(self, xref, dim=2, identical_particles=None):
        if isinstance(dim, bool) or int(dim) != dim or dim < 1:
            raise ValueError(f"dim must be a positive integer, got {dim!r}")
        dim = int(dim)
        ref = xref.detach().cpu().numpy() if isinstance(xref, torch.Tensor) else np.asarray(xref)
        ref = np.array(ref, dtype=np.float64).reshape(-1)
        if ref.size == 0 or ref.size % dim:
            raise ValueError(f"xref has {ref.size} values: not a positive multiple of dim = {dim}")
        n = ref.size // dim
        if identical_particles is None:
            ip = np.arange(n, dtype=np.int64)
        else:
            raw = identical_particles.detach().cpu().numpy() if isinstance(identical_particles, torch.Tensor) else np.asarray(identical_particles)
            raw = raw.reshape(-1)
            if raw.size == 0:
                raise ValueError("identical_particles is empty")
            if raw.dtype.kind not in "iu":
                raise ValueError(f"identical_particles must be integer particle indices, got dtype {raw.dtype}")
            ip = np.sort(raw.astype(np.int64))
            if ip[0] < 0 or ip[-1] >= n:
                raise ValueError(f"identical_particles must lie in [0, {n}), got {int(ip[0])} .. {int(ip[-1])}")
            if np.any(ip[1:] == ip[:-1]):
                raise ValueError("identical_particles names a particle twice")
        self.xref = xref
        self.dim = dim
        self.n_particles = n
        self.identical_particles = ip
        self.ip_indices = (dim * ip[:, None] + np.arange(dim)[None, :]).reshape(-1)          # sorted coordinate indices
        self._ref64 = ref
        self._ref_ip = ref[self.ip_indices].reshape(len(ip), dim)
        self._ref_finite = bool(np.isfinite(self._ref_ip).all())
        self._host_index = (ctypes.c_int32 * len(ip))(*[int(q) for q in ip])
        self._device_ref = {}             # device -> xref as an f32 tensor there, uploaded once
        self._device_cols = {}            # device -> ip_indices as an int64 tensor there (general path on device tensors)

    # ---- shapes ---------------------------------------------------------------------------------------------------------------------
    def _as_rows(self, X):
        """X as [B, n dim] (the reference's ensure_traj) and the shape to hand results back in"""
        if not isinstance(X, (torch.Tensor, np.ndarray)):
            X = np.asarray(X)
        nd = self.n_particles * self.dim
        shape = tuple(X.shape)
        if X.ndim == 1 and shape[0] == nd:
            rows = X.reshape(1, nd)
        elif X.ndim == 2 and shape[1] == nd:
            rows = X
        elif X.ndim == 3 and shape[1:] == (self.n_particles, self.dim):
            rows = X.reshape(shape[0], nd)
        else:
            raise ValueError(f"expected [{nd}], [B, {nd}] or [B, {self.n_particles}, {self.dim}], got {list(shape)}")
        if not (X.dtype.is_floating_point if isinstance(X, torch.Tensor) else X.dtype.kind == "f"):
            raise ValueError(f"expected floating-point coordinates, got {X.dtype}")
        return rows, shape

    def _takes_kernel(self, rows):
        return (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32
                and len(self.identical_particles) <= KERNEL_MAX_PARTICLES and self.dim <= KERNEL_MAX_DIM
                and self.n_particles * self.dim <= KERNEL_MAX_ROW)

    # ---- kernel path ----------------------------------------------------------------------------------------------------------------
    def _launch(self, rows, y=False, perm=False, cost=False, status=False, permuted=False):
        """one launch of bgk_assign_particles on the rows' device and current stream; returns the outputs asked for (None otherwise)"""
        dev = rows.device
        rows, ldx = _lib.rowmajor(rows.detach())
        B, nd, m = rows.shape[0], rows.shape[1], len(self.identical_particles)
        ref = self._device_ref.get(dev)
        if ref is None:
            ref = self._device_ref[dev] = torch.tensor(self._ref64, dtype=torch.float32, device=dev)
        out_y = torch.empty((B, nd), dtype=torch.float32, device=dev) if y else None
        out_perm = torch.empty((B, m), dtype=torch.int32, device=dev) if perm else None
        out_cost = torch.empty((B,), dtype=torch.float32, device=dev) if cost else None
        out_status = torch.empty((B,), dtype=torch.int32, device=dev) if status else None
        out_permuted = torch.empty((B,), dtype=torch.int32, device=dev) if permuted else None
        if B:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().bgk_assign_particles(
                    _lib.ptr(rows), ldx, B, self.n_particles, self.dim, _lib.ptr(ref), self._host_index, m,
                    _lib.ptr(out_y), nd, _lib.ptr(out_perm), _lib.ptr(out_cost), _lib.ptr(out_status), _lib.ptr(out_permuted),
                    _lib.stream_ptr(dev)), "bgk_assign_particles")
        return out_y, out_perm, out_cost, out_status, out_permuted

    # ---- general path ---------------------------------------------------------------------------------------------------------------
    def _solve_host(self, rows):
        """(perm [B, m] int64, cost [B] f64, bad [B] bool) of numpy rows by scipy on the f64 cost matrix of every sample"""
        from scipy.optimize import linear_sum_assignment
        B, m = rows.shape[0], len(self.identical_particles)
        pts = np.asarray(rows[:, self.ip_indices], dtype=np.float64).reshape(B, m, self.dim)
        perm = np.tile(np.arange(m, dtype=np.int64), (B, 1))
        cost = np.empty(B, dtype=np.float64)
        bad = ~np.isfinite(pts).all(axis=(1, 2)) if self._ref_finite else np.ones(B, dtype=bool)
        for b in range(B):
            C = ((self._ref_ip[:, None, :] - pts[b][None, :, :]) ** 2).sum(-1)
            if bad[b]:
                cost[b] = np.trace(C)
                continue
            r, c = linear_sum_assignment(C)
            perm[b, r] = c
            cost[b] = C[r, c].sum()
        return perm, cost, bad

    def _host_rows(self, rows):
        return rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows

    def _warn(self, n_bad, B):
        if n_bad:
            warnings.warn(f"HungarianMapper.map: {n_bad} of {B} configurations have non-finite coordinates among their identical "
                          "particles (or the reference has); they keep their order", stacklevel=3)

    # ---- public ---------------------------------------------------------------------------------------------------------------------
    def map(self, X):
        """Maps X (configuration or trajectory) to the reference structure by permuting identical particles."""
        rows, shape = self._as_rows(X)
        B = rows.shape[0]
        if self._takes_kernel(rows):
            y, _, _, status, _ = self._launch(rows, y=True, status=True)
            self._warn(int(status.sum()) if B else 0, B)
            return y.reshape(shape)
        perm, _, bad = self._solve_host(self._host_rows(rows))
        self._warn(int(bad.sum()), B)
        m = len(self.identical_particles)
        src = self.ip_indices.reshape(m, self.dim)[perm].reshape(B, m * self.dim)     # [B, m dim]: the column each slot is filled from
        if isinstance(rows, torch.Tensor):
            rows = rows.detach()
            cols = self._device_cols.get(rows.device)
            if cols is None:
                cols = self._device_cols[rows.device] = torch.as_tensor(self.ip_indices, device=rows.device)
            Y = rows.clone()
            Y[:, cols] = torch.gather(rows, 1, torch.as_tensor(src, device=rows.device))
        else:
            Y = rows.copy()
            Y[:, self.ip_indices] = np.take_along_axis(rows, src, axis=1)
        return Y.reshape(shape)

    def is_permuted(self, X):
        """Returns True for permuted configurations (one bool per configuration)."""
        rows, _ = self._as_rows(X)
        if self._takes_kernel(rows):
            return self._launch(rows, permuted=True)[4].bool()
        perm, _, _ = self._solve_host(self._host_rows(rows))
        moved = (perm != np.arange(perm.shape[1])[None, :]).any(axis=1)
        return torch.as_tensor(moved, device=rows.device) if isinstance(rows, torch.Tensor) else moved

    def assignment(self, X):
        """``(perm [B, m] int64, cost [B])``: sample particle ``identical_particles[perm[b, i]]`` belongs to reference particle
        ``identical_particles[i]``; ``cost`` is the assignment's sum of squared distances (in X's dtype)."""
        rows, _ = self._as_rows(X)
        if self._takes_kernel(rows):
            _, perm, cost, _, _ = self._launch(rows, perm=True, cost=True)
            return perm.long(), cost
        perm, cost, _ = self._solve_host(self._host_rows(rows))
        if isinstance(rows, torch.Tensor):
            return torch.as_tensor(perm, device=rows.device), torch.as_tensor(cost, device=rows.device).to(rows.dtype)
        return perm, cost.astype(rows.dtype)
