"""Streaming column statistics (count, mean, unbiased std, min, max) of tall [B, P] tensors: what
``InternalCoordinateMarginals.inform_with_data`` reduces the IC values of a data set to (factory/icmarginals.py:126-157 calls
``values.min() / .max() / .mean(axis=0) / .std(axis=0)``: four passes per field).

f32 HIP tensors go through bgk_column_moments_update (csrc/bgk_moments.hip): one pass, f64 shifted sums, deterministic.  CPU
tensors and other dtypes (the host tests, f64 builder contexts) run the same arithmetic as torch ops in f64.  The state between
chunks is one f64 tensor [P, 6] = {n, K, S1, S2, min, max} per column, so a data set larger than memory streams through."""
from collections import namedtuple

import torch

from . import _lib

__all__ = ["ColumnMoments", "ColumnMomentsResult"]

ColumnMomentsResult = namedtuple("ColumnMomentsResult", ["count", "mean", "std", "min", "max"])

MAX_BLOCKS = 1024         # row blocks of the kernel's first stage (4 per CU)
MIN_ROWS_PER_BLOCK = 64


class ColumnMoments:
    """Running per-column statistics of everything passed to ``update``.

    >>> m = ColumnMoments(17, device)
    >>> for chunk in chunks:        # [B_i, 17] each
    ...     m.update(chunk)
    >>> count, mean, std, lo, hi = m.result()       # f64 tensors [17] on the device
    """

    def __init__(self, n_columns, device=None):
        self.n_columns = int(n_columns)
        self.state = torch.zeros(self.n_columns, 6, dtype=torch.float64, device=device)
        self.n_rows = 0            # host-side count of the rows merged so far (the state's own n stays on the device)
        self._workspace = None

    def update(self, x):
        """merge the rows of ``x`` [B, P] (unit column stride) into the state: one kernel call, no host read"""
        if x.dim() != 2 or x.shape[1] != self.n_columns:
            raise ValueError(f"ColumnMoments.update: expected [B, {self.n_columns}], got {tuple(x.shape)}")
        if x.device != self.state.device:
            raise ValueError(f"ColumnMoments.update: tensor on {x.device}, state on {self.state.device}")
        x = x.detach()
        B, P = x.shape
        if x.is_cuda and x.dtype == torch.float32:
            if B > 0 and P > 0:
                x2, ldx = _lib.rowmajor(x)
                nblk = max(1, min(MAX_BLOCKS, (B + MIN_ROWS_PER_BLOCK - 1) // MIN_ROWS_PER_BLOCK))
                if self._workspace is None or self._workspace.numel() < nblk * P * 6:
                    self._workspace = torch.empty(nblk * P * 6, dtype=torch.float64, device=x.device)
                with torch.cuda.device(x.device):
                    st = _lib.lib().bgk_column_moments_update(_lib.ptr(x2), ldx, B, P, _lib.ptr(self._workspace), nblk,
                                                              _lib.ptr(self.state), _lib.stream_ptr(x.device))
                _lib.check(st, "bgk_column_moments_update")
        elif B > 0:
            self._update_torch(x.double())
        self.n_rows += B
        return self

    def _update_torch(self, x):
        """the kernel's arithmetic as torch ops: shifted sums under the state's K (row 0 of the first chunk)"""
        s = self.state
        first = self.n_rows == 0
        K = x[0].clone() if first else s[:, 1]
        d = x - K
        lo, hi = x.min(dim=0).values, x.max(dim=0).values          # (torch's min / max keep a NaN)
        s[:, 0] += x.shape[0]
        s[:, 2] += d.sum(dim=0)
        s[:, 3] += (d * d).sum(dim=0)
        if first:
            s[:, 1], s[:, 4], s[:, 5] = K, lo, hi
        else:
            s[:, 4] = torch.where((lo < s[:, 4]) | lo.isnan(), lo, s[:, 4])
            s[:, 5] = torch.where((hi > s[:, 5]) | hi.isnan(), hi, s[:, 5])

    def result(self):
        """(count, mean, std, min, max): f64 tensors [P] on the state's device; std with divisor n - 1 (NaN for one row)"""
        P = self.n_columns
        if self.state.is_cuda and P > 0:
            out = torch.empty(5, P, dtype=torch.float64, device=self.state.device)
            with torch.cuda.device(self.state.device):
                st = _lib.lib().bgk_column_moments_finalize(_lib.ptr(self.state), P, self.n_rows, _lib.ptr(out),
                                                            _lib.stream_ptr(self.state.device))
            _lib.check(st, "bgk_column_moments_finalize")
            return ColumnMomentsResult(*out.unbind(0))
        if self.n_rows == 0:
            raise RuntimeError("ColumnMoments.result: no rows were accumulated (n = 0): the statistics are undefined")
        n, K, S1, S2, lo, hi = self.state.unbind(1)
        shift = S1 / n
        var = (S2 - S1 * shift) / (n - 1.0)
        var = torch.where(var < 0, torch.zeros_like(var), var)
        return ColumnMomentsResult(n.clone(), K + shift, var.sqrt(), lo.clone(), hi.clone())
