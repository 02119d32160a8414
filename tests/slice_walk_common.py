"""Shared by test_host_slice_walk.py and test_gpu_slice_walk.py: the shapes at which the slice walk of csrc/bgk_reduce.h (head, 16-byte
pieces, tail; BAR element by element, MBAR tile by tile) can drop or double-count a sample, seeded inputs for them, the references and
the bounds.  torch and numpy only.

Inputs: uniform in [0, 1) from a seeded CPU generator, drawn in f64 and rounded to the case's dtype, placed at an element offset inside
a padded buffer so that the first element takes every phase of 16 bytes (f32: 0 .. 3 elements, f64: 0, 1), a canary on both sides.

BAR, one step on a zeroed record (the BOUNDS phase): record[R_UPPER] = -(LSE(-wF) - log nF), record[R_LOWER] = LSE(-wR) - log nR against
``torch.logsumexp`` in f64 on the same values,

    |got - ref| <= 2 ((n + 8) 2^-52 + 2^-52 |ref|)                                                   (``bar_bound``)

(n + 8) 2^-52 is one rounding per add of terms e^(v - max) <= 1 plus the exp, the rescales and the log, relative to a sum >= 1;
2^-52 |ref| the roundings of max + log and of the log n; the factor 2 covers both sides, kernel and reference.
MBAR, one iteration from f = 0 over K = 5 windows (centres -1 .. 1, kappa = 1, counts n // 5 with the remainder in window 0): f against
``umbrella._mbar_torch`` with the same arguments on the CPU,

    max_k |f_k - ref_k| <= 2 (n + 2 K + 16) 2^-52                                                    (``mbar_bound``)

one rounding per add of the n terms W_nk <= 1 relative to S_k >= its largest term, 2 K for the two passes over the windows inside every
D_n, 16 for the exp, the two logs and the two subtractions; again both sides.

test_host_slice_walk.py asserts what makes these bounds mean something: the references alone, against long-double restatements, stay
within REFERENCE_SHARE of the one-sided bound, and leaving out one element moves the result by more than BAR_DROP / MBAR_DROP bounds.
Measured on the CPU for exactly these inputs: ``torch.logsumexp`` uses at most 0.049 of the one-sided bound and the least effect of a
dropped element is 7.8e7 bounds; ``_mbar_torch`` uses at most 0.054 (f64, n = 5: 1.7 x 2^-52 of a bound of 31 x 2^-52 -- at the small
sizes the share is a count of ulps of f; 0.002 from n = 1023 on), and a dropped first or last sample moves f by 1.3e13 bounds at n = 5,
about 1e9 at n = 1023 .. 1029, 1.2e8 at 2053 and 4.2e7 at 3077: the effect is W_nk / S_k <= K / n while the bound grows with n, so the
ratio falls as 1 / n^2 and 1e9 cannot hold at the two largest sizes; MBAR_DROP is set below the least of them."""
import functools

import numpy as np
import torch

from bgflow_amd import umbrella

BAR_NS = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 1027, 1028, 1029, 4101)
MBAR_NS = (5, 6, 7, 8, 9, 1023, 1024, 1025, 1027, 1028, 1029, 2053, 3077)
BLOCKS = (1, 2, 7)             # 7 blocks on 5 elements: slices of 4 and empty blocks; 3077 in one block: three tiles and a ragged fourth
OFFSETS = {torch.float32: (0, 1, 2, 3), torch.float64: (0, 1)}
DTYPES = (torch.float32, torch.float64)
K = 5
PAD = 8                        # canary elements on either side of the used range
CANARIES = (float("nan"), -30.0)      # read into a log-sum-exp of -w, or into an S_k, either one changes the result beyond any bound
EPS = 2.0 ** -52
REFERENCE_SHARE = 0.06
BAR_DROP, MBAR_DROP = 1e3, 1e7


def bar_bound(n, ref):
    return 2.0 * ((n + 8) * EPS + EPS * abs(ref))


def mbar_bound(n):
    return 2.0 * (n + 2 * K + 16) * EPS


@functools.lru_cache(maxsize=None)
def values(n, dtype, stream):
    """n values of ``dtype`` in [0, 1); ``stream`` 0 / 1 / 2: forward work, reverse work, MBAR samples"""
    g = torch.Generator().manual_seed(1000003 * stream + n)
    return torch.rand(n, generator=g, dtype=torch.float64).to(dtype)


def padded(v, offset, canary):
    """(buffer, view): ``v`` at element ``offset`` + PAD of a buffer that holds ``canary`` everywhere else"""
    buf = torch.full((v.numel() + 2 * PAD + offset,), canary, dtype=v.dtype)
    buf[PAD + offset:PAD + offset + v.numel()] = v
    return buf, buf[PAD + offset:PAD + offset + v.numel()]


# ---- BAR ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bar_reference(n, dtype, stream):
    """torch.logsumexp(-w) in f64"""
    return float(torch.logsumexp(-values(n, dtype, stream).double(), 0))


def bar_upper(n, dtype):
    return -(bar_reference(n, dtype, 0) - float(np.log(np.float64(n))))


def bar_lower(n, dtype):
    return bar_reference(n, dtype, 1) - float(np.log(np.float64(n)))


def lse_long_double(x):
    x = np.asarray(x, np.longdouble)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


# ---- MBAR --------------------------------------------------------------------------------------------------------------------------------
def mbar_counts(n):
    return [n // K + n % K] + [n // K] * (K - 1)


def mbar_table(n, device="cpu"):
    return umbrella._window_table(mbar_counts(n), np.linspace(-1.0, 1.0, K), np.ones(K), 1.0, device)


@functools.lru_cache(maxsize=None)
def mbar_reference(n, dtype):
    """f [K] after one iteration from f = 0: ``_mbar_torch`` on the CPU, stopped by its budget"""
    r = umbrella._mbar_torch(values(n, dtype, 2), mbar_table(n), 1, 0.0)
    assert r.status == umbrella.BUDGET and r.iterations == 1
    return r.f


def mbar_long_double(rc, table, skip=None):
    """the same iteration in numpy long double on the f64 table; ``skip``: the index of a sample that is left out of the sums"""
    r = np.asarray(rc, np.longdouble)
    if skip is not None:
        r = np.delete(r, skip)
    m, kappa, log_n = (np.asarray(table[:, i], np.longdouble) for i in range(3))
    a = log_n[None, :] - kappa[None, :] * (r[:, None] - m[None, :]) ** 2
    mx = a.max(1)
    D = mx + np.log(np.exp(a - mx[:, None]).sum(1))
    f = -(np.log(np.exp(a - D[:, None]).sum(0)) - log_n)
    return f - f[0]
