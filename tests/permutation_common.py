"""Shared by test_host_permutation.py and test_gpu_permutation.py: the cases of tests/golden/permutation.npz (written by
tests/golden/make_permutation_goldens.py), and what "the same assignment" means.

The stable-row rule: a row is stable when scipy's solution on the f32-computed cost matrix equals the one on the f64 matrix (recorded by
the generator).  On stable rows a permutation must EQUAL the recorded one; on the others it must be a permutation (and the status 0).  At
most 0.5 % of a case's rows may be unstable -- checked by the generator for the fixture and by ``solve_rows`` for inputs drawn in a test."""
import json

import numpy as np
from scipy.optimize import linear_sum_assignment

import bgflow_amd as bg

MAX_UNSTABLE = 0.005


def case_list(G):
    return json.loads(str(G["cases"]))


def case(G, name):
    """(mapper, X [B, n d] f32, expected perm [B, m] int64, stable [B], the case's record)"""
    meta = {c["name"]: c for c in case_list(G)}[name]
    ip = G[name + "_ip"]
    mapper = bg.HungarianMapper(G[name + "_xref"], dim=meta["d"], identical_particles=ip)
    return mapper, G[name + "_X"], G[name + "_perm"].astype(np.int64), G[name + "_stable"], meta


def gathered(mapper, X, perm):
    """X with slot i of the identical set filled from sample particle perm[b, i] (numpy; moves bits only)"""
    m, d = len(mapper.identical_particles), mapper.dim
    cols = mapper.ip_indices.reshape(m, d)
    Y = X.copy()
    Y[:, mapper.ip_indices] = np.take_along_axis(X, cols[perm].reshape(X.shape[0], -1), axis=1)
    return Y


def cost64(mapper, X, perm):
    """f64 cost of ``perm`` on the f64 values of the (f32) inputs"""
    m, d = len(mapper.identical_particles), mapper.dim
    ref = np.asarray(mapper._ref_ip, dtype=np.float64)
    pts = X[:, mapper.ip_indices].astype(np.float64).reshape(X.shape[0], m, d)
    moved = np.take_along_axis(pts, perm[:, :, None], axis=1)
    return ((ref[None] - moved) ** 2).sum(axis=(1, 2))


def cost32_matrix(ref, pts):
    s = None
    for k in range(ref.shape[1]):
        t = (ref[:, None, k] - pts[None, :, k]).astype(np.float32)
        s = (t * t).astype(np.float32) if s is None else (s + (t * t).astype(np.float32)).astype(np.float32)
    return s


def solve_rows(mapper, X):
    """(perm [B, m], stable [B], optimal f64 cost [B]) of f32 rows X by scipy, as the generator does it; fails on too many unstable rows"""
    m, d = len(mapper.identical_particles), mapper.dim
    ref = np.asarray(mapper._ref_ip, dtype=np.float32)
    perm, stable, best = np.empty((X.shape[0], m), dtype=np.int64), np.empty(X.shape[0], dtype=bool), np.empty(X.shape[0])
    for b in range(X.shape[0]):
        pts = X[b, mapper.ip_indices].reshape(m, d)
        C = ((ref.astype(np.float64)[:, None] - pts.astype(np.float64)[None]) ** 2).sum(-1)
        r, c = linear_sum_assignment(C)
        perm[b], best[b] = c, C[r, c].sum()
        stable[b] = np.array_equal(c, linear_sum_assignment(cost32_matrix(ref, pts).astype(np.float64))[1])
    assert (~stable).sum() <= MAX_UNSTABLE * X.shape[0], f"{int((~stable).sum())} of {X.shape[0]} rows are unstable"
    return perm, stable, best


def check_perm(got, want, stable, label=""):
    """the stable-row rule"""
    got = np.asarray(got)
    m = got.shape[1]
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(m), (got.shape[0], 1))), f"{label}: not a permutation"
    wrong = np.flatnonzero((got != want).any(axis=1) & stable)
    assert wrong.size == 0, f"{label}: rows {wrong[:8].tolist()} of {got.shape[0]} differ from the recorded permutation"
