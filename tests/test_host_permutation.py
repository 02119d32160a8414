"""No GPU: bgflow_amd.HungarianMapper on its general path (scipy on the f64 cost matrix) against tests/golden/permutation.npz, the
class's interface and import paths, and what csrc/bgk_assign.hip shows without a device: its prototype in the header, in
``abi_signatures`` and in the built library, with the argument checks.  The stable-row rule: permutation_common.py."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols

from permutation_common import case, case_list, check_perm, gathered

M_VALUES, D_VALUES, B_VALUES = {1, 2, 3, 31, 32, 33, 63, 64}, {1, 2, 3}, {1, 3, 257}
i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
WANT = [p, i64, i64, i32, i32, p, p, i32, p, i64, p, p, p, p, p]


def names(golden):
    return [c["name"] for c in case_list(golden("permutation"))]


def test_the_fixture_covers_the_cases(golden):
    G = golden("permutation")
    cases = case_list(G)
    assert {c["m"] for c in cases} >= M_VALUES and {c["d"] for c in cases} == D_VALUES and {c["B"] for c in cases} == B_VALUES
    assert {(c["m"], c["d"]) for c in cases} >= {(m, d) for m in M_VALUES for d in D_VALUES}
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permutation.npz")) < 200_000
    for c in cases:
        ip, perm, stable = G[c["name"] + "_ip"], G[c["name"] + "_perm"], G[c["name"] + "_stable"]
        assert c["n"] > c["m"] == len(ip) and np.all(np.diff(ip) > 0) and ip[-1] < c["n"]          # a strict subset
        assert G[c["name"] + "_X"].dtype == np.float32 and G[c["name"] + "_X"].shape == (c["B"], c["n"] * c["d"])
        assert (~stable).sum() <= 0.005 * c["B"]
        identity = (perm == np.arange(c["m"])).all(axis=1)
        if c["B"] == 257:
            assert identity[7::8].all() and 0.1 < identity.mean() < 0.5
            moved = (perm != np.arange(c["m"])).sum(axis=1)
            assert c["m"] < 4 or np.median(moved[2::3][~identity[2::3]]) >= c["m"] // 2            # the large-noise rows are scrambled
    assert any(np.any(np.diff(G[c["name"] + "_ip"]) > 1) for c in cases)                           # a set with gaps


@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_general_path_meets_the_fixture(golden, kind):
    G = golden("permutation")
    for name in names(golden):
        mapper, X, want, stable, meta = case(G, name)
        arg = X if kind == "numpy" else torch.from_numpy(X)
        perm, cost = mapper.assignment(arg)
        Y, moved = mapper.map(arg), mapper.is_permuted(arg)
        assert type(perm) is type(arg) and type(cost) is type(arg) and type(Y) is type(arg) and type(moved) is type(arg)
        assert perm.dtype == (np.int64 if kind == "numpy" else torch.int64) and cost.dtype == arg.dtype and Y.dtype == arg.dtype
        perm, cost, Y, moved = (np.asarray(v) for v in (perm, cost, Y, moved))
        assert perm.shape == want.shape and cost.shape == (meta["B"],) and Y.shape == X.shape and moved.shape == (meta["B"],)
        check_perm(perm, want, stable, f"{name} {kind}")
        assert moved.dtype == np.bool_ and np.array_equal(moved, (perm != np.arange(meta["m"])).any(axis=1))
        assert np.array_equal(moved[stable], (want != np.arange(meta["m"])).any(axis=1)[stable])   # False exactly on identity rows
        assert Y.tobytes() == gathered(mapper, X, perm).tobytes()                                  # moves bits, other columns untouched
        rest = np.setdiff1d(np.arange(X.shape[1]), mapper.ip_indices)
        assert rest.size and Y[:, rest].tobytes() == X[:, rest].tobytes()
        again = np.asarray(mapper.map(Y if kind == "numpy" else torch.from_numpy(Y)))
        assert again.tobytes() == Y.tobytes(), f"{name}: map is not idempotent"
        assert not np.asarray(mapper.is_permuted(Y)).any()


def test_shapes(golden):
    mapper, X, want, stable, meta = case(golden("permutation"), "m36_d2_b3")
    n, d = meta["n"], meta["d"]
    Y = mapper.map(X)
    one = mapper.map(X[1])                                   # a single configuration is one sample
    assert one.shape == (n * d,) and np.array_equal(one, Y[1])
    assert mapper.is_permuted(X[1]).shape == (1,) and mapper.assignment(X[1])[0].shape == (1, meta["m"])
    cube = mapper.map(X.reshape(3, n, d))
    assert cube.shape == (3, n, d) and np.array_equal(cube.reshape(3, -1), Y)
    t = mapper.map(torch.from_numpy(X).reshape(3, n, d).double())
    assert t.shape == (3, n, d) and t.dtype == torch.float64 and np.array_equal(t.numpy().reshape(3, -1), Y.astype(np.float64))
    wide = np.zeros((3, n * d + 5), dtype=np.float32)
    wide[:, 3:3 + n * d] = X
    assert np.array_equal(mapper.map(wide[:, 3:3 + n * d]), Y)                                     # a strided view
    for bad in (X[:, :-1], X.reshape(3, d, n), X[0, :5], X.reshape(1, 3, -1).repeat(2, axis=0).reshape(2, 3, n, d)):
        with pytest.raises(ValueError):
            mapper.map(bad)
    with pytest.raises(ValueError):
        mapper.map(np.zeros((2, n * d), dtype=np.int64))
    empty = mapper.map(X[:0])
    assert empty.shape == (0, n * d) and mapper.is_permuted(X[:0]).shape == (0,) and mapper.assignment(X[:0])[0].shape == (0, meta["m"])


def test_a_nan_row_keeps_its_order_and_warns_once(golden):
    mapper, X, want, stable, meta = case(golden("permutation"), "m31_d1_b257")
    X = X[:12].copy()
    X[3, mapper.ip_indices[4]] = np.nan
    X[8, mapper.ip_indices[0]] = np.inf
    X[5, 0] = np.nan                                         # not an identical particle's coordinate: an ordinary row
    for arg in (X, torch.from_numpy(X)):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            Y = np.asarray(mapper.map(arg))
        assert len(caught) == 1 and "2 of 12" in str(caught[0].message) and "non-finite" in str(caught[0].message)
        assert Y[[3, 8]].tobytes() == X[[3, 8]].tobytes()
        perm = np.asarray(mapper.assignment(arg)[0])
        assert np.array_equal(perm[[3, 8]], np.tile(np.arange(meta["m"]), (2, 1)))
        keep = np.setdiff1d(np.arange(12), [3, 8])
        check_perm(perm[keep], want[:12][keep], stable[:12][keep], "neighbours of the NaN rows")
        assert not np.asarray(mapper.is_permuted(arg))[[3, 8]].any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mapper.map(X[[0, 1, 2, 5]])                          # no warning without such rows
    ref = golden("permutation")["m31_d1_b257_xref"].copy()
    ref[mapper.ip_indices[2]] = np.nan
    broken = bg.HungarianMapper(ref, dim=1, identical_particles=mapper.identical_particles)
    with pytest.warns(UserWarning, match="4 of 4"):
        assert broken.map(X[:4]).tobytes() == X[:4].tobytes()


def test_identical_particles_none_means_every_particle():
    rng = np.random.default_rng(3)
    xref = rng.uniform(-3, 3, 14)
    mapper = bg.HungarianMapper(xref, dim=2)
    assert np.array_equal(mapper.identical_particles, np.arange(7)) and np.array_equal(mapper.ip_indices, np.arange(14))
    order = rng.permutation(7)
    X = xref.reshape(7, 2)[order].reshape(1, 14) + 1e-3 * rng.standard_normal((1, 14))
    perm, cost = mapper.assignment(X)
    assert np.array_equal(order[perm[0]], np.arange(7)) and 0 < cost[0] < 1e-3 and cost.dtype == np.float64
    assert np.abs(mapper.map(X)[0] - xref).max() < 1e-2 and mapper.is_permuted(X)[0]
    unsorted = bg.HungarianMapper(xref, dim=2, identical_particles=[5, 1, 3])                      # a set: used in ascending order
    assert np.array_equal(unsorted.identical_particles, [1, 3, 5]) and np.array_equal(unsorted.ip_indices, [2, 3, 6, 7, 10, 11])
    assert bg.HungarianMapper(torch.tensor(xref), dim=2, identical_particles=torch.tensor([1, 3])).map(X).shape == (1, 14)


def test_import_paths():
    import bgflow_amd.distribution.sampling._mcmc as package
    import bgflow_amd.distribution.sampling._mcmc.permutation as module
    from bgflow_amd.distribution.sampling._mcmc.permutation import HungarianMapper
    assert HungarianMapper is bg.HungarianMapper is package.HungarianMapper is module.HungarianMapper is bg.permutation.HungarianMapper
    assert sys.modules["bgflow_amd.distribution.sampling._mcmc.permutation"] is module and package.permutation is module
    assert bg.distribution.sampling._mcmc is package


def test_constructor_errors():
    xref = np.zeros(12)
    for kwargs in (dict(dim=0), dict(dim=-2), dict(dim=1.5), dict(dim=5), dict(identical_particles=[]), dict(identical_particles=[0, 6]),
                   dict(identical_particles=[-1, 2]), dict(identical_particles=[1, 1, 2]), dict(identical_particles=[0.5, 1.0])):
        with pytest.raises(ValueError):
            bg.HungarianMapper(xref, **{"dim": 2, **kwargs})
    with pytest.raises(ValueError):
        bg.HungarianMapper(np.zeros(0), dim=2)
    assert bg.HungarianMapper(xref, dim=np.int64(3)).n_particles == 4


def test_more_particles_or_dimensions_than_the_kernel_takes():
    rng = np.random.default_rng(4)
    for n, d in ((70, 2), (5, 4)):
        xref = rng.uniform(-4, 4, (n, d))
        mapper = bg.HungarianMapper(xref, dim=d)
        order = rng.permutation(n)
        X = torch.tensor((xref[order] + 1e-4 * rng.standard_normal((n, d))).reshape(1, -1), dtype=torch.float32)
        assert not mapper._takes_kernel(X)
        assert np.array_equal(order[mapper.assignment(X)[0][0].numpy()], np.arange(n))


def test_the_prototype_is_declared_parsed_and_exported(hip_lib):
    assert abi_signatures()["bgk_assign_particles"] == (ctypes.c_int, WANT)
    assert "bgk_assign_particles" in abi_symbols()
    assert list(hip_lib.bgk_assign_particles.argtypes) == WANT
    assert ctypes.cast(ctypes.CDLL(_lib.LIB_PATH).bgk_assign_particles, ctypes.c_void_p).value, "bgk_assign_particles is not exported"


def test_argument_checks_of_the_entry(hip_lib):
    fake = ctypes.c_void_p(64)              # never dereferenced: every check comes before the first launch, and B = 0 launches nothing

    def call(x=fake, ldx=76, B=0, n=38, d=2, xref=fake, ident=tuple(range(2, 38)), m=None, y=fake, ldy=76, perm=fake, cost=fake,
             status=fake, permuted=fake):
        host = (ctypes.c_int32 * max(len(ident), 1))(*ident) if ident is not None else None
        return hip_lib.bgk_assign_particles(x, ldx, B, n, d, xref, host, len(ident) if m is None else m, y, ldy, perm, cost, status,
                                            permuted, None)

    assert call() == 0
    assert call(y=None, perm=None, cost=None, status=None, permuted=None, ldy=0) == 0               # every output is optional
    for bad in (dict(x=None), dict(xref=None), dict(ident=None, m=3)):
        assert call(**bad) == -1 and b"null pointer" in hip_lib.bgk_last_error()
    assert call(B=-1) == -1 and b"batch" in hip_lib.bgk_last_error()
    assert call(m=0) == -1 and call(ident=tuple(range(65)), n=70, ldx=140, ldy=140) == -1 and b"identical particles" in hip_lib.bgk_last_error()
    assert call(ident=tuple(range(64)), n=70, ldx=140, ldy=140) == 0
    assert call(d=0) == -1 and call(d=4, ldx=152, ldy=152) == -1 and b"dimensions" in hip_lib.bgk_last_error()
    assert call(d=3, ldx=114, ldy=114) == 0 and call(d=1, ident=(0,), n=4096, ldx=4096, ldy=4096) == 0
    assert call(d=1, ident=(0,), n=4097, ldx=4097, ldy=4097) == -1 and call(n=35) == -1 and b"particles" in hip_lib.bgk_last_error()
    for ident in ((2, 2, 3), (3, 2), (0, 38), (-1, 4)):
        assert call(ident=ident) == -1 and b"strictly increasing" in hip_lib.bgk_last_error()
    assert call(ldx=75) == -1 and call(ldy=75) == -1 and b"stride" in hip_lib.bgk_last_error() and call(ldy=75, y=None) == 0
    assert call(x=ctypes.c_void_p(66)) == -1 and call(status=ctypes.c_void_p(65)) == -1 and b"aligned" in hip_lib.bgk_last_error()
    assert call(x=ctypes.c_void_p(68)) == 0                                                          # 4 bytes are enough
