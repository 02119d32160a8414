"""CPU: InternalCoordinateMarginals.inform_with_data / inform_with_force_field (reference factory/icmarginals.py:82-163) and the
streaming column statistics behind it (bgflow_amd.moments.ColumnMoments, torch form) against tests/golden/g_icmarginals.npz, which
tests/golden/make_icmarginal_goldens.py wrote by running the unmodified reference in f32 and in f64.

Bounds.  The statistics here are formed in f64 from the reference's own f32 internal coordinates and rounded once to f32; the
reference forms them in f32.  Against its f32 values the bound is 4 f32 ulp (the larger share of that is the reference's own
error); against its f64 values it is the reference's own f32-vs-f64 deviation recorded in the fixture (dev_*)."""
import inspect

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import BONDS, ANGLES, TORSIONS, FIXED, InternalCoordinateMarginals

FIELDS = (("bonds", BONDS), ("angles", ANGLES), ("torsions", TORSIONS))
CTX = {"device": None, "dtype": torch.float32}


class StubTransform:
    """a coordinate transform whose forward returns recorded internal coordinates (and the two outputs the method ignores)"""

    def __init__(self, G, dtype=torch.float32):
        self.values = [torch.tensor(G[f"ic_{name}"], dtype=dtype) for name, _ in FIELDS]
        self.calls = []

    def forward(self, data):
        assert not torch.is_grad_enabled(), "inform_with_data runs the transform under no_grad"
        self.calls.append(len(data))
        rows = data.long()                        # the stub's "data" are frame numbers
        return (*[v[rows] for v in self.values], torch.zeros(len(rows), 9), torch.zeros(len(rows), 1))


def dims(n_constrained=0, with_fixed=True):
    shapes = bg.ShapeDictionary()
    shapes[BONDS], shapes[ANGLES], shapes[TORSIONS] = (17 - n_constrained,), (17,), (17,)
    if with_fixed:
        shapes[FIXED] = (9,)
    return shapes


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def test_signature_is_the_references_plus_batch_size():
    p = list(inspect.signature(InternalCoordinateMarginals.inform_with_data).parameters.values())
    positional = [(q.name, q.default) for q in p if q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    empty = inspect.Parameter.empty
    assert positional == [("self", empty), ("data", empty), ("coordinate_transform", empty), ("bond_lower", 0.01), ("bond_upper", 1),
                          ("angle_lower", 0.01), ("angle_upper", 1.0), ("torsion_lower", 0.0), ("torsion_upper", 1.0),
                          ("constrained_bond_indices", None), ("bonds", BONDS), ("angles", ANGLES), ("torsions", None),
                          ("broadening", 1)]
    assert [(q.name, q.default, q.kind) for q in p[len(positional):]] == [("batch_size", None, inspect.Parameter.KEYWORD_ONLY)]
    q = list(inspect.signature(InternalCoordinateMarginals.inform_with_force_field).parameters.values())
    assert [(r.name, r.default) for r in q] == [("self", empty), ("system", empty), ("coordinate_transform", empty),
                                                ("temperature", empty), ("bonds", BONDS), ("angles", ANGLES), ("torsions", None)]


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("b", [0, 1])
@pytest.mark.parametrize("t", [0, 1])
def test_marginals_match_the_reference(golden, c, b, t):
    G = golden("g_icmarginals")
    constrained = [None, list(G["c_idx"])][c]
    broadening = [1, float(G["broadening"])][b]
    m = InternalCoordinateMarginals(dims(2 * c), CTX)
    fixed_before, torsions_before = m[FIXED], m[TORSIONS]
    kwargs = {"torsions": TORSIONS} if t else {}
    m.inform_with_data(torch.arange(256), StubTransform(G), constrained_bond_indices=constrained, broadening=broadening, **kwargs)
    assert m[FIXED] is fixed_before
    if not t:
        assert m[TORSIONS] is torsions_before and type(m[TORSIONS]).__name__ == "SloppyUniform"
    for name, field in FIELDS[:2 + t]:
        d = m[field]
        assert type(d) is bg.TruncatedNormalDistribution and d._mu.dtype == torch.float32
        assert d._mu.shape == (17 - 2 * c if name == "bonds" else 17,)
        for stat, got in (("mu", d._mu.numpy()), ("sigma", d._sigma.numpy())):
            ref32, ref64 = G[f"{stat}_{name}_c{c}_b{b}_t{t}_32"], G[f"{stat}_{name}_c{c}_b{b}_t{t}_64"]
            assert got.shape == ref32.shape
            e32 = np.abs(got.astype(np.float64) - ref32) / ulp32(ref32)
            dev = np.abs(ref32.astype(np.float64) - ref64).max()       # the reference's own deviation, this combination (dev_*: c1 b0 t1)
            e64 = np.abs(got.astype(np.float64) - ref64).max()
            print(f"{name} {stat} c{c} b{b} t{t}: {e32.max():.2f} ulp of the f32 reference; vs f64 {e64:.3e} (reference's own {dev:.3e})")
            assert e32.max() <= 4
            assert e64 <= dev
    lower = {"bonds": 0.01, "angles": 0.01, "torsions": 0.0}
    for name, field in FIELDS[:2 + t]:
        assert float(m[field].lower_bound) == np.float32(lower[name]) and float(m[field].upper_bound) == 1.0


def test_streaming_over_batches_and_absent_fields(golden):
    G = golden("g_icmarginals")
    one, many = InternalCoordinateMarginals(dims(), CTX), InternalCoordinateMarginals(dims(), CTX)
    one.inform_with_data(torch.arange(256), StubTransform(G), torsions=TORSIONS)
    stub = StubTransform(G)
    many.inform_with_data(torch.arange(256), stub, torsions=TORSIONS, batch_size=100)
    assert stub.calls == [100, 100, 56]
    for _, f in FIELDS:
        np.testing.assert_allclose(many[f]._mu.double().numpy(), one[f]._mu.double().numpy(), rtol=1e-7, atol=0)
        np.testing.assert_allclose(many[f]._sigma.double().numpy(), one[f]._sigma.double().numpy(), rtol=1e-7, atol=0)
    # a field that is not in current_dims is neither read nor written
    shapes = bg.ShapeDictionary()
    shapes[ANGLES] = (17,)
    m = InternalCoordinateMarginals(shapes, CTX)
    m.inform_with_data(torch.arange(256), StubTransform(G), bond_lower=0.5, torsions=TORSIONS, torsion_lower=0.5)   # bounds inside the data
    assert list(m) == [ANGLES] and type(m[ANGLES]) is bg.TruncatedNormalDistribution
    # an f64 context gets f64 marginals from f64 values
    m64 = InternalCoordinateMarginals(dims(), {"device": None, "dtype": torch.float64})
    m64.inform_with_data(torch.arange(256), StubTransform(G, torch.float64), torsions=TORSIONS)
    assert m64[BONDS]._mu.dtype == torch.float64
    np.testing.assert_allclose(m64[BONDS]._mu.numpy(), G["ic_bonds"].astype(np.float64).mean(0), rtol=1e-13)
    np.testing.assert_allclose(m64[TORSIONS]._sigma.numpy(), G["ic_torsions"].astype(np.float64).std(0, ddof=1), rtol=1e-12)


def test_range_asserts(golden):
    G = golden("g_icmarginals")
    lo = {n: float(G[f"ic_{n}"].min()) for n, _ in FIELDS}
    hi = {n: float(G[f"ic_{n}"].max()) for n, _ in FIELDS}
    mid = {n: 0.5 * (lo[n] + hi[n]) for n, _ in FIELDS}

    def run(**kw):
        InternalCoordinateMarginals(dims(), CTX).inform_with_data(torch.arange(256), StubTransform(G), torsions=TORSIONS, **kw)

    for kw, message in (({"bond_lower": mid["bonds"]}, "Set a smaller bond_lower"), ({"bond_upper": mid["bonds"]}, "Set a larger bond_upper"),
                        ({"angle_lower": mid["angles"]}, "Set a smaller angle_lower"), ({"angle_upper": mid["angles"]}, "Set a larger angle_upper"),
                        ({"torsion_lower": mid["torsions"]}, "Set a smaller torsion_lower"),
                        ({"torsion_upper": mid["torsions"]}, "Set a larger torsion_upper"),
                        ({"bond_lower": lo["bonds"]}, "Set a smaller bond_lower"), ({"bond_upper": hi["bonds"]}, "Set a larger bond_upper"),
                        ({"angle_lower": lo["angles"]}, "Set a smaller angle_lower"), ({"angle_upper": hi["angles"]}, "Set a larger angle_upper")):
        with pytest.raises(AssertionError) as err:
            run(**kw)
        assert str(err.value) == message, kw
    run(torsion_lower=lo["torsions"], torsion_upper=hi["torsions"])          # the torsion checks are not strict
    # the checks see every bond column: the extremes of a constrained column count (the reference asserts before it drops them)
    col = int(G["ic_bonds"].min(0).argmin())
    second = float(np.delete(G["ic_bonds"], col, axis=1).min())
    assert second > lo["bonds"]
    with pytest.raises(AssertionError, match="Set a smaller bond_lower"):
        InternalCoordinateMarginals(dims(1), CTX).inform_with_data(torch.arange(256), StubTransform(G), constrained_bond_indices=[col],
                                                                   bond_lower=0.5 * (lo["bonds"] + second))


def test_column_moments_on_cpu_tensors():
    g = torch.Generator().manual_seed(3)
    x = torch.stack([torch.rand(1000, generator=g), 0.1 + 0.003 * torch.randn(1000, generator=g),
                     1000 + 0.001 * torch.randn(1000, generator=g), torch.full((1000,), 0.3)], dim=1)
    one = bg.ColumnMoments(4).update(x).result()
    m = bg.ColumnMoments(4)
    for a, b in ((0, 300), (300, 300), (300, 1000)):         # (an empty chunk in between)
        m.update(x[a:b])
    many = m.result()
    x64 = x.double().numpy()
    assert one._fields == ("count", "mean", "std", "min", "max") and all(v.dtype == torch.float64 and v.shape == (4,) for v in one)
    for r in (one, many):
        assert r.count.tolist() == [1000.0] * 4
        np.testing.assert_allclose(r.mean.numpy(), x64.mean(0), rtol=1e-12, atol=0)
        np.testing.assert_allclose(r.std.numpy()[:3], x64.std(0, ddof=1)[:3], rtol=1e-9, atol=0)
        assert np.array_equal(r.min.numpy(), x64.min(0)) and np.array_equal(r.max.numpy(), x64.max(0))
        assert float(r.std[3]) == 0.0 and float(r.mean[3]) == float(np.float32(0.3))          # a constant column: exactly 0
    np.testing.assert_allclose(many.mean.numpy(), one.mean.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(many.std.numpy(), one.std.numpy(), rtol=1e-12, atol=0)
    # one row: NaN, as torch.std; a NaN stays in its column; f64 and non-contiguous inputs
    r1 = bg.ColumnMoments(2).update(torch.tensor([[1.0, 2.0]])).result()
    assert r1.std.isnan().all() and r1.mean.tolist() == [1.0, 2.0]
    xn = x.clone()
    xn[517, 1] = float("nan")
    rn = bg.ColumnMoments(4).update(xn[:400]).update(xn[400:]).result()
    assert rn.mean.isnan().tolist() == [False, True, False, False] and rn.std.isnan().tolist() == [False, True, False, False]
    assert rn.min.isnan().tolist() == [False, True, False, False]
    assert torch.equal(rn.mean[[0, 2, 3]], many.mean[[0, 2, 3]])
    rs = bg.ColumnMoments(2).update(x.double()[:, 1:3]).result()
    np.testing.assert_allclose(rs.std.numpy(), x64.std(0, ddof=1)[1:3], rtol=1e-9, atol=0)
    with pytest.raises(RuntimeError, match="no rows"):
        bg.ColumnMoments(3).result()
    with pytest.raises(ValueError):
        bg.ColumnMoments(3).update(torch.zeros(5, 4))


def test_inform_with_force_field_needs_bgmol(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "bgmol", None)           # "import bgmol" raises ImportError, installed or not
    with pytest.raises(ImportError):
        InternalCoordinateMarginals(dims(), CTX).inform_with_force_field(None, None, 300.0)
