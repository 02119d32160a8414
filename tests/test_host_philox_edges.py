"""Host: the word -> uniform map of the Philox draws (``u01`` of csrc/bgk_philox.h, restated in oracle/philox.py) at the ends of the unit
interval, and the fixture of rows at which a kernel's draw lands there (tests/golden/philox_edges.npz, philox_edges_common.py).

u = min(((x >> 8) + 0.5) 2^-24, 1 - 2^-24) in f32.  The sum needs 25 significand bits, so it is exact only for x >> 8 < 2^23 and rounds to
even above; unclamped, the 256 largest words give exactly 1.0 -- a uniform draw outside [low, high), and a refused replica exchange at
equal temperatures.  The GPU counterpart is test_gpu_philox_edges.py."""
import numpy as np
import pytest

from oracle import philox

import philox_edges_common as C


@pytest.fixture(scope="module")
def all_u():
    """u01 of every value of x >> 8 (the low byte does not enter), computed once"""
    k = np.arange(2 ** 24, dtype=np.uint32)
    return k, philox.u01(k << np.uint32(8))


def test_u01_over_all_words_range_order_and_error(all_u):
    k, u = all_u
    assert u.dtype == np.float32
    assert u.min() == C.U_MIN == u[0] and u.max() == C.U_MAX == u[-1] and C.U_MAX < 1.0
    assert (np.diff(u) >= 0).all()
    exact = (k.astype(np.float64) + 0.5) * 2.0 ** -24
    err = u.astype(np.float64) - exact
    assert np.abs(err).max() <= 2.0 ** -25
    assert (err[: 2 ** 23] == 0).all()                        # the lower half is exact
    # the mean error.  Every term is a multiple of 2^-25, so the f64 sums are exact.  Round-to-even alone is unbiased: the errors sum
    # to 0 with the last value at 1.0, 2^-25 above its exact value; the clamp puts that one 2^-25 below instead: a mean of -2^-48
    assert err[:-1].sum() + 2.0 ** -25 == 0.0 and err[-1] == -2.0 ** -25 and err.mean() == -2.0 ** -48
    # the low byte does not enter
    assert np.array_equal(philox.u01((k[::4099] << np.uint32(8)) | np.uint32(255)), u[::4099])


def test_the_clamp_changes_the_256_largest_words_only(all_u):
    k, u = all_u
    raw = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    changed = np.nonzero(raw != u)[0]
    assert changed.tolist() == [2 ** 24 - 1] and raw[-1] == 1.0
    # distinct values: all 2^23 below 1/2, above it ties to even merge two of every four, and the last value stands alone -- at
    # 1 - 2^-24 as it did at 1.0: the clamp merges nothing
    assert len(np.unique(u)) == len(np.unique(raw)) == 2 ** 23 + 2 ** 22 + 1 and u[-2] < u[-1]


def test_fixture_entries_reproduce():
    es = C.entries()
    assert 12 <= len(es) <= 64
    for e in es:
        w = C.words_of(e)
        assert w[e.word] == e.x, e
        assert (e.x >= C.TOP_FROM) if e.top else (e.x < C.BOTTOM_BELOW), e
        assert e.row - max(C.LANES) >= 0
    for layout in ("field0", "field1"):
        for parity in (0, 1):
            assert len(C.select(layout, True, parity)) >= 2 and len(C.select(layout, False, parity)) >= 1
    for layout in ("accept", "exchange"):
        assert len(C.select(layout, True)) >= 2 and len(C.select(layout, False)) >= 1
        assert all(e.word == 0 for e in C.select(layout, True) + C.select(layout, False))
    assert all(e.row % 2 == 0 for e in C.entries() if e.layout == "exchange")       # the lower slot of a ladder of two


@pytest.mark.parametrize("layout,field", [("field0", 0), ("field1", 1)])
def test_uniform_draw_at_a_top_word_is_below_one(layout, field):
    for e in C.select(layout, True):
        u = philox.sample_field(e.seed, e.offset, field, 1, 4, 0, row0=e.row)
        assert u.shape == (1, 4) and u.dtype == np.float32
        assert (u < 1.0).all() and (u > 0.0).all(), (e, u)
        assert u[0, e.word] == C.U_MAX
    for e in C.select(layout, False):
        u = philox.sample_field(e.seed, e.offset, field, 1, 4, 0, row0=e.row)
        assert u[0, e.word] == C.U_MIN and (u > 0.0).all()


@pytest.mark.parametrize("layout,field", [("field0", 0), ("field1", 1)])
def test_normal_draw_at_the_edges_is_finite_and_has_the_extreme_radius(layout, field):
    for e in C.select(layout, True) + C.select(layout, False):
        n = philox.sample_field(e.seed, e.offset, field, 1, 4, 1, row0=e.row)
        assert np.isfinite(n).all(), (e, n)
    for e in C.select(layout, False, 0):                      # the bottom word as u1: the largest radius
        n = philox.sample_field(e.seed, e.offset, field, 1, 4, 1, row0=e.row)
        rad = np.hypot(n[0, e.word], n[0, e.word + 1])
        assert abs(rad - C.R_MAX) <= 4 * np.finfo(np.float64).eps * C.R_MAX
    for e in C.select(layout, True, 0):                       # the top word as u1: the smallest radius, sqrt(-2 ln(1 - 2^-24)) > 0
        n = philox.sample_field(e.seed, e.offset, field, 1, 4, 1, row0=e.row)
        rad = np.hypot(n[0, e.word], n[0, e.word + 1])
        assert abs(rad - np.sqrt(-2.0 * np.log1p(-2.0 ** -24))) <= 1e-12


def test_c_oracle_probe_restates_u01_and_box_muller(oracle):
    """codes 7 / 8 / 9 of bgo_detmath_probe (the host mirror of bgk_detmath_probe): u01 has the bits of oracle/philox.py::u01 on the
    probe's words; the f32 Box-Muller pair on the deterministic log / sincos is finite and within the device test's bound of f64"""
    ref = C.probe_reference()
    w = ref["w"].view(np.float32)
    assert np.array_equal(oracle.detmath_probe(w, "u01").view(np.uint32), ref["u"].view(np.uint32))
    for which, want in (("normal_cos", ref["cos64"]), ("normal_sin", ref["sin64"])):
        got = oracle.detmath_probe(w, which)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want)
        print(f"{which}: max error {err.max():.3g}, at |n| > 1 {err[np.abs(want) > 1].max():.3g}")
        assert (err <= C.normal_bound(want, ref["err32_large"])).all()


def test_f32_box_muller_error_on_the_probe_words():
    """the figure the device bound of test_gpu_philox_edges.py::test_probe_u01_and_box_muller rests on: plain numpy-f32 Box-Muller against
    f64 on the probe's words.  Measured: 6.1e-7 at |n| > 1 (radii up to 5.887), 3.3e-7 at |n| <= 1; 4 x 6.1e-7 < 4e-6, so the suite's
    4e-6 holds at every radius."""
    ref = C.probe_reference()
    print(f"numpy f32 vs f64 Box-Muller on {ref['w'].size} words: {ref['err32_large']:.3g} at |n| > 1, {ref['err32_small']:.3g} at |n| <= 1")
    assert np.isfinite(ref["cos64"]).all() and np.isfinite(ref["sin64"]).all()
    assert float(np.abs(ref["cos64"]).max()) > 5.88                          # the largest radius is among the words
    assert ref["err32_small"] <= 4e-6 and 4 * ref["err32_large"] <= 4e-6
