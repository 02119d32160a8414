"""CPU: the host side of the fused sampling tail's bound windows -- cdf._tail_descriptor and the reverted cdf series it tabulates
(csrc/bgk_tail.hip::icdf_chan evaluates h = s + c2 s^2 + ... + c5 s^5 for s = v k < 0.03) -- against f64 / multi-precision."""
import warnings

import numpy as np
import pytest
import torch

import domain_maps_common as dm

ALPHAS = [-6.0, -5.0, -4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
# relative truncation error of the five-term series in h at the window's edge s = 0.03 (f64 against the multi-precision inverse):
# the figures this test pins, each rounded up in its second digit
EDGE_ERROR = {-6.0: 3.3e-5, -5.0: 1.4e-5, -4.0: 4.8e-6, -3.0: 1.3e-6, -2.0: 2.3e-7, -1.0: 2.0e-8, 0.0: 1.9e-11}


def _have_mpmath():
    try:
        import mpmath  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.mark.parametrize("alpha", ALPHAS)
def test_reverted_series_against_the_exact_inverse(alpha):
    """the five-term series against the exact solution of Phi(alpha + h) - Phi(alpha) = s pdf(alpha) over the whole window"""
    if not _have_mpmath() and abs(alpha) > 3.0:
        pytest.skip("the scipy form of the exact inverse is only good for |alpha| <= 3")
    s = np.array([1e-4, 1e-3, 0.01, 0.02, 0.0299, 0.03])
    h, hx = dm.series_h(alpha, s), dm.exact_h(alpha, s)
    rel = np.abs(h - hx) / hx
    print(f"alpha {alpha:+.0f}: relative truncation error of h at s = {s.tolist()}: {rel.tolist()}")
    assert np.all(np.diff(hx) > 0) and np.all(hx > 0)
    # the sixth-order term bounds the error: it grows like s^5 relative to h, so the edge is the worst point of the window
    assert rel.max() == rel[-1] or rel.max() < 1e-13
    if alpha in EDGE_ERROR:
        assert rel[-1] <= EDGE_ERROR[alpha], f"{rel[-1]:.3e}"
        assert rel[-1] >= 0.5 * EDGE_ERROR[alpha], f"the pinned figure is stale: {rel[-1]:.3e}"
    if alpha <= 0:
        assert rel[2] < 1.4e-7, f"s = 0.01: {rel[2]:.3e}"
    # a dropped or swapped coefficient is far outside these figures: four terms only are worse by orders of magnitude
    rel4 = np.abs(dm.series_h(alpha, s[-1:], terms=4) - hx[-1:]) / hx[-1:]
    if alpha != 0.0 and abs(alpha) != 1.0:
        assert rel4[0] > 5.0 * rel[-1]


def _desc(dist, d=1):
    from bgflow_amd.cdf import _tail_descriptor
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # an overflow in the f64 -> f32 cast warns: that is an error here
        return _tail_descriptor(dist, d).numpy()


@pytest.mark.parametrize("alpha,beta", [(-4.0, np.inf), (-3.0, 2.0), (-1.0, 0.75), (0.0, 2.0)])
def test_tail_descriptor_slots_against_f64(alpha, beta):
    dist = dm.truncated_normal(alpha, beta)
    ds = _desc(dist)[0]
    _, p = dm.params(dist, torch.float64)
    mu, sigma, clo, Z = (float(p[k][0]) for k in ("mu", "sigma", "clo", "Z"))
    cup = clo + Z
    from scipy import special as sps
    a_eff = float(sps.ndtri(clo))                       # the bound as the f32 cdf value places it
    pdf = np.exp(-0.5 * a_eff ** 2) / np.sqrt(2 * np.pi)
    want = {1: mu, 2: sigma * dm.SQRT2, 3: 2 * Z, 4: 2 * clo - 1, 5: np.log(Z * sigma) + dm.HALF_LOG_2PI, 6: 1 / (sigma * dm.SQRT2),
            7: Z / pdf, 12: mu + sigma * a_eff, 13: sigma}
    for slot, v in want.items():
        assert ds[slot] == np.float32(v), (slot, ds[slot], v)
    assert abs(a_eff - alpha) < 1e-3                    # (the module's f32 cdf value moves the bound by up to ~1e-4 sigma)
    from bgflow_amd.cdf import _reverted_cdf_series
    assert np.array_equal(ds[8:12], np.asarray(_reverted_cdf_series(a_eff), np.float32))
    if np.isfinite(beta):
        b_eff = float(sps.ndtri(cup))
        assert ds[14] == np.float32(Z / (np.exp(-0.5 * b_eff ** 2) / np.sqrt(2 * np.pi))) and ds[19] == np.float32(mu + sigma * b_eff)
        assert np.array_equal(ds[15:19], np.asarray(_reverted_cdf_series(-b_eff), np.float32))
    else:
        assert np.isposinf(ds[14]) and not ds[15:20].any()
    assert ds[:1].view(np.int32)[0] == 2


def test_no_bound_and_bound_too_far_share_one_sentinel_the_kernel_never_enters():
    """k = inf for a normal, for an absent bound and for a bound whose k = Z / pdf(bound) is no f32 (a cdf value of 1e-42, 13.6
    sigmas out: k = 3e40) -- without an overflow warning; and the kernel's window test s = v k < SMAX in f32 is false for
    every v >= 0 under that sentinel, v = 0 included (0 * inf = NaN), which no finite sentinel achieves"""
    # The module's own cdf of a bound (0.5 (1 + erf)) is 0 beyond 5.4 sigmas in f32 and beyond 8.3 in f64, which already reads as "no
    # bound": k <= 1e15 through the constructor.  A tiny cdf value reaches the descriptor only through the buffer (a loaded state).
    far = dm.truncated_normal(-3.0, np.inf, d=3)
    far._cdf_lower_bound.fill_(1e-42)                    # 13.6 sigmas: k = 3e40
    for dist, d in ((far, 3), (dm.normal(0.0, 20.0, 2), 2)):
        ds = _desc(dist, d)
        assert np.isposinf(ds[:, 7]).all() and np.isposinf(ds[:, 14]).all()
        assert not ds[:, 8:13].any() and not ds[:, 15:20].any()
    half = dm.truncated_normal(-3.0, np.inf)
    ds = _desc(half)
    assert np.isfinite(ds[0, 7]) and np.isposinf(ds[0, 14])
    v = np.concatenate([[0.0], dm.from_bits(np.arange(1, 64, dtype=np.uint32)), dm.binade_sweep(0, 127, 4), [np.inf]]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = v * np.float32(np.inf)
        assert not (s < dm.SMAX).any()
        assert (np.float32(0.0) * np.float32(1e30) < dm.SMAX)          # what the finite sentinel did at v = 0
    # the largest finite k still has a window; an f32-representable k is kept as it is
    from bgflow_amd.cdf import TAIL_K_MAX
    assert TAIL_K_MAX == float(np.finfo(np.float32).max)
    edge = dm.truncated_normal(-3.0, np.inf)
    edge._cdf_lower_bound.fill_(1e-33)                   # 12 sigmas: k = 5e31, beyond the old finite sentinel
    ds = _desc(edge)
    assert np.isfinite(ds[0, 7]) and ds[0, 7] > 1e30 and ds[0, 8:13].any()


def test_smallest_v_that_enters_a_window_of_the_builders_default_marginals():
    """the builder's default marginals (configs._ic_domain_maps, icmarginals.py:41-77): bonds N(1, 1) on [1e-5, inf) -- alpha = -1,
    k = 3.48: the lower window is entered for v < 8.63e-3; angles N(0.5, 1) on [1e-5, 1] -- alpha = -0.5, beta = 0.5, k = 1.09: both
    windows are entered within 2.76e-2 of an end.  So with uniform prior samples about 0.9 % of the bond channels and 5.5 % of the
    angle channels take the series branch."""
    from bgflow_amd import configs
    dims = {"BONDS": 17, "ANGLES": 17, "TORSIONS": 17, "FIXED": 9}
    slot = {f: i for i, f in enumerate(dims)}
    maps = configs._ic_domain_maps(dims, slot, dict(dtype=torch.float32))
    dists = [m._flow._delegate.distribution for m in maps]
    kb, ka = _desc(dists[0], 17), _desc(dists[1], 17)
    assert (kb == kb[:1]).all() and (ka == ka[:1]).all()
    v_b = float(dm.SMAX) / float(kb[0, 7])
    v_a_lo, v_a_hi = float(dm.SMAX) / float(ka[0, 7]), float(dm.SMAX) / float(ka[0, 14])
    print(f"window entered for v < {v_b:.4e} (bonds), v < {v_a_lo:.4e} or 1 - v < {v_a_hi:.4e} (angles)")
    assert np.isposinf(kb[0, 14])
    assert abs(v_b - 8.63e-3) < 1e-5 and abs(v_a_lo - 2.758e-2) < 1e-5 and abs(v_a_hi - 2.758e-2) < 1e-5
    assert all(np.isposinf(_desc(d_, n)[:, [7, 14]]).all() for d_, n in ((dists[3], 9),))     # the normal of the fixed field: no window
    assert _desc(dists[2], 17)[0, :1].view(np.int32)[0] == 0
