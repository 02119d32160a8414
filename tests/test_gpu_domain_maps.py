"""GPU (-m gpu): the CDF / ICDF domain maps PER ELEMENT against f64, at the ends of their domains and at the bounds of truncated
normals -- erf_fast / erfinv_fast (csrc/bgk_erf.h, through bgk_detmath_probe codes 5 / 6), the stand-alone bgk_cdf_transform /
bgk_cdf_backward (csrc/bgk_cdf.hip), icdf_chan and the bound windows of the fused sampling tail and cdf_chan / atan2_fast of the
inference head (csrc/bgk_tail.hip), and the older bgk_icdf_ic2xyz (csrc/bgk_ic.hip).  No element is left out of an assertion, except gradients where
the map itself is not finite.

Bounds (tests/domain_maps_common.py): outside a bound window |v - v64| <= 4 |v32_ref - v64| + 4 ulp(v64) with v32_ref the reference's
own f32 torch op chain on the CPU (row sums: 2^-22 |dlogp64| in place of the ulp term; non-finite results: the same infinity sign /
NaN-ness as that chain).  Where the run on the MI355X showed that bound out of f32's reach with the chain's error R taken at the element
alone, R is taken over the element's own input point or its own row (dm.within), never wider; each test says which and why.  Inside a window |y - y64| <= E_m + ulp(y64) + 8 * 2^-24 sigma h with E_m the f64 series' own error."""
import numpy as np
import pytest
import torch
from scipy import special as sps

import domain_maps_common as dm

pytestmark = pytest.mark.gpu

# Maximum error of the two functions against f64 over the sweeps below, measured on an MI355X and rounded up to the next half ulp
# (erf_fast: 1.262 ulp at 0.93813723, erfinv_fast: 2.738 ulp at 0.822265625).  csrc/bgk_erf.h and DESIGN.md section 4 quote these constants.
ERF_MAX_ULP = 1.5
ERFINV_MAX_ULP = 3.0


def _probe(hip_lib, dev, x, which):
    from bgflow_amd import _lib
    xd = torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(dev)
    out = torch.empty_like(xd)
    assert hip_lib.bgk_detmath_probe(_lib.ptr(xd), xd.numel(), which, _lib.ptr(out), _lib.stream_ptr(dev)) == 0
    return out.cpu().numpy()


def _report(name, err, x):
    i = int(np.argmax(err))
    print(f"{name}: {err.size} points, max {err[i]:.3f} ulp at x = {float(x[i])!r} ({x[i:i + 1].view(np.uint32)[0]:#010x}), mean {err.mean():.3f} ulp")


# ---- (a) erf_fast -------------------------------------------------------------------------------------------------------------
def test_erf_fast_per_element(hip_lib, dev):
    """both signs of 256 mantissas in every binade from 2^-126 to 2^4 and of the subnormals, every float in [0.92, 0.94] (the branch
    switch is at 0.927734375), the saturated range and the special values"""
    pos = np.concatenate([dm.binade_sweep(0, 131), dm.floats_between(0.92, 0.94),
                          np.asarray([0.0, 2.0 ** -149, 2.0 ** -127, 3.8, 3.9, 3.92, 4.0, 4.5, 5.0, 6.0, 8.0, 10.0, 1e30, np.inf], np.float32)])
    got_p, got_n = _probe(hip_lib, dev, pos, 5), _probe(hip_lib, dev, -pos, 5)
    assert np.array_equal(dm.bits(got_n), dm.bits(got_p) ^ np.uint32(0x80000000)), "erf_fast(-a) != -erf_fast(a) bit for bit"
    ref = sps.erf(pos.astype(np.float64))
    err = dm.ulp_error(got_p, ref)
    _report("erf_fast", err, pos)
    for lo, hi in ((0.0, 2.0 ** -126), (2.0 ** -126, 0.92), (0.92, 0.94), (0.94, 4.0)):
        m = (pos >= lo) & (pos < hi)
        print(f"  [{lo:.3g}, {hi:.3g}): max {err[m].max():.3f} ulp")
    assert err.max() <= ERF_MAX_ULP
    sat = pos >= 4.0                                    # 1 - erf(4) = 1.5e-8 < 2^-25: f32 has nothing between it and 1
    assert sat.sum() >= 7 and np.array_equal(dm.bits(got_p[sat]), dm.bits(np.ones(int(sat.sum()), np.float32)))
    assert dm.bits(got_p[pos == 0.0])[0] == 0 and (np.abs(got_p) <= 1.0).all()
    assert np.isnan(_probe(hip_lib, dev, np.asarray([np.nan, -np.nan], np.float32), 5)).all()
    # monotone across the branch switch
    sw = np.sort(dm.floats_between(0.92, 0.94))
    assert (np.diff(_probe(hip_lib, dev, sw, 5).astype(np.float64)) >= 0).all()


# ---- (b) erfinv_fast ----------------------------------------------------------------------------------------------------------
def test_erfinv_fast_per_element(hip_lib, dev):
    """every float in [1 - 2^-8, 1), +-2^13 floats around the w = 5 switch at |x| = sqrt(1 - e^-5), 256 mantissas in every binade
    down to the subnormals, both signs"""
    one_m = np.nextafter(np.float32(1.0), np.float32(0.0))
    sw = int(dm.bits([dm.ERFINV_SWITCH])[0])
    pos = np.concatenate([dm.floats_between(1.0 - 2.0 ** -8, one_m), dm.from_bits(np.arange(sw - (1 << 13), sw + (1 << 13) + 1, dtype=np.uint32)),
                          dm.binade_sweep(0, 126)])
    got_p, got_n = _probe(hip_lib, dev, pos, 6), _probe(hip_lib, dev, -pos, 6)
    assert np.array_equal(dm.bits(got_n), dm.bits(got_p) ^ np.uint32(0x80000000)), "erfinv_fast(-x) != -erfinv_fast(x) bit for bit"
    ref = sps.erfinv(pos.astype(np.float64))
    assert np.isfinite(got_p).all()
    err = dm.ulp_error(got_p, ref)
    _report("erfinv_fast", err, pos)
    for lo, hi in ((0.0, 2.0 ** -126), (2.0 ** -126, 0.99), (0.99, dm.ERFINV_SWITCH), (dm.ERFINV_SWITCH, 1.0 - 2.0 ** -12), (1.0 - 2.0 ** -12, 1.0)):
        m = (pos >= lo) & (pos < hi)
        print(f"  [{lo:.6g}, {hi:.8g}): max {err[m].max():.3f} ulp, mean {err[m].mean():.3f}")
    assert err.max() <= ERFINV_MAX_ULP


def test_erfinv_fast_special_values(hip_lib, dev):
    """+-0 keeps its sign; +-1 gives +-inf (the tail polynomial's q(inf) = -inf gave -+inf); |x| > 1 and NaN give NaN"""
    x = np.asarray([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), -np.nextafter(np.float32(1), np.float32(2)), 2.0, -2.0,
                    1e30, -1e30, np.inf, -np.inf, np.nan], np.float32)
    for pad in (0.0, 0.999):                            # in a wave without and with other tail lanes
        got = _probe(hip_lib, dev, np.concatenate([x, np.full(64 - x.size, pad, np.float32)]), 6)[:x.size]
        print("erfinv_fast specials:", dict(zip(x.tolist(), got.tolist())))
        assert dm.bits(got[:2]).tolist() == [0, 0x80000000]
        assert got[2] == np.inf and got[3] == -np.inf
        assert np.isnan(got[4:]).all()


def test_erfinv_fast_is_independent_of_the_wave_composition(hip_lib, dev):
    """the tail branch sits behind a wave-level ballot: the same x must give the same bits in a wave with no tail lane, with only
    tail lanes and with exactly one tail lane (the probe runs 256-thread blocks: elements 64 k .. 64 k + 63 share a wave)"""
    c = np.linspace(-0.99, 0.99, 64).astype(np.float32)                                # w < 5
    tl = dm.floats_between(dm.ERFINV_SWITCH, 1.0)[1:-1]
    tl = tl[np.linspace(0, tl.size - 1, 64).astype(np.int64)] * np.where(np.arange(64) % 2, -1.0, 1.0).astype(np.float32)   # w >= 5
    one = np.tile(c, (64, 1))
    one[np.arange(64), np.arange(64)] = tl                                             # wave i: lane i is the only tail lane
    one_c = np.tile(tl, (64, 1))
    one_c[np.arange(64), np.arange(64)] = c                                            # ... and the only central lane
    x = np.concatenate([c, tl, one.reshape(-1), one_c.reshape(-1)])
    got = _probe(hip_lib, dev, x, 6)
    g_c, g_t, g_one, g_onec = got[:64], got[64:128], got[128:128 + 4096].reshape(64, 64), got[128 + 4096:].reshape(64, 64)
    want = np.tile(g_c, (64, 1))
    want[np.arange(64), np.arange(64)] = g_t
    assert np.array_equal(dm.bits(g_one), dm.bits(want))
    want_c = np.tile(g_t, (64, 1))
    want_c[np.arange(64), np.arange(64)] = g_c
    assert np.array_equal(dm.bits(g_onec), dm.bits(want_c))


# ---- (c), (d) the stand-alone maps ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (257, 1), (7, 3), (241, 17)]      # d = 1: own row-index branch; d = 3: an empty row-sum lane; d = 17: 240-row tiles + 1 row
EPS = [1e-7, 1e-3, None]
MARGINALS = {
    "uniform": lambda d: dm.uniform(-0.3, 1.7, d),
    "normal": lambda d: dm.normal(0.0, 20.0, d),
    "tn(-3,inf)": lambda d: dm.truncated_normal(-3.0, np.inf, d),
    "tn(-1,2)": lambda d: dm.truncated_normal(-1.0, 2.0, d),
    "tn(0,0.75)": lambda d: dm.truncated_normal(0.0, 0.75, d),
    "tn(-4,4)": lambda d: dm.truncated_normal(-4.0, 4.0, d),
}


def _inputs(dist, name, inverse, eps, B, d):
    """([B, d] f32 inputs, [B, d] point ids) of one case: the icdf edge points per column, or (cdf direction) their f64 icdf plus --
    for a uniform -- points outside the support by more and by less than its tolerance.  Elements with one id share an input point."""
    pts = dm.icdf_edge_inputs(eps)
    pid = (np.arange(B)[:, None] + np.arange(d)[None, :]) % len(pts)
    u = np.ascontiguousarray(pts[pid])
    if inverse:
        return u, pid
    with np.errstate(all="ignore"):
        x = dm.icdf_exact(dist, u.astype(np.float64)).astype(np.float32)
    if name == "uniform":
        low, high, tol = dist.low.numpy(), dist.high.numpy(), np.float32(dist.tol)
        out = np.stack([low - 2 * tol, low - tol / 2, high + tol / 2, high + 2 * tol]).astype(np.float32)       # [4, d]
        rows = np.arange(B) % 7 == 3
        which = (np.arange(B) // 7) % 4
        x[rows] = out[which][rows]
        pid[rows] = len(pts) + which[rows, None]
    return x, pid


def _cases(name, inverse, eps):
    """every shape of one (marginal, direction, eps) with both reference chains, and the f32 chain's error per input point: its
    maximum over all shapes and columns (the columns of a map have different parameters), for y and for the per-element log-det"""
    cases, n_pid = [], len(dm.icdf_edge_inputs(eps)) + 4
    r_y, r_l = np.zeros(n_pid), np.zeros(n_pid)
    for B, d in SHAPES:
        dist = MARGINALS[name](d)
        x, pid = _inputs(dist, name, inverse, eps, B, d)
        y64, l64, y32, l32 = dm.chain_np(dist, x, inverse, eps)
        for r, v32, v64 in ((r_y, y32, y64), (r_l, l32, l64)):
            with np.errstate(invalid="ignore"):
                e = np.abs(v32.astype(np.float64) - v64)
            fin = np.isfinite(e)
            np.maximum.at(r, pid[fin], e[fin])
        cases.append(dict(B=B, d=d, dist=dist, x=x, pid=pid, y64=y64, l64=l64, y32=y32, l32=l32))
    return cases, r_y, r_l


def _launch_cdf(hip_lib, dev, x, desc, inverse, eps, pad=0, acc0=None):
    """bgk_cdf_transform through the C entry: ``pad`` extra floats per input / output row (ldx, ldo > d), ``acc0`` = initial contents of
    the log-det buffer (accumulate = 1)"""
    from bgflow_amd import _lib
    B, d = x.shape
    xin = torch.full((B, d + pad), 7.0, dtype=torch.float32, device=dev)
    xin[:, :d] = torch.as_tensor(x).to(dev)
    out = torch.full((B, d + pad), -7.0, dtype=torch.float32, device=dev)
    dl = torch.empty(B, dtype=torch.float32, device=dev) if acc0 is None else torch.as_tensor(acc0).to(dev).clone()
    st = hip_lib.bgk_cdf_transform(_lib.ptr(xin), d + pad, _lib.ptr(desc), B, d, int(inverse), int(eps is not None), float(eps or 0.0),
                                   _lib.ptr(out), d + pad, _lib.ptr(dl), int(acc0 is not None), _lib.stream_ptr(dev))
    assert st == 0
    assert bool((out[:, d:] == -7.0).all()), "the kernel wrote past a row's d columns"
    return out[:, :d].cpu().numpy(), dl.cpu().numpy()


def _floor_1_over_eps(dl, eps):
    """the log-det floor of CDFTransform: -1 / eps (the kernel divides in f32, the reference rounds the f64 quotient: one ulp apart)"""
    return np.abs(dl.astype(np.float64) + 1.0 / eps) <= 2.0 * dm.ulp32(1.0 / eps)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("inverse", [True, False], ids=["icdf", "cdf"])
@pytest.mark.parametrize("name", list(MARGINALS))
def test_cdf_transform_per_element(hip_lib, dev, name, inverse, eps):
    """bgk_cdf_transform through CDFTransform and through the C entry (ldx, ldo > d and accumulate = 1), every shape.  The bound taken
    literally, with R at the element alone, is not attainable in f32 (the count of elements beyond it is printed: up to 154 of 4097
    for a map; the f32 chain rounds exactly at some elements, and next to a bound (Phi - cdf_lower) / Z cancels): R is the f32 chain's
    error at the element's own input point, its maximum over the columns that hold that point (their parameters differ by 5 % per
    column); for a row sum, over the rows that hold the same points."""
    import bgflow_amd as bg
    from bgflow_amd.cdf import _descriptor
    cases, r_y, r_l = _cases(name, inverse, eps)
    misses, worst, literal = [], 0.0, 0
    for c in cases:
        B, d, dist, x, pid = c["B"], c["d"], c["dist"], c["x"], c["pid"]
        desc = _descriptor(dist, d).to(dev)
        layer = bg.CDFTransform(MARGINALS[name](d).to(dev), eps=eps)
        with torch.no_grad():
            y_t, dl_t = (layer._inverse if inverse else layer._forward)(torch.as_tensor(x).to(dev))
        y, dl = y_t.cpu().numpy(), dl_t.cpu().numpy()[:, 0]
        tag = f"{name} {'icdf' if inverse else 'cdf'} B={B} d={d} eps={eps}"
        ok, ratio = dm.within(y, c["y64"], c["y32"], ref_err=r_y[pid])
        literal += int((~dm.within(y, c["y64"], c["y32"])[0]).sum())
        for i, j in np.argwhere(~ok)[:6]:
            misses.append(f"{tag}: y[{i},{j}] x {x[i, j]!r} got {y[i, j]!r} f64 {c['y64'][i, j]!r} f32 chain {c['y32'][i, j]!r} error/bound {ratio[i, j]:.2f}")
        s64, s32 = c["l64"].sum(-1), torch.as_tensor(c["l32"]).sum(-1).numpy()
        with np.errstate(invalid="ignore"):
            # the floor of a row sum: 2^-22 times the sum of the MAGNITUDES of its d terms (= 2^-22 |dlogp64| where nothing cancels).
            # An f32 sum carries a rounding of each term, whatever its order: a row that holds u = eps and u = 1 - eps adds +-13.6 to
            # a sum of -2, and 2^-22 * 2 = 4.6e-7 is half a rounding of 13.6.
            p64 = np.abs(c["l64"]).sum(-1)
            if d == 1:                                  # per element
                okl, ratio_l = dm.within(dl, s64, s32, floor=2.0 ** -22 * p64, ref_err=r_l[pid[:, 0]])
            else:                                       # row sums: R over the rows with the same input points (column j of row r holds point r + j)
                okl, ratio_l = dm.within(dl, s64, s32, floor=2.0 ** -22 * p64, groups=pid[:, 0])
            literal += int((~dm.within(dl, s64, s32, floor=2.0 ** -22 * np.abs(s64))[0]).sum())
        for i in np.nonzero(~okl)[0][:6]:
            misses.append(f"{tag}: log-det[{i}] got {dl[i]!r} f64 {s64[i]!r} f32 chain {s32[i]!r} error/bound {ratio_l[i]:.2f}")
        worst = max(worst, float(ratio.max()), float(ratio_l.max()))
        if d == 1 and name == "uniform" and not inverse and B > 7:      # -inf outside a uniform's support, floored at -1 / eps
            outside = (x[:, 0] < dist.low.numpy()[0] - dist.tol) | (x[:, 0] > dist.high.numpy()[0] + dist.tol)
            assert outside.sum() >= 2 and (~outside).sum() > 2
            if eps is None:
                assert np.isneginf(dl[outside]).all() and np.isfinite(dl[~outside]).all()
            else:
                assert _floor_1_over_eps(dl[outside], eps).all() and (dl[~outside] > -1.0).all()
        if eps is not None:
            assert (dl.astype(np.float64) >= -d * (1.0 / eps) * (1 + 2.0 ** -22)).all()
        # the C entry: row strides wider than d, and accumulation into a log-det buffer that holds something
        acc0 = (np.arange(B, dtype=np.float32) - 3.0) * np.float32(0.25)
        y_c, dl_c = _launch_cdf(hip_lib, dev, x, desc, inverse, eps, pad=3, acc0=acc0)
        assert np.array_equal(dm.bits(y_c), dm.bits(y)), f"{tag}: ldx > d changes y"
        with np.errstate(invalid="ignore"):
            assert np.array_equal(dm.bits(dl_c), dm.bits(acc0 + dl)), f"{tag}: accumulate = 1 is not buffer + log-det"
    print(f"{name} {'icdf' if inverse else 'cdf'} eps={eps}: worst error / bound {worst:.3f}; {literal} elements beyond the bound with R taken at the element alone")
    assert not misses, "\n".join(misses)


def _vjp_pieces(dist, x, y, inverse, eps):
    """f64 pieces of the map's VJP at the f32 inputs x and the f64 forward values y, for the conditioning terms of the gradient bound:
    (dy/dx, |z|, sigma, per-element log-det, d logdet / dx)"""
    kind, p = dm.params(dist, torch.float64)
    x = x.astype(np.float64)
    if kind == 0:
        w = (p["high"] - p["low"]).numpy()
        u = (x - p["low"].numpy()) / w
        dy = np.broadcast_to(w, x.shape) if inverse else np.where((u >= 0) & (u <= 1), 1.0 / w, 0.0)
        return dy, np.zeros(x.shape), np.ones(x.shape), np.zeros(x.shape), np.zeros(x.shape)
    mu, sigma = p["mu"].numpy(), p["sigma"].numpy()
    logn = np.log(sigma * (p["Z"].numpy() if kind == 2 else 1.0)) + dm.HALF_LOG_2PI
    with np.errstate(all="ignore"):
        z = ((y if inverse else x) - mu) / sigma
        ld = (0.5 * z * z + logn) if inverse else -(0.5 * z * z + logn)
        dy = np.exp(ld)
        dld = (z / sigma) * dy if inverse else -z / sigma
    return dy, np.abs(z), np.broadcast_to(sigma, x.shape), ld, dld


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("inverse", [True, False], ids=["icdf", "cdf"])
@pytest.mark.parametrize("name", list(MARGINALS))
def test_cdf_backward_per_element(hip_lib, dev, name, inverse, eps):
    """bgk_cdf_backward against f64 autograd of the distributions' own ops with torch.clamp, both cotangents non-zero, on the forward
    kernel's own y.  The gradient passes at u == eps and u == 1 - eps in the icdf direction (torch.clamp's rule); in the cdf direction
    the kernel sees only the saved y, so a y that equals a clamp bound passes none and every other y passes: where the f64 forward value
    is clear of the bounds the saved y must sit on a bound exactly when autograd's clamp fires; the gradient is then compared with
    autograd's log-det part alone where the saved y sits on a bound and with autograd of the unclamped y elsewhere.

    Bound: |g - g64| <= 4 R + F.  R: the f32 autograd's error, maximum over the elements that share the input point.  F, the part any
    f32 evaluation on a saved f32 y has: with T = |g_y dy| + |g_l dlogdet| (the two terms, which may cancel), T (8 + 4 |logdet|) 2^-24
    for the roundings and for exp of an f32 log-det, and in the icdf direction, where dy = exp(z^2 / 2 + c) is formed from the
    rounded y, dz = 4 ulp(y) / sigma: (|g_y| dy |z| + |g_l| dy (1 + z^2) / sigma) dz.  The median of F / 4 R is printed.
    Elements at which autograd's gradient is not finite (eps=None at u = 0 or 1) have no value to compare: the kernel's must not be
    finite there either."""
    from bgflow_amd.cdf import _descriptor, cdf_backward
    cases, _, _ = _cases(name, inverse, eps)
    lo = hi = None
    if eps is not None:
        lo, hi = np.float32(eps), np.float32(1.0) - np.float32(eps)
    floor_over_r = []
    n_pid = len(dm.icdf_edge_inputs(eps)) + 4
    r_g = np.zeros(n_pid)
    work = []
    for c in cases:
        B, d, dist, x, pid = c["B"], c["d"], c["dist"], c["x"], c["pid"]
        rs = np.random.RandomState(B + d)
        g_y = (0.5 + rs.rand(B, d)).astype(np.float32) * np.where(rs.rand(B, d) < 0.5, -1, 1).astype(np.float32)
        g_l = (0.5 + rs.rand(B)).astype(np.float32) * np.where(rs.rand(B) < 0.5, -1, 1).astype(np.float32)
        grads = {}
        for dtype in (torch.float64, torch.float32):
            parts = []
            for with_y in (1, 0, 2):                    # the whole gradient, the log-det's part alone, and the whole with y unclamped
                xt = torch.as_tensor(x).to(dtype).requires_grad_(True)
                yy, ll = dm.chain(dist, xt, inverse, eps, dtype)
                if with_y == 2:
                    yy = dm.chain(dist, xt, inverse, None, dtype)[0]
                fin = torch.isfinite(yy) & torch.isfinite(ll)       # (a non-finite output has no gradient to compare)
                if with_y == 1:
                    fin_chain = fin.numpy()
                loss = (torch.where(fin, ll, torch.zeros_like(ll)).sum(-1) * torch.as_tensor(g_l).to(dtype)).sum()
                if with_y:
                    loss = loss + (torch.where(fin, yy, torch.zeros_like(yy)) * torch.as_tensor(g_y).to(dtype)).sum()
                gr = torch.autograd.grad(loss, xt, allow_unused=True)[0] if loss.requires_grad else None       # (a uniform's log-det is constant)
                parts.append(np.zeros(x.shape, np.float64 if dtype == torch.float64 else np.float32) if gr is None else gr.numpy())
            grads[dtype] = (parts[0], parts[1], parts[2], fin_chain)
        (g64, g64_l, g64_u, fin64), (g32, g32_l, g32_u, fin32) = grads[torch.float64], grads[torch.float32]
        y_k, _ = _launch_cdf(hip_lib, dev, x, desc := _descriptor(dist, d).to(dev), inverse, eps)
        g = cdf_backward(torch.as_tensor(x).to(dev), torch.as_tensor(y_k).to(dev), desc, inverse, eps, torch.as_tensor(g_y).to(dev),
                         torch.as_tensor(g_l).to(dev)).cpu().numpy()
        on_bound = np.zeros(x.shape, bool)
        if eps is not None and not inverse:             # the saved y sits on a clamp bound: only the log-det's cotangent arrives
            on_bound = (y_k == lo) | (y_k == hi)
            with torch.no_grad():
                y_pre = dm.chain(dist, torch.as_tensor(x), inverse, None, torch.float64)[0].numpy()
                y_pre32 = dm.chain(dist, torch.as_tensor(x), inverse, None, torch.float32)[0].numpy()
            # "clear of a bound": by more than 16 ulp of it plus 8 times what the f32 chain itself misses the unclamped value by at this point
            slack = 8.0 * dm.group_max(np.abs(y_pre32 - y_pre), pid)
            clear = (np.abs(y_pre - float(lo)) > 16 * dm.ulp32(float(lo)) + slack) & (np.abs(y_pre - float(hi)) > 16 * dm.ulp32(float(hi)) + slack)
            inside = (y_pre > float(lo)) & (y_pre < float(hi))
            assert (on_bound[clear] == ~inside[clear]).all(), "a clamped y must sit on the bound, an unclamped one must not"
            assert on_bound.any() or B < 13
            # ... and everything else its own: whether an element within a rounding of the bound was clamped is the forward's business
            g64, g32 = np.where(on_bound, g64_l, g64_u), np.where(on_bound, g32_l, g32_u)
        cmp = np.isfinite(x) & np.isfinite(g64) & np.isfinite(g32)
        with np.errstate(invalid="ignore"):
            e = np.where(cmp, np.abs(g32.astype(np.float64) - g64), 0.0)
        np.maximum.at(r_g, pid, e)
        dy, az, sigma, ld, dld = _vjp_pieces(dist, x, c["y64"], inverse, eps)
        with np.errstate(all="ignore"):
            t = np.where(on_bound, 0.0, np.abs(g_y * dy)) + np.abs(g_l[:, None] * dld)
            floor = t * (8.0 + 4.0 * np.abs(ld)) * 2.0 ** -24
            if inverse:
                dz = 4.0 * dm.ulp32(c["y64"]) / sigma
                floor = floor + (np.abs(g_y) * dy * az + np.abs(g_l[:, None]) * dy * (1.0 + az * az) / sigma) * dz
        work.append((c, g, g64, g32, cmp, floor, f"{name} {'icdf' if inverse else 'cdf'} backward B={B} d={d} eps={eps}"))
    misses, worst = [], 0.0
    for c, g, g64, g32, cmp, floor, tag in work:
        x, pid = c["x"], c["pid"]
        z0 = lambda a: np.where(cmp, a, 0.0)            # noqa: E731
        ok, ratio = dm.within(z0(g), z0(g64), z0(g32), floor=z0(floor), ref_err=r_g[pid])
        worst = max(worst, float(ratio.max()))
        with np.errstate(all="ignore"):
            floor_over_r.append(np.median((floor / (4.0 * r_g[pid]))[cmp & (r_g[pid] > 0)]) if (cmp & (r_g[pid] > 0)).any() else 0.0)
        # where autograd's gradient is not finite in a chain (eps=None at u = 0 or 1) there is no value to compare: the kernel's
        # gradient must not be an ordinary number there either
        lost = ~cmp & np.isfinite(x)
        print(f"{tag}: {int(lost.sum())} elements without a finite reference gradient; the kernel's there: {np.unique(g[lost])[:6]}")
        assert (~np.isfinite(g[lost])).all(), f"{tag}: finite gradients {g[lost][np.isfinite(g[lost])][:4]} at x {x[lost][np.isfinite(g[lost])][:4]} where autograd's is not"
        for i, j in np.argwhere(~ok)[:6]:
            misses.append(f"{tag}: g[{i},{j}] x {x[i, j]!r} got {g[i, j]!r} f64 {g64[i, j]!r} f32 autograd {g32[i, j]!r} error/bound {ratio[i, j]:.2f}")
        if eps is not None and inverse:
            at_edge, beyond = (x == lo) | (x == hi), (x < lo) | (x > hi)
            assert (at_edge.any() and beyond.any()) or c["B"] < 13
            assert (g[beyond] == 0.0).all() and (g64[beyond] == 0.0).all()
            assert (g[at_edge] != 0.0).all() and (g64[at_edge] != 0.0).all()
    print(f"{name} {'icdf' if inverse else 'cdf'} backward eps={eps}: worst error / bound {worst:.3f}; median F / 4 R {np.max(floor_over_r):.2f} (largest over the shapes)")
    assert not misses, "\n".join(misses)


# ---- (e), (f) bound windows of the fused sampling tail ------------------------------------------------------------------------------
ALPHA_BETA = [(a, b) for a in (-4.0, -3.0, -1.0, 0.0) for b in (0.75, 2.0, np.inf)]
S_POINTS = [1e-4, 1e-3, 0.01, 0.0299, 0.031]
B_TAIL = 130                                            # two 64-sample tiles and two rows


@pytest.fixture(scope="module")
def ala2(dev):
    """the coordinate transform of the cfg-3 generator on the device and on the CPU"""
    from test_gpu_round3 import _make
    pick = lambda gen: [m for m in gen.flow.modules() if type(m).__name__ == "MixedCoordinateTransformation"][0]       # noqa: E731
    return pick(_make("cfg3", dev)), pick(_make("cfg3"))


def _crossing(k32, upper):
    """the two f32 neighbours v of the SMAX crossing of s = v k (lower bound) resp. s = (1 - v) k (upper bound), evaluated as the
    kernel does (f32 product, f32 compare): (last v inside the window, first v outside)"""
    one = np.float32(1.0)
    inside = (lambda v: (one - v) * k32 < dm.SMAX) if upper else (lambda v: v * k32 < dm.SMAX)
    v = np.float32(one - dm.SMAX / k32) if upper else np.float32(dm.SMAX / k32)
    step = np.float32(-np.inf) if upper else np.float32(np.inf)            # direction that leaves the window
    while inside(v):
        v = np.nextafter(v, step)
    while not inside(np.nextafter(v, -step)):
        v = np.nextafter(v, -step)
    return np.nextafter(v, -step), v


def _tail_case(alpha, beta, eps, n, keep, spread=0.0):
    """(marginals, the four [B, w] f32 input fields) of one case: in every row one channel of the bonds or of the angles field takes a
    special v; all other channels stay in (0.2, 0.8)"""
    from bgflow_amd.cdf import _tail_descriptor
    dists = [dm.truncated_normal(alpha, beta, n, lower=0.5, sigma=0.1, spread=spread), dm.truncated_normal(alpha, beta, n, lower=0.3, sigma=0.05, spread=spread),
             dm.uniform(0.0, 1.0, n, spread=0.0), dm.normal(0.0, 1.0, keep, spread=spread)]
    rs = np.random.RandomState(int(10 * abs(alpha)) + (7 if np.isinf(beta) else int(4 * beta)))
    vs = [(0.2 + 0.6 * rs.rand(B_TAIL, w)).astype(np.float32) for w in (n, n, n, keep)]
    special = []                                        # [field][channel]: the channel's own special points
    for f in (0, 1):
        per_channel = []
        for ds in _tail_descriptor(dists[f], n).numpy():
            pts = [np.float32(s / float(ds[7])) for s in S_POINTS] + list(_crossing(ds[7], False))
            if np.isfinite(ds[14]):
                pts += [np.float32(1.0) - np.float32(s / float(ds[14])) for s in S_POINTS] + list(_crossing(ds[14], True))
            if eps is None:
                pts += [np.float32(0.0), np.float32(1.0)]
            per_channel.append(pts)
        special.append(per_channel)
    for r in range(B_TAIL):
        f, q = r % 2, r // 2
        pts = special[f][q % n]
        vs[f][r, q % n] = pts[q % len(pts)]
    return dists, vs


def _point_groups(dists, eps, n):
    """group id of every row of a tail case: the rows that give the same special v to the same field (_tail_case)"""
    from bgflow_amd.cdf import _tail_descriptor
    npts = []
    for f in (0, 1):
        ds = _tail_descriptor(dists[f], n).numpy()[0]
        npts.append(len(S_POINTS) + 2 + (len(S_POINTS) + 2 if np.isfinite(ds[14]) else 0) + (2 if eps is None else 0))
    r = np.arange(B_TAIL)
    return (r % 2) * 64 + (r // 2) % np.asarray(npts)[r % 2]


def _tail_tables(dists, rel, dev):
    """the descriptor tables of the tail kernels as flow._FusedGenerationTail._desc20 builds them: [3 n + keep, 20] in placement order
    with the field-uniform [4, 20] table attached, and the four [w, 6] tables of the older kernel"""
    from bgflow_amd.cdf import _descriptor, _tail_descriptor
    n, keep = rel._n, 9
    parts = [_tail_descriptor(dist, w) for dist, w in zip(dists, (n, n, n, keep))]
    idx = torch.as_tensor(rel._placement_zrows)
    tab = torch.cat([parts[0][idx], parts[1][idx], parts[2][idx], parts[3]], dim=0).contiguous().to(dev)
    uniform = all(bool((p == p[:1]).all()) for p in parts)
    tab.uniform4 = torch.cat([p[:1] for p in parts], dim=0).contiguous().to(dev) if uniform else None
    return tab, [_descriptor(dist, w).to(dev) for dist, w in zip(dists, (n, n, n, keep))]


def _tail_reference(ic_cpu, dists, vs, eps, dtype):
    """the tail as the reference runs it, in ``dtype`` on the CPU: the four icdf maps (torch ops of the distributions, torch.clamp),
    then IC -> xyz with blackening (oracle/torch_flow.py::ic2xyz_torch) -> (mapped fields, x, dlogp [B], P [B]).
    P is the sum of the MAGNITUDES of what dlogp adds up: the maps' per-element log-dets, the coordinate transform's log-det and
    its constant n (ln pi + ln 2 pi) (the kernels start from the constant: their partial sums reach it).  An f32 sum carries a
    rounding of each term and partial sum, whatever its order, so where terms cancel the floor of a row sum is 2^-22 P instead of
    2^-22 |dlogp64|; the two agree where nothing cancels."""
    from oracle.torch_flow import ic2xyz_torch
    ys, ld, mag = [], 0.0, 0.0
    with torch.no_grad():
        for dist, v in zip(dists, vs):
            y, l = dm.chain(dist, torch.as_tensor(v), True, eps, dtype)
            ys.append(y)
            ld = ld + l.sum(-1)
            mag = mag + l.abs().sum(-1)
        ic = ic_cpu if dtype == torch.float32 else _ic64(ic_cpu)
        x, dl = ic2xyz_torch(ic, *ys)
        mag = mag + dl[:, 0].abs() + ys[0].shape[1] * (np.log(np.pi) + np.log(2.0 * np.pi))
    return [y.numpy() for y in ys], x.numpy(), (ld + dl[:, 0]).numpy(), mag.numpy()


_IC64 = {}


def _ic64(ic_cpu):
    if id(ic_cpu) not in _IC64:
        import copy
        _IC64[id(ic_cpu)] = copy.deepcopy(ic_cpu).double()      # the f32 whitening buffers, widened
    return _IC64[id(ic_cpu)]


def _window_bound(dist, v_cl, upper):
    """inside a window: (E_m, y64, the bound E_m + ulp(y64) + 8 * 2^-24 sigma h) at the clamped inputs v_cl (f32), all f64.  The series
    is the host's: cdf._tail_descriptor's f64 constants before they are rounded to f32."""
    _, p = dm.params(dist, torch.float64)
    mu, sigma, clo, Z = (float(p[k][0]) for k in ("mu", "sigma", "clo", "Z"))
    c = clo + Z if upper else clo
    x0 = float(sps.ndtri(c))
    pdf = np.exp(-0.5 * x0 * x0) / np.sqrt(2.0 * np.pi)
    v = v_cl.astype(np.float64)
    s = ((1.0 - v) if upper else v) * (Z / pdf)
    h = dm.series_h(-x0 if upper else x0, s)
    y_series = (mu + sigma * x0) + (-sigma if upper else sigma) * h
    y64 = mu + sigma * sps.ndtri(Z * v + clo)          # (field-uniform: column 0 stands for all)
    e_m = np.abs(y_series - y64)
    return e_m, y64, e_m + dm.ulp32(y64) + 8.0 * 2.0 ** -24 * sigma * h


def _check_fields(dists, vs, ys, eps, ref64, ref32, tag):
    """per element: the window bound where the kernel takes a window (its own f32 test), the chain bound elsewhere"""
    from bgflow_amd.cdf import _tail_descriptor
    n_win = 0
    worst_w = worst_o = 0.0
    for f in range(4):
        v, y, y64, y32 = vs[f], ys[f], ref64[f], ref32[f]
        v_cl = v if eps is None else np.clip(v, np.float32(eps), np.float32(1.0) - np.float32(eps))
        in_win = np.zeros(v.shape, bool)
        if f < 2:
            ds = _tail_descriptor(dists[f], v.shape[1]).numpy()[0]
            with np.errstate(invalid="ignore"):
                wins = [(v_cl * ds[7] < dm.SMAX, False), ((np.float32(1.0) - v_cl) * ds[14] < dm.SMAX, True)]
            for m, upper in wins:
                if not m.any():
                    continue
                e_m, yw64, bound = _window_bound(dists[f], v_cl[m], upper)
                err = np.abs(y[m].astype(np.float64) - yw64)
                worst_w = max(worst_w, float((err / bound).max()))
                assert (err <= bound).all(), f"{tag}: field {f} {'upper' if upper else 'lower'} window: v {v_cl[m][err > bound][:4]}, error {err[err > bound][:4]}, bound {bound[err > bound][:4]}"
                ref_err = np.abs(y32[m].astype(np.float64) - yw64)
                assert (e_m <= ref_err).all(), f"{tag}: the series does worse than the f32 chain it replaces: {e_m[e_m > ref_err][:4]} > {ref_err[e_m > ref_err][:4]}"
                in_win |= m
                n_win += int(m.sum())
        out = ~in_win
        if f < 2 and eps is None and not np.isfinite(ds[14]):
            # v = 1 exactly without an upper bound: Z + cdf_lower is within one rounding of 1, and which side it falls on differs
            # between the f32 chain (+inf if it reaches 1) and the kernel, whose argument is a = fma(v, 2 Z, 2 cdf_lower - 1) rounded
            # once.  A deviation from the f32 chain's class, pinned exactly: +inf if a == 1, else mu + sigma sqrt2 erfinv(a) within
            # erfinv_fast's pinned error (and a > 1 cannot happen).
            at_one = out & (v_cl == np.float32(1.0))
            assert at_one.any()
            a = np.float32(np.float64(ds[3]) + np.float64(ds[4]))
            assert a <= 1.0
            if a == 1.0:
                assert np.isposinf(y[at_one]).all(), f"{tag}: field {f} at v = 1: {y[at_one][:4]}, not +inf"
            else:
                e = float(sps.erfinv(np.float64(a)))
                want = float(ds[1]) + float(ds[2]) * e
                lim = dm.ulp32(want) + float(ds[2]) * ERFINV_MAX_ULP * dm.ulp32(e)
                assert (np.abs(y[at_one].astype(np.float64) - want) <= lim).all(), f"{tag}: field {f} at v = 1: {y[at_one][:4]} against {want!r}"
            out &= ~at_one
        ok, ratio = dm.within(y[out], y64[out], y32[out])
        worst_o = max(worst_o, float(ratio.max()))
        assert ok.all(), f"{tag}: field {f} outside a window: v {v[out][~ok][:4]}, got {y[out][~ok][:4]}, f64 {y64[out][~ok][:4]}, f32 chain {y32[out][~ok][:4]}"
    return n_win, worst_w, worst_o


def _edge_rows(ref32, ref64):
    """rows with v = 1 exactly on a truncated normal without an upper bound (eps=None).  The map's argument Z v + cdf_lower sits within
    one rounding of 1 there: (inf_rows) both reference chains map the row's bond or angle to +inf, or (edge_rows) only one of them
    does -- the f32 chain rounds to 1, the f64 chain on the same f32 parameters falls short of it, or the other way round.
    -> (inf_rows, edge_rows, angle_rows: the infinite value is an angle, not a bond)"""
    inf32, inf64 = (np.any([(~np.isfinite(y)).any(-1) for y in ys], axis=0) for ys in (ref32, ref64))
    assert not np.any([np.isneginf(y).any() for y in list(ref32) + list(ref64)])
    assert np.isfinite(ref32[2]).all() and np.isfinite(ref32[3]).all() and np.isfinite(ref64[2]).all() and np.isfinite(ref64[3]).all()
    angle = (~np.isfinite(ref32[1])).any(-1) | (~np.isfinite(ref64[1])).any(-1)
    # (the f32 chain's own Z + cdf_lower may even round beyond 1: its y is then NaN, not +inf)
    beyond = np.any([np.isnan(y).any(-1) for y in list(ref32) + list(ref64)], axis=0)
    return inf32 & inf64, inf32 != inf64, angle, beyond


def _check_edge_rows(tag, edges, x, dlogp, x64, dl64, x_bound):
    """what the kernels give in the rows of _edge_rows, pinned exactly.
    inf_rows with an infinite ANGLE: the log-det is NaN (sin of an infinite angle), as in the f32 chain.
    inf_rows with an infinite BOND: the log-det is +inf where the reference gives NaN -- a DEVIATION from the f32 chain's class.  The
      channel's own -log_prob is +inf; the reference's explicit 3 x 3 determinant then turns the infinite bond into inf - inf, the
      kernels' closed form ln|d (d sin a)| does not.  Coordinates: the atoms the chain keeps finite stay finite.
    edge_rows: the kernel's own argument -- fma(v, 2 Z, 2 cdf_lower - 1), rounded once, or the older kernel's f32 chain -- decides.
      Either the row is as in inf_rows, or every value is finite and agrees with the f64 chain within the bound of an ordinary row."""
    inf_rows, edge_rows, angle, beyond = edges
    for r in np.nonzero(inf_rows | edge_rows)[0]:
        if inf_rows[r] or not np.isfinite(dlogp[r]):
            if beyond[r]:       # a chain's argument rounds beyond 1 (y NaN); the kernel's own may or may not: NaN or the +inf of a == 1
                assert np.isnan(dlogp[r]) or (np.isposinf(dlogp[r]) and not angle[r]), f"{tag}: row {r}: log-det {dlogp[r]!r}"
            elif angle[r]:
                assert np.isnan(dlogp[r]), f"{tag}: row {r} (infinite angle): log-det {dlogp[r]!r}, not NaN"
            else:
                assert np.isposinf(dlogp[r]), f"{tag}: row {r} (infinite bond): log-det {dlogp[r]!r}, not +inf"
            if inf_rows[r]:
                keep = np.isfinite(x64[r])
                assert np.isfinite(x[r][keep]).all(), f"{tag}: row {r}: atoms the chain keeps finite are not"
            continue
        assert np.isfinite(x64[r]).all() and np.isfinite(x[r]).all(), f"{tag}: row {r}: a finite log-det with coordinates that are not"
        assert (np.abs(x[r] - x64[r]) <= x_bound[r]).all(), f"{tag}: row {r}: x off the f64 chain by {np.abs(x[r] - x64[r]).max():.2e}"
        # the log-det holds e^2 with e = erfinv(1 - 2^-24 ..): ERFINV_MAX_ULP of e, 2 e^2 ERFINV_MAX_ULP 2^-23 <= 32 * 3 * 2^-23 of it
        assert abs(dlogp[r] - dl64[r]) <= 2.0 ** -22 * abs(dl64[r]) + 96.0 * 2.0 ** -23, f"{tag}: row {r}: log-det {dlogp[r]!r} against {dl64[r]!r}"


@pytest.mark.parametrize("eps", [1e-7, None])
@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
def test_bound_windows_of_the_fused_tail(hip_lib, dev, ala2, alpha, beta, eps):
    """icdf_chan through the elementwise tail kernel (RelativeInternalCoordinateTransformation._icdf_ic2xyz_train returns the mapped
    fields): s = v k at {1e-4, 1e-3, 0.01, 0.0299, both f32 neighbours of the SMAX crossing, 0.031} at either bound of field-uniform
    truncated normals on the bonds and the angles; with eps=None also v exactly 0 and 1 (k = 1e30 as "no bound" entered the window
    there and returned y = 0)"""
    ic_dev, ic_cpu = ala2
    rel = ic_dev._rel_ic
    dists, vs = _tail_case(alpha, beta, eps, rel._n, 9)
    tab, _ = _tail_tables(dists, rel, dev)
    res = rel._icdf_ic2xyz_train(*[torch.as_tensor(v).to(dev) for v in vs], eps, ic_dev._wh("blacken", dev), tab)
    assert res is not None, "the elementwise tail kernel must have run"
    x, dlogp, ys = res
    ys = [y.cpu().numpy() for y in ys]
    ref64, x64, dl64, p64 = _tail_reference(ic_cpu, dists, vs, eps, torch.float64)
    ref32, x32, dl32, _ = _tail_reference(ic_cpu, dists, vs, eps, torch.float32)
    tag = f"alpha {alpha} beta {beta} eps {eps}"
    n_win, worst_w, worst_o = _check_fields(dists, vs, ys, eps, ref64, ref32, tag)
    assert n_win >= 60, "the inputs must enter the windows"
    dlogp = dlogp.cpu().numpy()
    edges = _edge_rows(ref32, ref64)
    inf_rows, edge_rows = edges[0], edges[1]
    ordinary = ~(inf_rows | edge_rows)
    okl, ratio_l = dm.within(dlogp, dl64, dl32, floor=2.0 ** -22 * np.abs(dl64))           # per row, R the row's own
    print(f"{tag}: {n_win} window elements, worst error / bound {worst_w:.3f} inside, {worst_o:.3f} outside, {ratio_l[ordinary].max():.3f} log-det")
    assert okl[ordinary].all(), f"{tag}: log-det rows {np.nonzero(~okl & ordinary)[0][:6]}: got {dlogp[~okl & ordinary][:4]}, f64 {dl64[~okl & ordinary][:4]}, f32 chain {dl32[~okl & ordinary][:4]}"
    xk = x.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        x_bound = 4.0 * dm.ulp32(np.where(np.isfinite(x64), x64, 1.0)) + _frame_floor(ic_cpu, [np.where(np.isfinite(y), y, 1.0) for y in ref64]) + 2e-6
    _check_edge_rows(tag, edges, xk, dlogp, x64, dl64, x_bound)


def test_v_zero_without_a_lower_bound_through_the_fused_tail(hip_lib, dev, ala2):
    """the kernel side of the "no bound" sentinel: a truncated normal whose lower bound has the cdf value 0 (beyond 5.4 sigma in f32, or
    loaded that way) has k = inf in its tail descriptor.  v = 0 exactly with eps=None must then give the f32 chain's y = -inf; with the
    finite sentinel 1e30 the kernel entered the lower window (0 * 1e30 < 0.03) and returned y = y0 = 0 with a finite log-det."""
    from bgflow_amd.cdf import _tail_descriptor
    ic_dev, ic_cpu = ala2
    rel = ic_dev._rel_ic
    n, keep = rel._n, 9
    dists, _ = _tail_case(-3.0, 2.0, 1e-7, n, keep)
    dists[0]._cdf_lower_bound.fill_(0.0)
    ds = _tail_descriptor(dists[0], n).numpy()
    assert np.isposinf(ds[:, 7]).all() and np.isfinite(ds[:, 14]).all() and not ds[:, 8:13].any()
    rs = np.random.RandomState(3)
    vs = [(0.2 + 0.6 * rs.rand(B_TAIL, w)).astype(np.float32) for w in (n, n, n, keep)]
    zero_rows = np.arange(0, B_TAIL, 5)
    vs[0][zero_rows, zero_rows % n] = 0.0
    tab, _ = _tail_tables(dists, rel, dev)
    res = rel._icdf_ic2xyz_train(*[torch.as_tensor(v).to(dev) for v in vs], None, ic_dev._wh("blacken", dev), tab)
    assert res is not None, "the elementwise tail kernel must have run"
    _, dlogp, ys = res
    ys, dlogp = [y.cpu().numpy() for y in ys], dlogp.cpu().numpy()
    ref64, _, dl64, p64 = _tail_reference(ic_cpu, dists, vs, None, torch.float64)
    ref32, _, dl32, _ = _tail_reference(ic_cpu, dists, vs, None, torch.float32)
    at_zero = vs[0] == 0.0
    assert at_zero.sum() == len(zero_rows) and np.isneginf(ref32[0][at_zero]).all() and np.isneginf(ref64[0][at_zero]).all()
    for f in range(4):
        ok, _ = dm.within(ys[f], ref64[f], ref32[f])                   # per element; -inf exactly where the chain has it
        assert ok.all(), f"field {f}: {ys[f][~ok][:4]} against {ref64[f][~ok][:4]}"
    assert np.isneginf(ys[0][at_zero]).all() and np.isfinite(ys[0][~at_zero]).all()
    rows = at_zero.any(-1)
    # the log-det of such a row: +inf (the bond's own -log_prob); the reference's determinant makes NaN of the infinite bond
    assert np.isposinf(dlogp[rows]).all() and np.isnan(dl32[rows]).all()
    okl, _ = dm.within(dlogp[~rows], dl64[~rows], dl32[~rows], floor=2.0 ** -22 * np.abs(dl64[~rows]))
    assert okl.all()


def _frame_floor(ic_cpu, ys64):
    """what the f32 rounding of the fixed atoms alone costs every coordinate, per element [B, 66]: sum over the 15 fixed coordinates c
    of |dx / dxfix_c| * 4.5 ulp(xfix_c).  The kernels blacken by nine fmas onto the mean (1.4 .. 1.7 here), each rounding at the
    coordinate's magnitude: up to nine half ulps, where the reference adds the mean once.  The five fixed atoms sit 0.1 .. 0.25 apart and
    carry bonds of 0.5 .. 1: the frame they span turns that rounding into a rotation of everything placed on it (lever / baseline ~ 10).
    The sensitivities are central differences of the f64 chain."""
    from oracle.torch_flow import ic2xyz_torch
    ic64 = _ic64(ic_cpu)
    w = ic64._whiten
    b, a, t, zf = [torch.as_tensor(np.asarray(y, np.float64)) for y in ys64]
    with torch.no_grad():
        xf = zf @ w.Tblacken + w.X0mean
        floor = np.zeros((b.shape[0], 3 * (b.shape[1] + xf.shape[1] // 3)))
        h = 1e-6
        for c in range(xf.shape[1]):
            d = torch.zeros_like(xf)
            d[:, c] = h
            xp, _ = ic2xyz_torch(ic64._rel_ic, b, a, t, xf + d)
            xm, _ = ic2xyz_torch(ic64._rel_ic, b, a, t, xf - d)
            floor += np.abs(((xp - xm) / (2 * h)).numpy()) * 4.5 * dm.ulp32(xf[:, c].numpy())[:, None]
    return floor


@pytest.mark.parametrize("variant", ["register", "lds_table"])
@pytest.mark.parametrize("eps", [1e-7, None])
@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
def test_bound_windows_through_the_other_tail_kernels(hip_lib, dev, ala2, alpha, beta, eps, variant):
    """rows like those of the test above through bgk_icdf_ic2xyz_reg (REGISTER_TAIL on, UNIFORM_TAIL off) and the older bgk_icdf_ic2xyz
    (OCML erfinv), with marginals that differ from channel to channel (sigma grows by 2 % per channel, so a descriptor row that
    reaches the wrong channel of its field shows): x and dlogp against the f64 chain, every row and every coordinate.

    x: |x - x64| <= 4 R + 4 ulp(x64) + F.  R is the f32 chain's worst coordinate of the element's own row (with R at the element alone
    the bound is missed by a factor of up to 55: a coordinate collects the roundings of up to 17 sequential placements, and the chain
    rounds exactly at some).  F is _frame_floor: measured on an MI355X both kernels are 2e-6 .. 5e-6 off where the f32 chain's row
    maximum is 5e-7, in every row alike -- without F the worst error / bound of a case is 0.8 .. 2.7 (printed),
    with it at most 0.35; F's median is 4e-6 .. 1e-5 against a median 4 R of 2e-6 .. 3e-5.
    dlogp: 4 R + 2^-22 P with R over the rows that give the same special input to the same field and P the sum of the magnitudes of
    the row's terms (_tail_reference): these two kernels add some 80 terms onto the constant 50.7 one by one."""
    from bgflow_amd import _lib
    ic_dev, ic_cpu = ala2
    rel = ic_dev._rel_ic
    dists, vs = _tail_case(alpha, beta, eps, rel._n, 9, spread=0.02)
    tab, descs = _tail_tables(dists, rel, dev)
    assert tab.uniform4 is None, "the marginals must differ inside a field"
    cls = type(rel)
    saved = (cls.UNIFORM_TAIL, cls.REGISTER_TAIL)
    lib = _lib.lib()
    entry = "bgk_icdf_ic2xyz_reg" if variant == "register" else "bgk_icdf_ic2xyz"
    orig, calls = getattr(lib, entry), []

    def spy(*args):
        calls.append(orig(*args))
        return calls[-1]
    try:
        setattr(lib, entry, spy)
        cls.UNIFORM_TAIL, cls.REGISTER_TAIL = False, variant == "register"
        with torch.no_grad():
            x, dlogp = ic_dev._generate_fused(*[torch.as_tensor(v).to(dev) for v in vs], descs, eps, desc20=tab)
    finally:
        setattr(lib, entry, orig)
        cls.UNIFORM_TAIL, cls.REGISTER_TAIL = saved
    assert calls == [0], f"{entry} must have run, once and without an error: {calls}"
    x, dlogp = x.cpu().numpy(), dlogp.cpu().numpy().reshape(-1)
    ref64, x64, dl64, p64 = _tail_reference(ic_cpu, dists, vs, eps, torch.float64)
    ref32, x32, dl32, _ = _tail_reference(ic_cpu, dists, vs, eps, torch.float32)
    tag = f"{variant} alpha {alpha} beta {beta} eps {eps}"
    rows = np.arange(B_TAIL)
    # rows with v = 1 exactly and no upper bound: see _edge_rows
    edges = _edge_rows(ref32, ref64)
    inf_rows, edge_rows = edges[0], edges[1]
    with np.errstate(invalid="ignore", over="ignore"):
        frame = _frame_floor(ic_cpu, [np.where(np.isfinite(y), y, 1.0) for y in ref64])
        floor_x = 4.0 * dm.ulp32(np.where(np.isfinite(x64), x64, 1.0)) + frame
    row_grp = np.broadcast_to(rows[:, None], x.shape)
    okx, ratio_x = dm.within(x, x64, x32, floor=floor_x, groups=row_grp)
    okl, ratio_l = dm.within(dlogp, dl64, dl32, floor=2.0 ** -22 * p64, groups=_point_groups(dists, eps, rel._n))
    ordinary = ~(inf_rows | edge_rows)
    with np.errstate(invalid="ignore"):
        dx32, dxk = np.abs(x32 - x64), np.abs(x - x64)
    r_row = dm.group_max(np.where(np.isfinite(dx32), dx32, np.nan), row_grp)
    # the inputs keep the reference's own f32 chain well conditioned in every ordinary row (no IC clamp fires: all other channels in (0.2, 0.8))
    assert np.isfinite(x32[ordinary]).all() and np.isfinite(dl32[ordinary]).all() and dx32[ordinary].max() <= 1e-4
    print(f"{tag}: worst error / bound {ratio_x[ordinary].max():.3f} x, {ratio_l[ordinary].max():.3f} log-det; without the frame term "
          f"{dm.within(x, x64, x32, groups=row_grp)[1][ordinary].max():.3f}, with R at the element alone {dm.within(x, x64, x32)[1][ordinary].max():.3f} x, "
          f"{dm.within(dlogp, dl64, dl32, floor=2.0 ** -22 * p64)[1][ordinary].max():.3f} log-det; median frame term {np.median(frame[ordinary]):.2e} "
          f"against median 4 R {4 * np.median(r_row[ordinary]):.2e}; max |x error| {dxk[ordinary].max():.2e}, the f32 chain's {dx32[ordinary].max():.2e}")
    assert okx[ordinary].all(), f"{tag}: x rows {np.unique(np.nonzero(~okx & ordinary[:, None])[0])[:6]}"
    assert okl[ordinary].all(), f"{tag}: log-det rows {np.nonzero(~okl & ordinary)[0][:6]}: got {dlogp[~okl & ordinary][:4]}, f64 {dl64[~okl & ordinary][:4]}, f32 chain {dl32[~okl & ordinary][:4]}"
    _check_edge_rows(tag, edges, x, dlogp, x64, dl64, floor_x + 4.0 * r_row)


# ---- (g) the inference head ---------------------------------------------------------------------------------------------------
B_HEAD = 132           # two tiles and four rows; a multiple of 4, so that the [B, 17] output tiles are 16-byte aligned (the head's envelope)
ANGLES = [1e-4, 1e-2, *dm.neighbours(np.pi / 8)[::2], np.pi / 4, *dm.neighbours(np.pi / 2)[::2], np.pi - 1e-3]          # radians
TORSIONS = [0.3, 2.0, -2.0, -0.3, np.pi / 2, -np.pi / 2, 0.0, float(dm.neighbours(np.pi)[0]), -float(dm.neighbours(np.pi)[0])]


def _leaf_rows(rel):
    """Z rows whose atom no other row builds on: a near-straight or near-zero angle there makes no later placement singular"""
    z = np.asarray(rel._z_matrix)
    used = set(z[:, 1:].reshape(-1).tolist())
    return [i for i in range(len(z)) if int(z[i, 0]) not in used]


def _molecules(ic_cpu, bonds, angles_n, torsions_n, zfix):
    """f32 coordinates [B, 66] built in f64 from IC values (normalised angles / torsions, whitened fixed coordinates)"""
    from oracle.torch_flow import ic2xyz_torch
    with torch.no_grad():
        x, _ = ic2xyz_torch(_ic64(ic_cpu), *[torch.as_tensor(np.asarray(v, np.float64)) for v in (bonds, angles_n, torsions_n, zfix)])
    return np.ascontiguousarray(x.numpy().astype(np.float32))


def _head_reference(ic_cpu, x32, dists, eps, dtype):
    """the NLL direction of the tail as the reference runs it, in ``dtype`` on the CPU, from the f32 coordinates the kernel receives:
    xyz -> IC + whitening (the oracle's restatement of the reference's op chain), then the cdf maps (``dists[f]`` None: none)
    -> (four fields, dlogp [B])"""
    from oracle import flow_oracle as fo
    npd = np.float64 if dtype == torch.float64 else np.float32
    *fields, dl = fo.ic_block(ic_cpu, [x32.astype(npd)], False, npd)
    dl = np.asarray(dl, npd).reshape(-1)
    out = []
    with torch.no_grad():
        for v, dist in zip(fields, dists):
            if dist is None:
                out.append(np.asarray(v, npd))
                continue
            y, l = dm.chain(dist, torch.as_tensor(np.asarray(v, npd)), False, eps, dtype)
            out.append(y.numpy())
            dl = dl + l.sum(-1).numpy()
    return out, dl


def _desc4(dists, n, keep, dev):
    from bgflow_amd.cdf import TAIL_DESC, _tail_descriptor
    rows = []
    for dist, w in zip(dists, (n, n, n, keep)):
        if dist is None:
            t = torch.zeros(1, TAIL_DESC)
            t[:, 0] = torch.tensor(-1, dtype=torch.int32).view(torch.float32)
        else:
            t = _tail_descriptor(dist, w)[:1]
        rows.append(t)
    return torch.cat(rows, dim=0).contiguous().to(dev)


def _row_groups(special):
    """group ids [B, w]: a special element keeps its id (the elements with the same special value), an ordinary one (id 0) gets its
    row's"""
    rows = np.arange(special.shape[0])[:, None]
    return np.where(special > 0, special, 64 + rows)


def _wrapped(got, ref):
    """got moved by a whole turn where that brings a normalised torsion closer to ref (0 and 1 are the same angle)"""
    got = np.asarray(got, np.float64)
    return got - np.round(got - np.asarray(ref, np.float64))


def test_inference_head_angles_and_torsions_without_maps(hip_lib, dev, ala2):
    """atan2_fast of bgk_xyz2ic_cdf_uni, observed through fields with no map (kind -1): angles at {1e-4, 1e-2, pi/8 -+ ulp, pi/4,
    pi/2 -+ ulp, pi - 1e-3} and torsions in all four quadrants, on the axes and at +-(pi - ulp); every molecule is built in f64 from
    its IC values, and the f64 reference recomputes the ICs from the f32 coordinates the kernel receives.  R of the bound: the f32
    chain's worst element among those with the same special value; for an ordinary element, the worst ordinary element of the same
    field in its own row (with R at the element alone the bound is missed by factors of up to 14 on the torsions and 6 on the fixed
    coordinates, where the chain rounds exactly)."""
    ic_dev, ic_cpu = ala2
    rel = ic_dev._rel_ic
    n, keep = rel._n, 9
    rs = np.random.RandomState(11)
    bonds = 0.4 + 0.4 * rs.rand(B_HEAD, n)
    angles = 0.25 + 0.5 * rs.rand(B_HEAD, n)
    torsions = 0.05 + 0.9 * rs.rand(B_HEAD, n)
    zfix = rs.randn(B_HEAD, keep)
    leaves = _leaf_rows(rel)
    assert len(leaves) >= 4
    groups = [np.zeros((B_HEAD, n), np.int64) for _ in range(3)]
    for r in range(B_HEAD):
        ka, kt = r % len(ANGLES), r % len(TORSIONS)
        ca, ct = leaves[(r // len(ANGLES)) % len(leaves)], (r // 3) % n
        angles[r, ca] = float(ANGLES[ka]) / np.pi
        torsions[r, ct] = (float(TORSIONS[kt]) + np.pi) / (2.0 * np.pi)
        groups[1][r, ca], groups[2][r, ct] = 1 + ka, 1 + kt
    x32 = _molecules(ic_cpu, bonds, angles, torsions, zfix)
    res = ic_dev._infer_fused(torch.as_tensor(x32).to(dev), _desc4([None] * 4, n, keep, dev), 1e-7)
    assert res is not None, "the fused inference head must have run"
    got = [v.cpu().numpy() for v in res[:4]]
    dl = res[4].cpu().numpy().reshape(-1)
    ref64, dl64 = _head_reference(ic_cpu, x32, [None] * 4, 1e-7, torch.float64)
    ref32, dl32 = _head_reference(ic_cpu, x32, [None] * 4, 1e-7, torch.float32)
    # the inputs reach what they are meant to reach
    a64 = ref64[1] * np.pi
    assert np.abs(a64[groups[1] == 3] - np.pi / 8).max() < 1e-6 and np.abs(a64[groups[1] == 6] - np.pi / 2).max() < 1e-6
    assert a64.min() < 5e-4 and a64.max() > np.pi - 2e-3
    t64 = ref64[2]
    assert t64.min() < 1e-6 or t64.max() > 1 - 1e-6
    misses = []
    for f, name in enumerate(("bonds", "angles", "torsions", "fixed")):
        g, r64, r32 = got[f], ref64[f], ref32[f]
        if f == 2:
            g, r32 = _wrapped(g, r64), _wrapped(r32, r64)
        grp = _row_groups(groups[f] if f < 3 else np.zeros(g.shape, np.int64))
        ok, ratio = dm.within(g, r64, r32, groups=grp)
        print(f"{name}: worst error / bound {ratio.max():.3f} ({dm.within(g, r64, r32)[1].max():.3f} with R taken at the element alone), "
              f"max |error| {np.abs(g - r64).max():.3e}, the f32 chain's {np.abs(r32 - r64).max():.3e}")
        for i, j in np.argwhere(~ok)[:6]:
            misses.append(f"{name}[{i},{j}] (group {grp[i, j]}): got {got[f][i, j]!r} f64 {r64[i, j]!r} f32 chain {ref32[f][i, j]!r} error/bound {ratio[i, j]:.2f}")
    okl, ratio_l = dm.within(dl, dl64, dl32, floor=2.0 ** -22 * np.abs(dl64), groups=np.arange(B_HEAD) % len(ANGLES))
    print(f"log-det: worst error / bound {ratio_l.max():.3f}")
    for i in np.nonzero(~okl)[0][:6]:
        misses.append(f"log-det[{i}]: got {dl[i]!r} f64 {dl64[i]!r} f32 chain {dl32[i]!r} error/bound {ratio_l[i]:.2f}")
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("eps", [1e-7, 1e-3])
@pytest.mark.parametrize("alpha,beta", [(-3.0, 2.0), (-1.0, 0.75), (0.0, 2.0)])
def test_inference_head_cdf_next_to_a_bound(hip_lib, dev, ala2, alpha, beta, eps):
    """cdf_chan of bgk_xyz2ic_cdf_uni: bonds and angles at {1e-6, 1e-4, 1e-2} sigma inside either bound of a truncated normal, and
    beyond the bounds by 1e-2 sigma, where the map clamps to [eps, 1 - eps]"""
    ic_dev, ic_cpu = ala2
    rel = ic_dev._rel_ic
    n, keep = rel._n, 9
    dists = [dm.truncated_normal(alpha, beta, n, lower=0.5, sigma=0.1, spread=0.0), dm.truncated_normal(alpha, beta, n, lower=0.3, sigma=0.05, spread=0.0),
             dm.uniform(0.0, 1.0, n, spread=0.0), dm.normal(0.0, 1.0, keep, spread=0.0)]
    rs = np.random.RandomState(int(10 * abs(alpha) + 4 * beta))
    with torch.no_grad():
        u0 = [torch.as_tensor(0.2 + 0.6 * rs.rand(B_HEAD, w)) for w in (n, n, n, keep)]
        fields = [dm.chain(d_, u, True, None, torch.float64)[0].numpy() for d_, u in zip(dists, u0)]
    groups = [np.zeros((B_HEAD, n), np.int64) for _ in range(2)]
    deltas = [1e-6, 1e-4, 1e-2, -1e-2]                  # in sigmas, inside the bound (negative: beyond it)
    for r in range(B_HEAD):
        f, q = r % 2, r // 2
        _, p = dm.params(dists[f], torch.float64)
        mu, sigma = float(p["mu"][0]), float(p["sigma"][0])
        k, upper, ch = q % len(deltas), (q // len(deltas)) % 2, q % n
        bound = mu + (beta if upper else alpha) * sigma
        fields[f][r, ch] = bound + (-1.0 if upper else 1.0) * deltas[k] * sigma
        groups[f][r, ch] = 1 + k + len(deltas) * upper
    x32 = _molecules(ic_cpu, *fields)
    res = ic_dev._infer_fused(torch.as_tensor(x32).to(dev), _desc4(dists, n, keep, dev), eps)
    assert res is not None, "the fused inference head must have run"
    got = [v.cpu().numpy() for v in res[:4]]
    dl = res[4].cpu().numpy().reshape(-1)
    ref64, dl64 = _head_reference(ic_cpu, x32, dists, eps, torch.float64)
    ref32, dl32 = _head_reference(ic_cpu, x32, dists, eps, torch.float32)
    lo, hi = np.float32(eps), np.float32(1.0) - np.float32(eps)
    misses = []
    for f, name in enumerate(("bonds", "angles", "torsions", "fixed")):
        g, r64, r32 = got[f], ref64[f], ref32[f]
        if f == 2:
            g, r32 = _wrapped(g, r64), _wrapped(r32, r64)
        grp = _row_groups(groups[f] if f < 2 else np.zeros(g.shape, np.int64))       # R: as in the test above
        ok, ratio = dm.within(g, r64, r32, groups=grp)
        print(f"alpha {alpha} beta {beta} eps {eps} {name}: worst error / bound {ratio.max():.3f}")
        for i, j in np.argwhere(~ok)[:6]:
            misses.append(f"{name}[{i},{j}] (group {grp[i, j]}): got {got[f][i, j]!r} f64 {r64[i, j]!r} f32 chain {ref32[f][i, j]!r} error/bound {ratio[i, j]:.2f}")
        if f < 2:
            beyond_lo, beyond_hi = groups[f] == 4, groups[f] == 8
            assert beyond_lo.any() and beyond_hi.any()
            assert (got[f][beyond_lo] == lo).all() and (got[f][beyond_hi] == hi).all(), "beyond a bound the map clamps to [eps, 1 - eps]"
            assert (got[f] >= lo).all() and (got[f] <= hi).all()
    okl, ratio_l = dm.within(dl, dl64, dl32, floor=2.0 ** -22 * np.abs(dl64), groups=(np.arange(B_HEAD) // 2) % (2 * len(deltas)))
    print(f"alpha {alpha} beta {beta} eps {eps} log-det: worst error / bound {ratio_l.max():.3f}")
    for i in np.nonzero(~okl)[0][:6]:
        misses.append(f"log-det[{i}]: got {dl[i]!r} f64 {dl64[i]!r} f32 chain {dl32[i]!r} error/bound {ratio_l[i]:.2f}")
    assert not misses, "\n".join(misses)
