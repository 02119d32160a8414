"""Helpers of tests/test_gpu_domain_maps.py and tests/test_host_domain_maps.py: f64 references of the CDF / ICDF domain maps, the
reference's own f32 torch op chain, the error bounds, and the input builders.  Nothing here touches the GPU.

The f64 reference is the SAME formula chain evaluated in f64 on the SAME inputs: the marginal's parameters are the values the f32
module holds and hands to the kernels in its descriptor (mu, sigma = exp(logsigma), the cdf value of the lower bound and Z = cdf_upper
- cdf_lower, all as f32 and then widened): they are the layer's state.  Only the arithmetic on them is done in f64.  (Re-deriving the
cdf values of the bounds in f64 would describe another layer: the f32 cdf of a bound three sigmas out is off by 1e-7 relative, which
moves the bound by 6e-5 sigma.)"""
import numpy as np
import torch
from scipy import special as sps

SQRT2 = float(np.sqrt(2.0))
HALF_LOG_2PI = 0.9189385332046727
SMAX = np.float32(0.03)          # csrc/bgk_tail.hip: the series window is entered when s = v k < SMAX (f32 compare)
ERF_SWITCH = 0.927734375         # csrc/bgk_erf.h: erf_fast's branch switch
ERFINV_SWITCH = float(np.sqrt(1.0 - np.exp(-5.0)))      # |x| at which erfinv_fast's w = -ln(1 - x^2) reaches 5


# ---- floats ------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float32)


def ulp32(x):
    """spacing of the f32 grid at |x| (x in f64): 2^(floor(log2 |x|) - 23), 2^-149 in the subnormal range and at 0"""
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.where(ax > 0, e, -126.0)
    return np.exp2(np.clip(e, -126.0, 127.0) - 23.0)


def ulp_error(got32, ref64):
    """|got - ref| in units of the f32 spacing at ref, for finite ref"""
    return np.abs(np.asarray(got32, np.float64) - ref64) / ulp32(ref64)


def neighbours(x):
    """(the f32 below x, f32(x), the f32 above x)"""
    x = np.float32(x)
    return np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


def binade_sweep(e_lo, e_hi, n_mant=256):
    """n_mant mantissas in every f32 binade with biased exponent field e_lo .. e_hi (field 0 = the subnormals), positive"""
    e = np.arange(e_lo, e_hi + 1, dtype=np.uint32)[:, None]
    m = (np.arange(n_mant, dtype=np.uint32) * np.uint32((1 << 23) // n_mant))[None, :]
    return from_bits(((e << np.uint32(23)) | m).reshape(-1))


def floats_between(lo, hi):
    """every f32 in [lo, hi] (0 < lo <= hi)"""
    a, b = int(bits([lo])[0]), int(bits([hi])[0])
    return from_bits(np.arange(a, b + 1, dtype=np.uint32))


def same_class(got, ref):
    """infinity sign and NaN-ness of got equal those of ref wherever ref is not finite; got finite wherever ref is"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nf = ~np.isfinite(ref)
    ok = np.isfinite(got) == np.isfinite(ref)
    ok &= np.isnan(got) == np.isnan(ref)
    ok &= np.where(nf & ~np.isnan(ref), np.sign(got) == np.sign(ref), True)
    return ok


def group_max(err, groups):
    """per element: the maximum of the finite entries of ``err`` over the element's group (``groups``: integer ids, same shape)"""
    err, groups = np.asarray(err, np.float64), np.asarray(groups)
    top = np.zeros(int(groups.max()) + 1 if groups.size else 1)
    fin = np.isfinite(err)
    np.maximum.at(top, groups[fin], err[fin])
    return top[groups]


def within(got, ref64, ref32, floor=None, groups=None, ref_err=None):
    """the suite's idiom (tests/test_gpu_particles.py: the kernel's error against four times the error of the reference's own f32
    chain plus a floor), with no element left out: |v - v64| <= 4 R + 4 ulp(v64) wherever both chains are finite (``floor`` replaces
    the ulp term: 2^-22 |v64| for row sums), and the f32 chain's infinity sign / NaN-ness wherever it is not finite.  R is the f32
    chain's error |v32_ref - v64| at the element itself, or -- with ``groups`` -- its maximum over the elements of the same group.
    A group is never wider than the elements that share the element's own input point, or its own row: the same conditioning, so
    that one element at which the f32 chain happens to round exactly does not turn the bound into 4 ulp where f32 arithmetic cannot
    deliver it, and no group lets ill-conditioned elements license ordinary ones.  ``ref_err``: R given directly.
    -> (ok mask, error / bound with 0 where a reference is not finite)"""
    got, ref64, ref32 = (np.asarray(v, np.float64) for v in (got, ref64, ref32))
    fin = np.isfinite(ref32) & np.isfinite(ref64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(ref32 - ref64) if ref_err is None else np.broadcast_to(np.asarray(ref_err, np.float64), got.shape)
        if groups is not None and ref_err is None:
            r = group_max(np.where(fin, r, np.nan), np.broadcast_to(groups, got.shape))
        bound = 4.0 * r + (4.0 * ulp32(ref64) if floor is None else floor)
        ratio = np.where(fin, np.abs(got - ref64) / np.where(fin & (bound > 0), bound, 1.0), 0.0)
        ratio = np.where(fin & (bound == 0) & (got == ref64), 0.0, ratio)
    ok = np.where(fin, ratio <= 1.0, same_class(got, ref32))
    return ok, ratio


# ---- marginals ---------------------------------------------------------------------------------------------------------------
def _cols(v, d, step):
    """d per-column values v (1 + step j): every column of a map gets its own parameters"""
    return torch.as_tensor(float(v) * (1.0 + step * np.arange(d)), dtype=torch.float32)


def truncated_normal(alpha, beta, d=1, lower=0.5, sigma=0.1, spread=0.05):
    """TruncatedNormalDistribution whose lower bound is alpha sigmas and whose upper bound is beta sigmas from the mean (alpha <= 0 <
    beta; beta may be inf), f32, on the CPU; sigma grows by ``spread`` per column"""
    import bgflow_amd as bg
    sig = _cols(sigma, d, spread)
    mu = float(lower) - float(alpha) * sig
    upper = mu + float(beta) * sig if np.isfinite(beta) else torch.full((d,), np.inf)
    return bg.TruncatedNormalDistribution(mu=mu, sigma=sig, lower_bound=torch.tensor(float(lower)), upper_bound=upper)


def normal(loc, scale, d=1, spread=0.05):
    from bgflow_amd import configs
    return configs._NormalMarginal(float(loc) + 2.0 * spread * torch.arange(d, dtype=torch.float32), _cols(scale, d, spread))


def uniform(low, high, d=1, tol=1e-5, spread=0.05):
    from bgflow_amd import configs
    return configs.SloppyUniform(low=float(low) - 0.2 * spread * torch.arange(d, dtype=torch.float32), high=_cols(high, d, 0.4 * spread), tol=tol)


def params(dist, dtype):
    """(kind, parameter tensors as ``dtype``) of a marginal, read from the f32 module (see the module docstring)"""
    name = type(dist).__name__
    c = lambda t: torch.as_tensor(t, dtype=torch.float32).detach().cpu().to(dtype)     # noqa: E731
    if name == "TruncatedNormalDistribution":
        return 2, dict(mu=c(dist._mu), sigma=c(torch.exp(dist._logsigma)), clo=c(dist._cdf_lower_bound),
                       Z=c(dist._cdf_upper_bound - dist._cdf_lower_bound))
    if name in ("_NormalMarginal", "Normal"):
        return 1, dict(mu=c(dist.loc), sigma=c(dist.scale))
    return 0, dict(low=c(dist.low), high=c(dist.high), tol=float(getattr(dist, "tol", 0.0)))


def chain(dist, x, inverse, eps, dtype):
    """CDFTransform._forward / _inverse as the reference evaluates it (nn/flow/cdf.py:28-46 over the distributions' own cdf / icdf /
    log_prob, torch.clamp for eps), in ``dtype`` on the CPU, differentiable.  x: tensor [B, d] (any float dtype; widened or
    narrowed to ``dtype`` first -- pass f32 values).  -> (y [B, d], PER-ELEMENT log-det [B, d])"""
    kind, p = params(dist, dtype)
    x = x.to(dtype)
    lo_c = hi_c = None
    if eps is not None:                       # the clamp bounds as f32 holds them: f32(eps) and 1 - f32(eps) rounded to f32
        e32 = np.float32(eps)
        lo_c, hi_c = float(e32), float(np.float32(1.0) - e32)
    std = torch.distributions.Normal(torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype), validate_args=False)
    if kind == 0:
        low, high = p["low"], p["high"]
        cdf = lambda v: ((v - low) / (high - low)).clamp(0, 1)                                   # noqa: E731
        icdf = lambda u: low + u * (high - low)                                                  # noqa: E731

        def logp(v):
            inside = (v >= low - p["tol"]) & (v <= high + p["tol"])
            return torch.where(inside, -torch.log(high - low).expand_as(v), torch.full_like(v, -np.inf))
    elif kind == 1:
        nd = torch.distributions.Normal(p["mu"], p["sigma"], validate_args=False)
        cdf, icdf, logp = nd.cdf, nd.icdf, nd.log_prob
    else:
        mu, sigma, clo, Z = p["mu"], p["sigma"], p["clo"], p["Z"]
        cdf = lambda v: (std.cdf((v - mu) / sigma) - clo) / Z                                    # noqa: E731
        icdf = lambda u: std.icdf(Z * u + clo) * sigma + mu                                      # noqa: E731
        logp = lambda v: std.log_prob((v - mu) / sigma) - torch.log(Z * sigma)                   # noqa: E731
    if not inverse:
        y = cdf(x)
        if eps is not None:
            y = y.clamp(lo_c, hi_c)
        ld = logp(x)
    else:
        if eps is not None:
            x = x.clamp(lo_c, hi_c)
        y = icdf(x)
        ld = -logp(y)
    if eps is not None:
        ld = ld.clamp_min(-1.0 / eps)
    return y, ld


def chain_np(dist, x32, inverse, eps):
    """(y64, ld64, y32, ld32) numpy arrays of ``chain`` in f64 and in f32 on the f32 inputs x32"""
    xt = torch.as_tensor(np.ascontiguousarray(x32, np.float32))
    with torch.no_grad():
        y64, l64 = chain(dist, xt, inverse, eps, torch.float64)
        y32, l32 = chain(dist, xt, inverse, eps, torch.float32)
    return y64.numpy(), l64.numpy(), y32.numpy(), l32.numpy()


def icdf_exact(dist, u64):
    """f64 icdf of a truncated normal / normal at f64 points that keeps its accuracy next to cdf values of 0 and 1 (scipy's ndtri),
    numpy"""
    kind, p = params(dist, torch.float64)
    u64 = np.asarray(u64, np.float64)
    if kind == 0:
        return p["low"].numpy() + u64 * (p["high"] - p["low"]).numpy()
    mu, sigma = p["mu"].numpy(), p["sigma"].numpy()
    if kind == 1:
        return mu + sigma * sps.ndtri(u64)
    return mu + sigma * sps.ndtri(p["Z"].numpy() * u64 + p["clo"].numpy())


def icdf_edge_inputs(eps):
    """the icdf inputs of one column (f32, ascending): 0, 2^-149, 2^-30, eps and its two f32 neighbours, 0.5, f32(1 - eps) and its
    neighbours, 1 - 2^-24 and 1; for eps=None the eps points are those of 1e-7"""
    e = 1e-7 if eps is None else eps
    hi = np.float32(1.0) - np.float32(e)
    pts = [0.0, 2.0 ** -149, 2.0 ** -30, *neighbours(e), 0.5, *neighbours(hi), 1.0 - 2.0 ** -24, 1.0]
    return np.unique(np.asarray(pts, np.float32))


def fill(points, B, d):
    """[B, d] f32: column j holds ``points`` cyclically, starting at its j-th element (every point meets every column once B >=
    len(points) + d)"""
    idx = (np.arange(B)[:, None] + np.arange(d)[None, :]) % len(points)
    return np.ascontiguousarray(np.asarray(points, np.float32)[idx])


# ---- the reverted series of the fused tail's bound windows -------------------------------------------------------------------
def series_h(alpha, s, terms=5):
    """h = s + c2 s^2 + ... + c5 s^5 in f64 (cdf._reverted_cdf_series): the distance from the bound alpha in sigmas at s = (cdf
    distance from the bound) / pdf(alpha)"""
    from bgflow_amd.cdf import _reverted_cdf_series
    c = (1.0,) + tuple(_reverted_cdf_series(alpha))
    s = np.asarray(s, np.float64)
    return sum(ck * s ** (k + 1) for k, ck in enumerate(c[:terms]))


def exact_h(alpha, s, dps=40):
    """the exact distance: Phi(alpha + h) - Phi(alpha) = s pdf(alpha) solved for h, by mpmath where it imports (any alpha),
    otherwise scipy's ndtri(ndtr(alpha) + s pdf) - alpha (good to ~1e-16 / pdf(alpha) absolute: for |alpha| <= 3 only)"""
    s = np.atleast_1d(np.asarray(s, np.float64))
    try:
        import mpmath as mp
    except ImportError:
        assert abs(alpha) <= 3.0, "without mpmath the exact inverse is only good for |alpha| <= 3"
        pdf = np.exp(-0.5 * alpha * alpha) / np.sqrt(2.0 * np.pi)
        return sps.ndtri(sps.ndtr(alpha) + s * pdf) - alpha
    out = np.empty(s.shape, np.float64)
    with mp.workdps(dps):
        a = mp.mpf(float(alpha))
        pdf = mp.npdf(a)
        for i, si in enumerate(s.ravel()):
            if si == 0.0:
                out.ravel()[i] = 0.0
                continue
            target = mp.mpf(float(si)) * pdf
            f = lambda h: (mp.erfc(-(a + h) / mp.sqrt(2)) - mp.erfc(-a / mp.sqrt(2))) / 2 - target      # noqa: E731
            h0 = mp.mpf(float(series_h(float(alpha), float(si))))
            out.ravel()[i] = float(mp.findroot(f, h0, tol=mp.mpf(10) ** (-(dps - 8))))
    return out
