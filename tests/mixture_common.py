"""Inputs of the mixture tests, regenerated from seeds (tests/golden/mixture.npz stores their checksums and the reference's OUTPUTS),
and the comparisons the host and the GPU tests share.  The recipe (make_mixture_goldens.py builds the reference's mixture from the same
arrays):

  means 3 N(0, 1) [K, d];  every second component (odd k) a diagonal covariance with variances in [0.2, 2.2];  unnormalised
  log-weights N(0, 1), for K > 2 the one of component 1 is -inf;  B = 150 rows 4 N(0, 1), row 3 = +1e4 and row 4 = -1e3 in every
  column;  a [150]: the weights of the scalar sum_b a_b u_b whose gradients are compared, uniform in [0.5, 1.5]

from ``numpy.random.RandomState`` (the legacy generator: its stream is frozen), all rounded to f32 once.
"""
import numpy as np

B = 150
FAR = np.array([3, 4])                                 # the rows far from every mean
BULK = np.setdiff1d(np.arange(B), FAR)
CASES = [(1, 1), (2, 3), (7, 5), (40, 2), (64, 66), (5, 97), (3, 128)]
SEED = 20271
SAMPLE_CASE, SAMPLE_SEED, SAMPLE_N = (7, 5), 3, 100


def key(K, d):
    return f"k{K}_d{d}_"


def inputs(K, d):
    """dict of f32 arrays: mean [K, d], var [K, d] (used for odd k), logw [K], x [150, d], a [150]"""
    rng = np.random.RandomState(SEED + 1000 * K + d)
    mean = (3.0 * rng.standard_normal((K, d))).astype(np.float32)
    var = (0.2 + 2.0 * rng.random_sample((K, d))).astype(np.float32)
    logw = rng.standard_normal(K).astype(np.float32)
    if K > 2:
        logw[1] = -np.inf
    x = (4.0 * rng.standard_normal((B, d))).astype(np.float32)
    x[3], x[4] = 1e4, -1e3
    a = (0.5 + rng.random_sample(B)).astype(np.float32)
    return {"mean": mean, "var": var, "logw": logw, "x": x, "a": a}


def checksum(inp):
    """what the fixture stores of the inputs: the f64 sum of every array's finite entries and its largest finite magnitude"""
    out = []
    for name in ("mean", "var", "logw", "x", "a"):
        v = inp[name].astype(np.float64).ravel()
        v = v[np.isfinite(v)]
        out += [v.sum(), np.abs(v).max()]
    return np.array(out)


def build(module, K, d, dtype, trainable_weights=True, **kwargs):
    """the mixture of the case from the classes of ``module`` (this package or the reference): NormalDistribution components, odd k with
    the diagonal covariance"""
    import torch
    inp = inputs(K, d)
    comps = []
    for k in range(K):
        mean = torch.from_numpy(inp["mean"][k]).to(dtype)
        cov = torch.diag(torch.from_numpy(inp["var"][k]).to(dtype)) if k % 2 == 1 else None
        comps.append(module.NormalDistribution(d, mean, cov))
    return module.MixtureDistribution(comps, torch.from_numpy(inp["logw"]).to(dtype).clone(), trainable_weights=trainable_weights, **kwargs)


def evaluate(mix, x, a, temperature=1.0):
    """(u [B], g_x [B, d], neg_e [B, K], g_w bulk [K], g_w far [K]) of a mixture with trainable weights as numpy arrays, u the energy at
    ``temperature``: the gradients are those of sum_b a_b u_b; the weight gradient is taken separately over the bulk rows and over the
    far rows"""
    import torch
    x = x.detach().clone().requires_grad_(True)
    u = mix.energy(x, temperature=temperature)
    gx, = torch.autograd.grad((a * u[:, 0]).sum(), x, retain_graph=True)
    mask = torch.zeros_like(a)
    mask[torch.as_tensor(FAR, device=a.device)] = 1.0
    gw_far, = torch.autograd.grad((a * mask * u[:, 0]).sum(), mix._unnormed_log_weights, retain_graph=True)
    gw_bulk, = torch.autograd.grad((a * (1.0 - mask) * u[:, 0]).sum(), mix._unnormed_log_weights)
    with torch.no_grad():
        neg_e = mix._log_assignments(x.detach())
    assert u.shape == (x.shape[0], 1) and neg_e.shape == (x.shape[0], 1, len(mix._components))
    return tuple(t.detach().cpu().numpy() for t in (u[:, 0], gx, neg_e[:, 0], gw_bulk, gw_far))


def rel_err(v, v64):
    """max |v - v64| / (1 + |v64|)"""
    v, v64 = np.asarray(v, np.float64), np.asarray(v64, np.float64)
    if v.size == 0:
        return 0.0
    return float(np.max(np.abs(v - v64) / (1.0 + np.abs(v64))))


def split_errors(u, gx, neg_e, gw_bulk, gw_far, G, k, temperature=1.0):
    """{name: (error over the bulk rows, error over the far rows)} against the f64 arrays of fixture ``G`` under key prefix ``k``; at a
    ``temperature`` the energy and its gradients are the fixture's divided by it (energy/base.py:124-146), the log-assignments unchanged"""
    out = {}
    for name, v, ref in (("u", u, G[k + "u64"] / temperature), ("g", gx, G[k + "g64"] / temperature), ("e", neg_e, G[k + "neg_e64"])):
        out[name] = (rel_err(v[BULK], ref[BULK]), rel_err(v[FAR], ref[FAR]))
    out["w"] = (rel_err(gw_bulk, G[k + "gw64_bulk"] / temperature), rel_err(gw_far, G[k + "gw64_far"] / temperature))
    return out


def assert_within(errs, G, k, factor=4.0, floor=1e-6, what=""):
    """every error within factor * (the reference's own f32 error on the same rows) + floor"""
    for name, (bulk, far) in errs.items():
        for part, err in (("bulk", bulk), ("far", far)):
            bound = factor * float(G[f"{k}err_{name}32_{part}"]) + floor
            print(f"{what}{k}{name} {part}: error {err:.3g}, bound {bound:.3g}")
            assert np.isfinite(err) and err <= bound, (what, k, name, part, err, bound)
