"""Inputs of the circular bump-mixture tests, regenerated from seeds (tests/golden/circular.npz stores their checksums, the inverse
targets and the reference's OUTPUTS), and the comparisons the host and the GPU tests share.  The recipe, B = 100 rows, everything
rounded to f32 once, from ``numpy.random.RandomState`` (the legacy generator: its stream is frozen):

  mu_raw 3 N(0, 1), log_sigma 1.5 N(0, 1), log_weight 2 N(0, 1) [B, K, D];  log_eps 2 N(0, 1) - 3, y U[0, 1) [B, D];
  a [B, D], c [B] U[0.5, 1.5]: the weights of the scalar sum a out + sum c dlogp whose gradients are compared;
  t [B, D] U[0, 1): the inverse targets (row 0: 0, row 1: 1, row 5: linspace(0.01, 0.99, D))

and the special rows, overwritten in every column and component:

  0  y = 0                               1  y = 1                          2  mu_raw = 0, y = 0.5, log_sigma = 0 (y == mu == 0.5)
  3  log_sigma = 40                      4  log_sigma = 40, log_eps = -20  5  mu_raw = pi / 2, y = 0.5 (f32 mu == 1.0: the seam tie)
  6  mu_raw = -pi / 2, y = 0, log_sigma = 0                                7  log_sigma = 8, log_eps = -20 (staircase-like)
  8  log_sigma = -30 (sigma == 1 in f32)   9  log_weight[component 0] = -40   10  log_eps = 15

Row groups: UNYARDSTICKED = {3, 4, 5} (the reference's own f32 run is NaN or wrong there: compared with its f64 run under the BULK
bound), NARROW = {7}, TIES = {2, 6} (the reference's gradient with respect to y and mu is an artefact of abs'(0) = 0 there: compared
with central differences), BULK every other row.  The well-conditioned case WELL = (4, 3) of the inverse-gradient tests has no
special rows, log_eps >= -2 (the density is at least 0.1) and log_sigma <= 1.
"""
import numpy as np

B = 100
CASES = [(1, 1), (3, 2), (8, 5), (32, 3), (2, 66), (33, 2)]
ENVELOPE = [c for c in CASES if c[0] <= 32]
WELL = (4, 3)
SEED = 41017
UNYARDSTICKED = np.array([3, 4, 5])
NARROW = np.array([7])
TIES = np.array([2, 6])
BULK = np.setdiff1d(np.arange(B), np.concatenate([UNYARDSTICKED, NARROW, TIES]))
QUANTITIES = ("out", "dlogp", "g_y", "g_mu", "g_ls", "g_lw", "g_le")
NAMES = ("mu_raw", "log_sigma", "log_weight", "log_eps", "y", "a", "c", "t")
CD_H = 1e-6


def key(K, D, well=False):
    return f"{'well_' if well else ''}k{K}_d{D}_"


def inputs(K, D, well=False):
    """dict of f32 arrays: mu_raw, log_sigma, log_weight [B, K, D], log_eps, y, a, t [B, D], c [B]"""
    rng = np.random.RandomState(SEED + 1000 * K + D + (500000 if well else 0))
    f32 = np.float32
    v = {"mu_raw": (3.0 * rng.standard_normal((B, K, D))).astype(f32),
         "log_sigma": (1.5 * rng.standard_normal((B, K, D))).astype(f32),
         "log_weight": (2.0 * rng.standard_normal((B, K, D))).astype(f32),
         "log_eps": (2.0 * rng.standard_normal((B, D)) - 3.0).astype(f32),
         "y": rng.random_sample((B, D)).astype(f32),
         "a": (0.5 + rng.random_sample((B, D))).astype(f32),
         "c": (0.5 + rng.random_sample(B)).astype(f32),
         "t": rng.random_sample((B, D)).astype(f32)}
    if well:
        v["log_eps"] = np.maximum(v["log_eps"], f32(-2.0))
        v["log_sigma"] = np.minimum(v["log_sigma"], f32(1.0))
        return v
    v["y"][0], v["y"][1] = 0.0, 1.0
    v["mu_raw"][2], v["y"][2], v["log_sigma"][2] = 0.0, 0.5, 0.0
    v["log_sigma"][3] = 40.0
    v["log_sigma"][4], v["log_eps"][4] = 40.0, -20.0
    v["mu_raw"][5], v["y"][5] = f32(np.pi / 2), 0.5
    v["mu_raw"][6], v["y"][6], v["log_sigma"][6] = f32(-np.pi / 2), 0.0, 0.0
    v["log_sigma"][7], v["log_eps"][7] = 8.0, -20.0
    v["log_sigma"][8] = -30.0
    v["log_weight"][9, 0] = -40.0
    v["log_eps"][10] = 15.0
    v["t"][0], v["t"][1], v["t"][5] = 0.0, 1.0, np.linspace(0.01, 0.99, D).astype(f32)
    return v


def checksum(inp):
    """what the fixture stores of the inputs: the f64 sum of every array and its largest magnitude"""
    out = []
    for name in NAMES:
        v = inp[name].astype(np.float64).ravel()
        out += [v.sum(), np.abs(v).max()]
    return np.array(out)


def tensors(inp, dtype, device="cpu", rows=None):
    """the inputs as torch tensors of ``dtype`` in the order of NAMES, the three component parameters flattened to [B, K D]"""
    import torch
    out = []
    for name in NAMES:
        v = inp[name] if rows is None else inp[name][rows]
        out.append(torch.from_numpy(np.ascontiguousarray(v)).to(dtype).reshape(v.shape[0], -1).to(device) if name != "c"
                   else torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(device))
    return out


def evaluate(fn, inp, dtype, device="cpu", rows=None, grads=True):
    """(out, dlogp [B], g_y, g_mu, g_ls, g_lw, g_le) as numpy arrays, parameters and their gradients [B, K D]: ``fn(y, mu_raw,
    log_sigma, log_weight, log_eps) -> (out, dlogp [B, 1])``, the gradients those of sum a out + sum c dlogp"""
    import torch
    mr, ls, lw, le, y, a, c, _ = tensors(inp, dtype, device, rows)
    leaves = [t.requires_grad_(grads) for t in (y, mr, ls, lw, le)]
    out, dlogp = fn(*leaves)
    assert out.shape == y.shape and dlogp.shape == (y.shape[0], 1)
    res = [out, dlogp[:, 0]]
    if grads:
        res += list(torch.autograd.grad((a * out).sum() + (c * dlogp[:, 0]).sum(), leaves))
    return tuple(t.detach().cpu().numpy() for t in res)


def scalar_of_row(fn, inp, row, y, mu_raw):
    """the scalar a out + c dlogp of ONE row in f64 with that row's y [D] and mu_raw [K, D] replaced (central differences)"""
    import torch
    f64 = torch.float64
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).reshape(1, -1)
    out, dlogp = fn(t(y), t(mu_raw), t(inp["log_sigma"][row]), t(inp["log_weight"][row]), t(inp["log_eps"][row]))
    return float((t(inp["a"][row]).to(f64) * out).sum() + float(inp["c"][row]) * dlogp[0, 0])


def central_differences(fn, inp):
    """(cd_gy [2, D], cd_gmu [2, K, D]): central differences (h = 1e-6, f64, one component at a time) of the scalar on the TIES rows"""
    K, D = inp["mu_raw"].shape[1:]
    gy, gmu = np.zeros((len(TIES), D)), np.zeros((len(TIES), K, D))
    for i, row in enumerate(TIES):
        y0, m0 = inp["y"][row].astype(np.float64), inp["mu_raw"][row].astype(np.float64)
        for j in range(D):
            e = np.zeros(D)
            e[j] = CD_H
            gy[i, j] = (scalar_of_row(fn, inp, row, y0 + e, m0) - scalar_of_row(fn, inp, row, y0 - e, m0)) / (2 * CD_H)
            for k in range(K):
                e2 = np.zeros((K, D))
                e2[k, j] = CD_H
                gmu[i, k, j] = (scalar_of_row(fn, inp, row, y0, m0 + e2) - scalar_of_row(fn, inp, row, y0, m0 - e2)) / (2 * CD_H)
    return gy, gmu


def rel_err(v, v64):
    """max |v - v64| / (1 + |v64|); NaN if any entry is not finite"""
    v, v64 = np.asarray(v, np.float64), np.asarray(v64, np.float64)
    if v.size == 0:
        return 0.0
    if not np.isfinite(v).all():
        return float("nan")
    return float(np.max(np.abs(v - v64) / (1.0 + np.abs(v64))))


def references(G, k, name):
    """the f64 array every row of quantity ``name`` is compared with: the reference's f64 run, on the TIES rows of g_y / g_mu the
    recorded central differences"""
    ref = np.array(G[k + name + "64"])
    if name == "g_y":
        ref[TIES] = G[k + "cd_gy"]
    if name == "g_mu":
        ref[TIES] = G[k + "cd_gmu"].reshape(len(TIES), -1)
    return ref


def group_errors(res, G, k, names=QUANTITIES):
    """{quantity: {group: error}} of the arrays ``res`` (in the order of QUANTITIES) over the four row groups; no row is left out"""
    out = {}
    for name, v in zip(QUANTITIES, res):
        if name not in names:
            continue
        ref = references(G, k, name)
        out[name] = {g: rel_err(v[rows], ref[rows]) for g, rows in (("bulk", BULK), ("narrow", NARROW), ("ties", TIES),
                                                                    ("unyardsticked", UNYARDSTICKED))}
    return out


def assert_within(errs, G, k, factor=4.0, floor=1e-6, what=""):
    """every error within factor * (the reference's own f32 error of that quantity) + floor: the NARROW row under the reference's error
    on it, every other group under its error on the BULK rows"""
    for name, groups in errs.items():
        for group, err in groups.items():
            yard = "narrow" if group == "narrow" else "bulk"
            bound = factor * float(G[f"{k}err_{name}32_{yard}"]) + floor
            print(f"{what}{k}{name} {group}: error {err:.3g}, bound {bound:.3g}")
            assert np.isfinite(err) and err <= bound, (what, k, name, group, err, bound)


def assert_exact(errs, tol=1e-12, tol_ties=1e-7, what=""):
    """the f64 path against the fixture: 1e-12 on every row, except g_y / g_mu on the TIES rows (central differences: 1e-7)"""
    for name, groups in errs.items():
        for group, err in groups.items():
            bound = tol_ties if (group == "ties" and name in ("g_y", "g_mu")) else tol
            print(f"{what}{name} {group}: error {err:.3g}, bound {bound:.3g}")
            assert np.isfinite(err) and err <= bound, (what, name, group, err, bound)
