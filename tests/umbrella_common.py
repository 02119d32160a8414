"""Shared by tests/golden/make_umbrella_goldens.py, test_host_umbrella.py and test_gpu_umbrella.py: the toy system of fixture part (a), the
MBAR cases of part (b) and the bounds of the comparisons.  Imports numpy alone at module level: the fixture maker must not import
bgflow_amd."""
import json

import numpy as np

# ---- part (a): the reference's UmbrellaSampling on a 1-d double well -------------------------------------------------------------------
A_SEED = 2027
A_N_UMBRELLA, A_K, A_M_MIN, A_M_MAX, A_NSTEPS = 4, 10.0, -1.0, 1.0, 200
A_X0 = np.array([[-1.0]])
A_NOISE = 0.2


def double_well(x):
    """u(x) = 2 (x^2 - 1)^2 + x / 2 on configurations [walkers, 1]"""
    q = x[:, 0]
    return 2.0 * (q * q - 1.0) ** 2 + 0.5 * q


def first_coordinate(x):
    return x[:, 0]


def a_key(forward_backward):
    return "a_fb" if forward_backward else "a_fwd"


# ---- part (b): MBAR cases ------------------------------------------------------------------------------------------------------------
# name -> (counts per window, centres, force constant).  Samples of window k are draws of the exact biased density of u = x^2 / 2 under
# k (x - m)^2: a Gaussian of mean k m / (0.5 + k) and variance 0.5 / (0.5 + k), i.e. 0.58^2 at k = 1.  Every case overlaps well: all
# centres of a case lie within 2 (3.5 standard deviations), so the iteration contracts fast (tens of iterations to 1e-12; the same
# windows spread over -2 .. 2 at k = 4 need hundreds).  The 64- and 256-window cases run forward and backward over the same centres,
# as UmbrellaSampling(forward_backward=True) does: duplicated centres.
B_SEED = 2028


def _there_and_back(lo, hi, n):
    m = np.linspace(lo, hi, n)
    return np.concatenate([m, m[::-1]])


B_CASES = {
    "k1": ((37,), np.array([0.25]), 1.0),
    "k2": ((1, 3), np.array([-0.5, 0.5]), 1.0),
    "k5": ((257, 300, 129, 64, 250), np.linspace(-1.0, 1.0, 5), 1.0),
    "k64": ((8,) * 64, _there_and_back(-1.0, 1.0, 32), 1.0),
    "k256": ((8,) * 256, _there_and_back(-1.0, 1.0, 128), 1.0),
    "k257": ((8,) * 257, np.linspace(-1.0, 1.0, 257), 1.0),
}
B_TOLERANCE = 1e-12            # the stop rule the tests and the fixture's restatement run the cases at


def b_split(G, case):
    """the case's samples (float32, as stored) as one array per window"""
    counts = B_CASES[case][0]
    return np.split(G[f"{case}_rc"], np.cumsum(counts)[:-1])


def b_tensors(G, case, dtype, device="cpu"):
    """the case's windows as torch tensors of ``dtype`` (the stored float32 values, or their exact widening)"""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dtype).to(device) for t in b_split(G, case)]


def b_log_weights(G, case, f):
    """-D_n at the free energies ``f`` in numpy f64 on the widened samples"""
    counts, m, k = B_CASES[case]
    r = G[f"{case}_rc"].astype(np.float64)
    a = (np.log(np.array(counts, np.float64)) + np.asarray(f, np.float64))[None, :] - k * (r[:, None] - m[None, :]) ** 2
    mx = a.max(1)
    return -(mx + np.log(np.exp(a - mx[:, None]).sum(1)))


def b_bound(G):
    """|f - f_BFGS| allowed for any path: ten times the largest disagreement between the fixture maker's own f64 restatement of the
    iteration and BFGS over all cases (BFGS stops on its own gradient tolerance), recorded in the fixture"""
    return 10.0 * float(G["b_agreement"])


def b_meta(G):
    return json.loads(str(G["b_meta"]))


def path_bound(G, case):
    """|f(one path) - f(another path)| on the same numbers at ``B_TOLERANCE``: each path stops with err <= tolerance, i.e. within
    tolerance rho / (1 - rho) of the fixed point for a linear contraction rate rho, here taken from the iteration count the fixture
    recorded (err falls from O(1) to the tolerance in that many steps); the paths may stop one iteration apart (another tolerance);
    1e-13 covers the f64 rounding of the sums (K N eps at most)"""
    iterations = max(2, b_meta(G)[case]["iterations"])
    rho = B_TOLERANCE ** (1.0 / iterations)
    return 2.0 * B_TOLERANCE / (1.0 - rho) + 1e-13


def log_weight_bound(K, log_w):
    """-D_n from two implementations at the SAME f: a sum of K positive terms <= 1, each the exponential of an argument of magnitude up
    to ~40 (relative error ~ 40 eps), added in another order (K eps), then one log"""
    return (K + 64) * 2.0 ** -52 * (1.0 + float(np.abs(np.asarray(log_w)).max()))


def check_case(G, case, r, label):
    """an ``MBARResult`` of a fixture case run at ``B_TOLERANCE`` against the BFGS values, the fixture's iteration count and -D_n
    restated in numpy at the result's own f; returns f as a numpy array"""
    import torch
    counts, centres, k = B_CASES[case]
    want = G[f"{case}_f"]
    f = r.f.cpu().numpy() if torch.is_tensor(r.f) else r.f
    log_w = r.log_weights.cpu().numpy() if torch.is_tensor(r.log_weights) else r.log_weights
    diff = float(np.abs(f - want).max())
    print(f"{label}{case}: iterations {r.iterations} (fixture {b_meta(G)[case]['iterations']}), err {r.err:.2e}, |f - f_BFGS| {diff:.2e} "
          f"(bound {b_bound(G):.2e})")
    assert r.status == 0 and r.err <= B_TOLERANCE
    assert f.dtype == np.float64 and f.shape == (len(counts),) and f[0] == 0
    assert diff <= b_bound(G)
    assert abs(r.iterations - b_meta(G)[case]["iterations"]) <= 1
    want_w = b_log_weights(G, case, f)
    assert log_w.dtype == np.float64 and log_w.shape == want_w.shape
    assert np.abs(log_w - want_w).max() <= log_weight_bound(len(counts), want_w)
    return f


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def check_entry_arguments(lib):
    """every argument check of bgk_mbar_solve_steps / bgk_mbar_log_weights comes before the first launch: fake pointers are never
    dereferenced, so this runs with or without a device"""
    import ctypes
    fake = ctypes.c_void_p(64)

    def solve(rc=fake, n=8, dtype=0, table=fake, K=2, nb=1, partial=fake, f=fake, record=fake, max_iter=100, tol=1e-10, n_steps=0):
        return lib.bgk_mbar_solve_steps(rc, n, dtype, table, K, nb, partial, f, record, max_iter, tol, n_steps, None)

    assert solve() == 0                                               # n_steps == 0: nothing is launched
    for bad in (dict(rc=None), dict(table=None), dict(partial=None), dict(f=None), dict(record=None)):
        assert solve(**bad) == -1 and b"null pointer" in lib.bgk_last_error()
    assert solve(n=0) == -1 and solve(K=0) == -1 and solve(n=-1) == -1 and b"sizes" in lib.bgk_last_error()
    assert solve(dtype=2) == -1 and b"dtype" in lib.bgk_last_error() and solve(dtype=-1) == -1
    assert solve(dtype=1) == 0 and solve(rc=ctypes.c_void_p(68)) == 0                    # a 4-byte aligned f32 pointer is fine
    assert solve(rc=ctypes.c_void_p(68), dtype=1) == -1 and solve(table=ctypes.c_void_p(68)) == -1 and b"aligned" in lib.bgk_last_error()
    assert solve(f=ctypes.c_void_p(68)) == -1 and solve(record=ctypes.c_void_p(66)) == -1 and solve(partial=ctypes.c_void_p(65)) == -1
    assert solve(K=256, n=256) == 0
    assert solve(K=257, n=4096) == -2 and b"envelope" in lib.bgk_last_error()          # BGK_EUNSUPPORTED
    assert solve(K=9, n=8) == -1 and b"at least one" in lib.bgk_last_error()
    assert solve(nb=0) == -1 and solve(nb=513) == -1 and b"n_blocks" in lib.bgk_last_error() and solve(nb=512) == 0
    assert solve(max_iter=0) == -1 and b"maximum_iterations" in lib.bgk_last_error()
    assert solve(tol=-1.0) == -1 and solve(tol=float("nan")) == -1 and b"tolerance" in lib.bgk_last_error() and solve(tol=0.0) == 0
    assert solve(n_steps=-1) == -1

    def weights(rc=fake, n=8, dtype=0, table=fake, K=2, f=fake, out=fake):
        return lib.bgk_mbar_log_weights(rc, n, dtype, table, K, f, out, None)

    for bad in (dict(rc=None), dict(table=None), dict(f=None), dict(out=None)):
        assert weights(**bad) == -1 and b"null pointer" in lib.bgk_last_error()
    assert weights(n=0) == -1 and weights(K=0) == -1 and weights(dtype=3) == -1 and weights(K=9) == -1
    assert weights(K=257, n=4096) == -2 and weights(out=ctypes.c_void_p(68)) == -1 and weights(rc=ctypes.c_void_p(68), dtype=1) == -1


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def chain_bound(F):
    """umbrella_free_energies: every link is -log of a ratio of two means of numbers in (0, 1], the same numpy calls as the reference's;
    allowed: 8 roundings of the result's dtype per link, relative to 1 + |F|"""
    F = np.asarray(F)
    return 8.0 * np.finfo(F.dtype).eps * (F.size - 1) * (1.0 + np.abs(F).max())
