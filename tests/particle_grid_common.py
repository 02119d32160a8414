"""Shared by test_host_particle_grid.py and test_gpu_particle_grid.py: a grid of (n, d) on both sides of every LDS tile-height switch of the
particle kernels (csrc/bgk_pair.hip, bgk_kdyn.hip), well-conditioned inputs for it, closed-form numpy f64 restatements of the energies of
csrc/bgk_pair_terms.h with a per-element conditioning scale, and the per-element metric.  torch and numpy only.

For every kind the restatement gives u [B], g = d e / d x [B, n d] and Hu = (d^2 e / d x^2) v [B, n d], each divided by T, and for each of
the three an absolute-sum scale A of the same shape: the same sum with every pair contribution replaced by its magnitude and every
difference of monomials inside a coefficient by the sum of the monomials' magnitudes (``reference``).  An f32 evaluation in any summation
order errs by a small multiple of 2^-24 A, so |v - v64| / A sees a fault in a small component that max |v - v64| / (1 + max |v64|) hides.

    e(v) = max over elements of |v - v64| / (A + 1e-6 (1 + max |v64| over the element's sample))         (``metric``)
    e(kernel) <= 4 e(ref32) + 1e-6                                                                      (``bound``)

e(ref32): the same metric for the classes' own torch formulas (``_energy``, under autograd for g, under double backward for Hu) in f32 on
the CPU, measured per case; the factor 4 is the allowance of the particle tests for another summation order, the floor covers an f32 that
happens to be exact.  CAP: e(ref32) <= 64 x 2^-24 is asserted on the host for every case, so that no bound exceeds 1.6e-5."""
import functools

import numpy as np
import torch

import bgflow_amd as bg

B = 97                # a partial last tile at every tile height: 64, 63, 62, 61, 47, 39, 38, 32, 31, 30
# (n, d): what the shape reaches, S = (n d) | 1
GRID = [(3, 1),       # D = 1, odd width, more than one pair
        (64, 1),      # D = 1 at the envelope; hvp 63 rows, kdyn integrate 61 rows
        (3, 2),       # D = 2
        (63, 2),      # S = 127: the last 64-row backward tile (65,280 B); hvp 32 rows; kdyn 62 / 39 / 31 rows
        (64, 2),      # S = 129: the first 32-row backward tile; hvp 31 rows; D = 2 at the envelope
        (2, 3),       # D = 3 with a single pair
        (22, 3),      # S = 67: hvp 61 rows; kdyn backward 47 rows at K = 64
        (42, 3),      # S = 127 through D = 3
        (43, 3)]      # odd width, S = n d = 129
KINDS = ["lj", "ljn", "mdw", "mfn"]
TEMPERATURES = [1.0, 1.7]
CAP = 64 * 2.0 ** -24
COTANGENTS = (1.0, 0.0, -1.0, 1e-3, -1e3, 0.37)
TILE_SHAPES = [(64, 1), (63, 2), (64, 2), (43, 3)]
FAULT_SHAPES = [(64, 1), (63, 2), (43, 3)]
KDYN_SHAPES = [(64, 1), (63, 2), (64, 2), (22, 3), (43, 3)]


# ---- tile heights, from the header comments of bgk_pair.hip and bgk_kdyn.hip -------------------------------------------------------
def row_stride(nd):
    return nd | 1


def rows_forward(nd):
    return 64


def rows_backward(nd):
    """64 rows while x tile + gradient tile + 64 row scales fit 64 KiB, else 32"""
    return 64 if 2 * 64 * row_stride(nd) * 4 + 256 <= 65536 else 32


def rows_hvp(nd):
    """the most rows (<= 64) of four tiles x, u, g, Hu in 64 KiB"""
    return min(64, 65536 // (16 * row_stride(nd)))


def rows_kdyn(nd, what, K=10):
    """min(64, 63,488 B / bytes per row): eval 2 S floats, backward 3 S + 2 (K | 1), integrate 4 S"""
    S = row_stride(nd)
    floats = {"eval": 2 * S, "backward": 3 * S + 2 * (K | 1), "integrate": 4 * S}[what]
    return min(64, 63488 // (4 * floats))


def tile_rows(h):
    """the rows on both sides of the first tile boundary, and the ends of the batch"""
    return sorted({0, h - 1, h, B - 1})


# ---- targets and inputs ------------------------------------------------------------------------------------------------------------
def make(G, kind, n, d, two_event_dims=False):
    """the target of a case with the parameters of particles.npz (as test_gpu_particles.make)"""
    if kind in ("lj", "ljn"):
        eps, rm, osc = (float(v) for v in G["lj_params"])
        return bg.LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=kind == "lj", oscillator_scale=osc, two_event_dims=two_event_dims)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in G["mdw_params"])
        return bg.MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=two_event_dims)
    return bg.MeanFreeNormalDistribution(n * d, n, std=float(G["mfn_std"]), two_event_dims=two_event_dims)


def parameters(G, kind):
    """(pair kind, p, osc) of the restatement: p = (eps, rm) or (a, b, c, offset); the mean-free normal's 1 / std^2 is the class's
    (``std`` is an f32 buffer, squared in f32)"""
    if kind in ("lj", "ljn"):
        eps, rm, osc = (float(v) for v in G["lj_params"])
        return "lj", (eps, rm), osc if kind == "lj" else 0.0
    if kind == "mdw":
        return "mdw", tuple(float(v) for v in G["mdw_params"]), 0.0
    std = np.float32(float(G["mfn_std"]))
    return "none", (), 1.0 / float(std * std)


@functools.lru_cache(maxsize=None)
def _lattice(n, d, rm):
    m = 1
    while m ** d < n:
        m += 1
    points = np.stack(np.meshgrid(*[np.arange(m)] * d, indexing="ij"), axis=-1).reshape(-1, d)[:n]
    gen = torch.Generator(device="cpu").manual_seed(1000 * n + d)
    noise = torch.randn(B, n, d, generator=gen, dtype=torch.float32)
    x = torch.tensor(points * (1.15 * rm), dtype=torch.float32)[None] + (0.08 * rm) * noise
    return x.reshape(B, n * d).contiguous()


def positions(G, n, d):
    """f32 [B, n d]: the first n points of a ceil(n^(1/d))^d lattice at spacing 1.15 rm, plus 0.08 rm normal noise from a seeded CPU
    generator; deliberately well conditioned (no near-collision: ``min_pair_distance``)"""
    return _lattice(n, d, float(G["lj_params"][1])).clone()


def vector(n, d):
    """the seeded f32 normal vector [B, n d] of the Hessian products, of mean 2 and width 1.  (Of mean 0 it breaks the cap for the
    oscillator term: the scale osc (|v_ik| + |vbar_k|) is tiny where both happen to be, while any f32 mean of n numbers errs by
    2^-24 mean |v| -- the torch formulas then score up to 104 x 2^-24 on the mean-free normal.  With |vbar| ~ mean |v| the scale is the
    conditioning of the mean as well; the differences v_i - v_j of the pair terms keep both signs.)"""
    gen = torch.Generator(device="cpu").manual_seed(7000 + 10 * n + d)
    return 2.0 + torch.randn(B, n * d, generator=gen, dtype=torch.float32)


def min_pair_distance(x, n, d):
    x = np.asarray(x, dtype=np.float64).reshape(-1, n, d)
    d2 = ((x[:, :, None] - x[:, None, :]) ** 2).sum(-1) + np.eye(n) * 1e30
    return float(np.sqrt(d2.min()))


def cotangent(device="cpu"):
    """w [B, 1]: COTANGENTS in turn"""
    return torch.tensor([COTANGENTS[b % len(COTANGENTS)] for b in range(B)], dtype=torch.float32, device=device)[:, None]


BOX_NSOLVENT = [1, 61]          # 3 particles: the smallest bath the fixture lacks; 63 particles: S = 127, the last 64-row backward tile


@functools.lru_cache(maxsize=None)
def _box_lattice(nsolvent):
    n = nsolvent + 2
    gen = torch.Generator(device="cpu").manual_seed(500 + nsolvent)
    if nsolvent == 1:
        # the dimer's first particle below the lower wall in y, its second and the solvent particle 0.85 apart (rc = 0.9) at the upper wall
        base = torch.tensor([[-0.7, -3.25], [0.75, 2.4], [1.05, 3.2]])
        return (base[None] + 0.05 * torch.randn(B, n, 2, generator=gen)).reshape(B, 2 * n).contiguous()
    points = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    base = torch.tensor((points - 3.5) * 1.15, dtype=torch.float32)             # +-4.025: the outer rows and columns are beyond the walls
    return (base[None] + 0.08 * torch.randn(B, n, 2, generator=gen)).reshape(B, 2 * n).contiguous()


def box_positions(nsolvent):
    """f32 [B, 2 (nsolvent + 2)] for the particle box (walls at +-3, rc = 0.9): an 8 x 8 lattice at spacing 1.15 with 0.08 normal noise
    (a few dozen pairs of the batch within rc), or three hand-placed particles; every sample has coordinates beyond both walls"""
    return _box_lattice(nsolvent).clone()


def box_input_conditions(x, nsolvent, rc, half):
    """(pairs of the batch within rc, not counting the dimer's; samples with a coordinate below -half; samples with one above half)"""
    n = nsolvent + 2
    xp = np.asarray(x, dtype=np.float64).reshape(-1, n, 2)
    i, j = np.triu_indices(n, 1)
    i, j = i[1:], j[1:]
    dist = np.sqrt(((xp[:, i] - xp[:, j]) ** 2).sum(-1))
    flat = xp.reshape(xp.shape[0], -1)
    return int((dist < rc).sum()), int((flat.min(axis=1) < -half).sum()), int((flat.max(axis=1) > half).sum())


# ---- the f64 restatement -----------------------------------------------------------------------------------------------------------
def _pair_coefficients(pair_kind, p, d2):
    """per pair, from d2 = |x_i - x_j|^2 (bgk_pair_terms.h's header): (e, cf, cf'), d e_ij / d x_i = cf (x_i - x_j), cf' = d cf / d d2, and
    the three with the magnitudes of their monomials summed"""
    if pair_kind == "lj":
        eps, rm = p
        q = d2 + 1e-6
        s = rm * rm / q
        c12 = 12.0 * eps / (rm * rm)
        return (eps * (s ** 6 - 2 * s ** 3), -c12 * (s ** 7 - s ** 4), c12 * (7 * s ** 7 - 4 * s ** 4) / q,
                eps * (s ** 6 + 2 * s ** 3), c12 * (s ** 7 + s ** 4), c12 * (7 * s ** 7 + 4 * s ** 4) / q)
    a, b, c, off = p
    r = np.sqrt(d2)
    t = r - off
    ta = np.abs(t)
    f1, f2 = 4 * a * t ** 3 + 2 * b * t, 12 * a * t ** 2 + 2 * b
    f1a, f2a = 4 * abs(a) * ta ** 3 + 2 * abs(b) * ta, 12 * abs(a) * t ** 2 + 2 * abs(b)
    return (a * t ** 4 + b * t ** 2 + c, f1 / r, (f2 / r - f1 / d2) / (2 * r),
            abs(a) * t ** 4 + abs(b) * t ** 2 + abs(c), f1a / r, (f2a / r + f1a / d2) / (2 * r))


def reference(G, kind, x, n, d, temperature=1.0, v=None, pair_weight=None, parameters_override=None):
    """u, g (and Hu for a vector v) of the rows of x [B, n d] in f64 with their scales: dict u, A_u [B]; g, A_g, hu, A_hu [B, n d].
    ``pair_weight`` [n, n] (default 1 off the diagonal) multiplies what pair (i, j) adds to particle i -- for the planted faults of
    test_host_particle_grid.py only."""
    pair_kind, p, osc = parameters_override or parameters(G, kind)
    x = np.asarray(x, dtype=np.float64).reshape(-1, n, d)
    w = (1.0 - np.eye(n)) if pair_weight is None else np.asarray(pair_weight, dtype=np.float64)
    wa = np.abs(w)
    out = {k: 0.0 for k in ("u", "A_u", "g", "A_g", "hu", "A_hu")}
    if v is not None:
        v = np.asarray(v, dtype=np.float64).reshape(-1, n, d)
    if pair_kind != "none":
        df = x[:, :, None, :] - x[:, None, :, :]                            # [B, i, j, k]
        d2 = (df ** 2).sum(-1) + np.eye(n)                                  # (the diagonal: any positive number, weight 0)
        e, cf, cfp, ea, cfa, cfpa = _pair_coefficients(pair_kind, p, d2)
        out["u"] = 0.5 * (w * e).sum((1, 2))
        out["A_u"] = 0.5 * (wa * ea).sum((1, 2))
        out["g"] = ((w * cf)[..., None] * df).sum(2)
        out["A_g"] = ((wa * cfa)[..., None] * np.abs(df)).sum(2)
        if v is not None:
            dv = v[:, :, None, :] - v[:, None, :, :]
            s, sa = (df * dv).sum(-1), np.abs(df * dv).sum(-1)
            out["hu"] = ((w * cf)[..., None] * dv + (2 * w * cfp * s)[..., None] * df).sum(2)
            out["A_hu"] = ((wa * cfa)[..., None] * np.abs(dv) + (2 * wa * cfpa * sa)[..., None] * np.abs(df)).sum(2)
    if osc != 0.0:
        mean = x.mean(1, keepdims=True)
        centroid = osc * 0.5 * ((x - mean) ** 2).sum((1, 2))
        out["u"], out["A_u"] = out["u"] + centroid, out["A_u"] + centroid
        out["g"], out["A_g"] = out["g"] + osc * (x - mean), out["A_g"] + osc * (np.abs(x) + np.abs(mean))
        if v is not None:
            vmean = v.mean(1, keepdims=True)
            out["hu"], out["A_hu"] = out["hu"] + osc * (v - vmean), out["A_hu"] + osc * (np.abs(v) + np.abs(vmean))
    rows = x.shape[0]
    res = {}
    for k, val in out.items():
        if v is None and k in ("hu", "A_hu"):
            continue
        val = np.broadcast_to(val, (rows,) if k in ("u", "A_u") else (rows, n, d)) / temperature
        res[k] = val.copy() if k in ("u", "A_u") else val.reshape(rows, n * d).copy()
    return res


def metric(got, want, scale):
    """max over elements of |got - want| / (scale + 1e-6 (1 + max |want| over the element's sample)); [B] or [B, n d]"""
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    assert got.shape == want.shape == scale.shape and np.isfinite(got).all()
    top = np.abs(want) if want.ndim == 1 else np.abs(want).max(axis=1, keepdims=True)
    return float((np.abs(got - want) / (scale + 1e-6 * (1.0 + top))).max())


def bound(e_ref32):
    return 4.0 * e_ref32 + 1e-6


def worst(got, want, scale):
    """(row, column) of the element that sets ``metric``, for a failure's message"""
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    top = np.abs(want) if want.ndim == 1 else np.abs(want).max(axis=1, keepdims=True)
    return np.unravel_index(np.argmax(np.abs(got - want) / (scale + 1e-6 * (1.0 + top))), got.shape)


# ---- the classes' own torch formulas on the CPU ------------------------------------------------------------------------------------
def torch_formulas(energy, x, temperature=1.0, v=None):
    """u [B], g [B, n d] (and Hu) of ``_energy`` / T as torch ops in the dtype of x on the CPU: autograd and double backward"""
    x = x.detach().cpu().clone().requires_grad_(True)
    u = energy._energy(x) / temperature
    (g,) = torch.autograd.grad(u.sum(), x, create_graph=v is not None)
    res = {"u": u.detach().reshape(-1).numpy(), "g": g.detach().numpy()}
    if v is not None:
        (hu,) = torch.autograd.grad((g * v.to(x)).sum(), x, allow_unused=True)
        res["hu"] = (torch.zeros_like(x) if hu is None else hu).numpy()
    return res


def ref32_errors(G, kind, n, d, temperature=1.0):
    """(e(ref32) of u, g, Hu; the f64 restatement) of a grid case: the f32 CPU torch formulas under ``metric``"""
    x, v = positions(G, n, d), vector(n, d)
    ref = reference(G, kind, x, n, d, temperature, v)
    got = torch_formulas(make(G, kind, n, d), x, temperature, v)
    return {k: metric(got[k], ref[k], ref["A_" + k]) for k in ("u", "g", "hu")}, ref
