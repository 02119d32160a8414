"""Shared by test_host_grad_scale.py, test_gpu_grad_scale.py and test_gpu_rqs_vjp_edges.py: CPU references and input builders for the
hand-off of gradient tensors and their published maxima along the training backward (bgk_rqs_backward -> bgk_dense_backward_dx ->
bgk_dense_weight_grad) and for the spline VJP at its edges.  torch / numpy only, importable without a GPU."""
import numpy as np
import torch

from bgflow_amd.utils import synth

BATCHES = (1, 31, 32, 33, 129, 257)     # one row | a partial, a full, a full + 1 MFMA tile | the 128-row streaming tile + 1 | > 1 workgroup
CIRC7 = np.array([1, 0, 1, 1, 0, 0, 1], bool)
SETTINGS = dict(min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, enable_identity_init=True)
ROW_FILL, COL_FILL, CANARY = 1e30, float("nan"), -777.25


# ---------------------------------------------------------------------------------------------------------------------------------
# the scale: bgk_mfma_h2.h::h2_pow2_scale, and the f16 hi + lo split under it
# ---------------------------------------------------------------------------------------------------------------------------------
def pow2_scale(m):
    """(scale, 1 / scale) as np.float32: the power of two that brings a maximum magnitude m >= 0 into [2^14, 2^15); 1 for m = 0,
    subnormal or not finite; exponents beyond +-100 clamped (restated from the integer arithmetic of h2_pow2_scale)"""
    e = int((np.float32(m).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF))
    sb = min(max(268 - e, 27), 227)
    if e == 0 or e == 255:
        sb = 127
    return np.uint32(sb << 23).view(np.float32), np.uint32((254 - sb) << 23).view(np.float32)


def split_f16(v):
    """hi = rne_f16(v), lo = rne_f16(v - hi) of an f32 array (h2_split_pair: v_cvt_pk_f16_f32, then one fused f16(v - hi))"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)     # (v - hi is exact in f32: hi holds v's leading 11 bits)
    return hi, lo


def split_roundtrip(g, m):
    """what a GEMM sees of the f32 gradient g under the scale of maximum m: (hi + lo) / scale, in f64"""
    sc, inv = pow2_scale(m)
    hi, lo = split_f16(np.asarray(g, np.float32) * sc)
    return (hi.astype(np.float64) + lo.astype(np.float64)) * float(inv)


def element_bound(g, m):
    """round-off a gradient element carries into a GEMM: 22 bits of its own magnitude, or the f16 subnormal spacing under the scale
    (2^-25 where the maximum sits in [2^14, 2^15): 2^-39 of the governing maximum)"""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(g, np.float64)), 2.0 ** -39 * np.asarray(m, np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# section B: mixed row scales through the conditioner's input-gradient chain
# ---------------------------------------------------------------------------------------------------------------------------------
B_MIXED = 97        # three full 32-row tiles and one row


def mixed_row_exponents():
    """row r of the cotangent is randn * 2^-s[r]: tile 0 at 0 (rows 5, 6: the absolute-floor regime, 38 and 45), tile 1 at 20 with
    row 32 at 0, tile 2 at 30, row 96 (a tile of its own) at 10"""
    s = np.zeros(B_MIXED, np.int64)
    s[32:64] = 20
    s[32] = 0
    s[64:96] = 30
    s[96] = 10
    s[5], s[6] = 38, 45
    return s


def mixed_cotangent(P, seed):
    g = np.random.default_rng(seed).standard_normal((B_MIXED, P)).astype(np.float32)
    return g * (2.0 ** -mixed_row_exponents()[:, None]).astype(np.float32)          # (exact: powers of two, no underflow)


def act_f64(z, act):
    """(act(z), act'(z)) in f64; act: 1 SiLU, 3 Tanh (the kernels' activation codes)"""
    z = np.asarray(z, np.float64)
    if act == 1:
        s = 1.0 / (1.0 + np.exp(-z))
        return z * s, s * (1.0 + z * (1.0 - s))
    assert act == 3
    h = np.tanh(z)
    return h, 1.0 - h * h


def featurise(x, periodic):
    x = np.asarray(x, np.float64)
    return np.concatenate([np.cos(2 * np.pi * x), np.sin(2 * np.pi * x)], -1) if periodic else x


def conditioner_pre_activations(x, W0, b0, W1, b1, act, periodic):
    """z0, z1 [B, 128] of a plain f32 forward of the conditioner (torch on the CPU)"""
    f = torch.nn.functional.silu if act == 1 else torch.tanh
    xt = torch.as_tensor(np.asarray(x, np.float32))
    W0, b0, W1, b1 = (np.asarray(a, np.float32) for a in (W0, b0, W1, b1))
    feats = torch.cat([torch.cos(2 * np.pi * xt), torch.sin(2 * np.pi * xt)], -1) if periodic else xt
    z0 = feats @ torch.as_tensor(W0).t() + torch.as_tensor(b0)
    z1 = f(z0) @ torch.as_tensor(W1).t() + torch.as_tensor(b1)
    return z0.numpy(), z1.numpy()


def tile_max(a, tile=32):
    """per row: the largest magnitude of the row's 32-row tile (tiles start at multiples of 32)"""
    a = np.abs(np.asarray(a, np.float64))
    out = np.empty(a.shape[0])
    for b0 in range(0, a.shape[0], tile):
        out[b0:b0 + tile] = a[b0:b0 + tile].max()
    return out


def gemm_bound(G, W, M, carried):
    """element bound of (G W)[r, c] on the split-f16 matrix cores: G [B, n] the exact input, W [n, m], M the governing maximum of G's
    scale (scalar or per row), carried [B, n] the bound G's elements already carry:
    4 (2^-22 A + 2^-39 M Wabs) + n 2^-24 A + carried |W|,  A = |G| |W|,  Wabs = sum_k |W[k, c]|"""
    G, W = np.abs(np.asarray(G, np.float64)), np.abs(np.asarray(W, np.float64))
    A = G @ W
    M = np.broadcast_to(np.asarray(M, np.float64), (G.shape[0],))
    return 4.0 * (2.0 ** -22 * A + 2.0 ** -39 * M[:, None] * W.sum(0)[None, :]) + G.shape[1] * 2.0 ** -24 * A + np.asarray(carried) @ W


def dx_chain_reference(g, g_max, z1, z0, x, W0, W1, W2, act, periodic):
    """f64 input-gradient chain of the conditioner (Linear weights: W2 [P, 128], W1 [128, 128], W0 [128, n_in]) from the f32 tensors
    the kernel reads, with the design's element bound of every tensor the kernel writes.  ``g_max``: the maximum the first GEMM scales
    by.  Returns {name: (reference, bound)} for g_z1, g_z0, g_x."""
    g = np.asarray(g, np.float64)
    W0, W1, W2 = (np.asarray(w, np.float64) for w in (W0, W1, W2))
    d1, d0 = act_f64(z1, act)[1], act_f64(z0, act)[1]
    g_h1 = g @ W2
    b_h1 = gemm_bound(g, W2, float(g_max), np.zeros_like(g))
    g_z1, b_z1 = g_h1 * d1, b_h1 * np.abs(d1)
    g_h0 = g_z1 @ W1
    b_h0 = gemm_bound(g_z1, W1, tile_max(g_z1), b_z1)
    g_z0, b_z0 = g_h0 * d0, b_h0 * np.abs(d0)
    g_f = g_z0 @ W0
    b_f = gemm_bound(g_z0, W0, tile_max(g_z0), b_z0)
    if periodic:
        d_c = x.shape[1]
        c, s = np.cos(2 * np.pi * np.asarray(x, np.float64)), np.sin(2 * np.pi * np.asarray(x, np.float64))
        g_x = 2 * np.pi * (c * g_f[:, d_c:] - s * g_f[:, :d_c])
        b_x = 2 * np.pi * (np.abs(c) * b_f[:, d_c:] + np.abs(s) * b_f[:, :d_c])
    else:
        g_x, b_x = g_f, b_f
    return {"g_z1": (g_z1, b_z1), "g_z0": (g_z0, b_z0), "g_x": (g_x, b_x)}


def weight_grad_reference(g_p, g_z1, g_z0, z1, z0, x, act, periodic):
    """(f64 references, relative L2 of a plain f32 evaluation against them) of (gW0, gb0, gW1, gb1, gW2, gb2) = g^T h, sum g over rows"""
    h1, h0, feats = act_f64(z1, act)[0], act_f64(z0, act)[0], featurise(x, periodic)
    pairs = ((g_z0, feats), (g_z1, h0), (g_p, h1))
    ref, f32_err = [], []
    for g, h in pairs:
        g64 = np.asarray(g, np.float64)
        for want, got in ((g64.T @ h, (torch.as_tensor(np.asarray(g, np.float32)).t() @ torch.as_tensor(h.astype(np.float32))).numpy()),
                          (g64.sum(0), np.cumsum(np.asarray(g, np.float32), axis=0, dtype=np.float32)[-1])):      # (row after row)
            ref.append(want)
            f32_err.append(float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want)))
    return ref, f32_err


# ---------------------------------------------------------------------------------------------------------------------------------
# section A: inputs of bgk_rqs_backward whose largest gradient sits where the test wants it
# ---------------------------------------------------------------------------------------------------------------------------------
def n_params(Kb, circ):
    d = len(circ)
    return 3 * Kb * d + int((~circ).sum())


def rqs_absmax_inputs(Kb, B, circ=CIRC7, seed=0):
    """(y [B, d], params [B, P], g_out [B, d], g_dlogp [B]) of moderate magnitude, closed form"""
    d, P = len(circ), n_params(Kb, circ)
    return (synth(810 + seed + Kb, B, d, uniform=True), synth(710 + seed + Kb, B, P, scale=0.9),
            synth(910 + seed + Kb, B, d), synth(911 + seed + Kb, B))


def put_maximum_first(y, params, g_out, g_dl, Kb, circ=CIRC7, boost=2.0 ** 24):
    """row 0 takes part with its dim 0 alone (flat widths, input in bin 0, log-det cotangent 0) and that cotangent boosted: the largest
    gradient of the launch is then the first float of g_params -- d/d(width 0) = p0 (1 - p0) G_W against -p_m p0 G_W of the other bins,
    G_W ~ 1 / (bin width)^2; bin 0 is half the range high, which keeps the heights' gradients (flat heights: a tie with the widths')
    below it by a factor > 2 in both directions (test_host_grad_scale.py) -- written by the kernel's first lane.  In place; returns
    (row, column)."""
    d = len(circ)
    params[0] = 0.0
    params[0, d * Kb] = np.log(Kb - 1.0)
    y[0] = 0.5
    y[0, 0] = 0.25 / Kb
    g_out[0] = 0.0
    g_out[0, 0] = boost
    g_dl[0] = 0.0
    return 0, 0


def put_maximum_last(y, params, g_out, g_dl, Kb, circ=CIRC7, boost=2.0 ** 24):
    """the last row takes part with its last non-circular dim alone: widths and heights peaked on the last bin (every other bin at its
    minimum: their gradients are ~e^-30), the input at 0.9 inside it, equal slopes -- the output cotangent then reaches the parameters
    through the bin's right derivative, theta^2 / (1 - theta^2) ~ 4 times stronger than through the left one: the largest gradient of the
    launch is the dim's slot, the very last float of g_params.  In place; returns (row, column)."""
    d, P = len(circ), n_params(Kb, circ)
    j = int(np.nonzero(~circ)[0][-1])
    r = y.shape[0] - 1
    params[r] = 0.0
    params[r, 2 * d * Kb:] = 0.3
    for blk in (0, 1):
        params[r, blk * d * Kb + j * Kb + Kb - 1] = 30.0
    y[r] = 0.5
    y[r, j] = 0.9
    g_out[r] = 0.0
    g_out[r, j] = boost
    g_dl[r] = 0.0
    return r, P - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# section C: the spline VJP's edge rows
# ---------------------------------------------------------------------------------------------------------------------------------
VJP_B, VJP_D = 64, 4
VJP_ROWS = dict(lo=0, hi=1, below=2, above=3, under_hi=4, over_lo=5, clamp_lo=6, clamp_hi=7, knots=range(8, 24), knots_ulp=range(24, 32),
                dead=40, gy_zero=41, gl_zero=42)
UNIT_BOX, WIDE_BOX = (0.0, 1.0, 0.0, 1.0), (-2.0, 3.0, 0.5, 1.5)
# (K, inverse, all dims circular, parameter scale, box): K = 8 (register-resident) and 6 (walked), both directions, non-circular plus one
# all-circular K = 8 set, moderate to saturated parameters; and a second box
VJP_CASES = [(Kb, inverse, circ, scale, UNIT_BOX) for Kb, circs in ((8, (False, True)), (6, (False,))) for inverse in (False, True)
             for circ in circs for scale in (0.7, 4.0, 12.0)] + [(8, inverse, False, scale, WIDE_BOX) for inverse in (False, True) for scale in (0.7, 12.0)]


def vjp_edge_inputs(oracle, Kb, inverse, circular, scale, box=UNIT_BOX, params_row=None):
    """Inputs of the VJP's edge suite, B = 64, d = 4.  The searched interval [lo, hi] is [left, right] in the inverse direction and
    [bottom, top] in the forward one; inputs are clamped to [left, right] in both (transformer/spline.py:145-155).
      row 0 / 1: lo / hi; 2 / 3: left - 0.5 / right + 0.5 (clamped); 4: largest float below hi; 5: smallest float above lo (lo = 0: the
      smallest positive float); 6 / 7: left / right with the parameters and cotangents of rows 2 / 3; 8 - 23: interior knot
      1 + r % (K - 1) of the row's own element (the f32 oracle's knots); 24 - 27 / 28 - 31: that knot - / + 1 ulp; 40: both cotangents
      zero; 41: g_out = 0; 42: g_dlogp = 0; every other row: uniform random inside [lo, hi].
    ``params_row`` [P]: one parameter set for the whole batch (the fused layers' form) instead of synth(14, B, P, scale).
    Returns dict(y, params, g_out, g_dl, knot_rows, P)."""
    left, right, bottom, top = box
    lo, hi = (left, right) if inverse else (bottom, top)
    d, B = VJP_D, VJP_B
    circ = np.full(d, bool(circular))
    P = n_params(Kb, circ)
    params = synth(14, B, P, scale=scale) if params_row is None else np.repeat(np.asarray(params_row, np.float32)[None], B, 0)
    params[6:8] = params[2:4]
    y = (lo + (hi - lo) * synth(15 + Kb, B, d, uniform=True).astype(np.float64)).astype(np.float32)
    g_out, g_dl = synth(16 + Kb, B, d), synth(17 + Kb, B)
    g_out[6:8], g_dl[6:8] = g_out[2:4], g_dl[2:4]
    f = np.float32
    y[0], y[1], y[2], y[3] = f(lo), f(hi), f(left - 0.5), f(right + 0.5)
    y[4], y[5] = np.nextafter(f(hi), f(-np.inf)), np.nextafter(f(lo), f(np.inf))
    y[6], y[7] = f(left), f(right)
    kw = {k: v for k, v in SETTINGS.items() if k != "enable_identity_init"}
    det = oracle.rqs(y, params, is_circular=circ, inverse=inverse, left=left, right=right, bottom=bottom, top=top, n_bins=Kb,
                     dtype=np.float32, want_details=True, **kw)[2]
    knots = det["knots"]                                             # [B, d, K + 1]: the searched set
    for r in range(8, 32):
        kn = knots[r, :, 1 + r % (Kb - 1)]
        y[r] = kn if r < 24 else np.nextafter(kn, f(-np.inf) if r < 28 else f(np.inf))
    g_out[40], g_dl[40] = 0.0, 0.0
    g_out[41] = 0.0
    g_dl[42] = 0.0
    return dict(y=y, params=params, g_out=g_out, g_dl=g_dl, circ=circ, P=P, knots=knots, box=box)


def extrapolated(inp, inverse):
    """[B, d]: elements whose input, clamped to [left, right], lies outside the searched interval -- the forward direction searches
    [bottom, top], so with a box whose two intervals differ the first / last bin's rational function is extrapolated there (forward
    kernels and reference alike; the root's discriminant may be negative: NaN, in f64 too)"""
    left, right, bottom, top = inp["box"]
    if inverse:
        return np.zeros(inp["y"].shape, bool)
    x = np.clip(inp["y"].astype(np.float64), left, right)
    return (x < bottom) | (x > top)


def element_finite(gy, gp, Kb, circ):
    """[B, d]: the element's input gradient and all of its parameter gradients are finite"""
    cols = element_columns(Kb, gy.shape[1], circ)
    out = np.isfinite(gy)
    for j in range(gy.shape[1]):
        out[:, j] &= np.isfinite(gp[:, cols[j][cols[j] >= 0]]).all(1)
    return out


def vjp_oracle(oracle, inp, Kb, inverse, dtype):
    left, right, bottom, top = inp["box"]
    kw = {k: v for k, v in SETTINGS.items() if k != "enable_identity_init"}
    gy, gp = oracle.rqs_backward(inp["y"], inp["params"], inp["g_out"], inp["g_dl"], is_circular=inp["circ"], inverse=inverse,
                                 left=left, right=right, bottom=bottom, top=top, n_bins=Kb, dtype=dtype, **kw)
    idx = oracle.rqs(inp["y"], inp["params"], is_circular=inp["circ"], inverse=inverse, left=left, right=right, bottom=bottom, top=top,
                     n_bins=Kb, dtype=dtype, want_details=True, **kw)[2]["bin_idx"]
    return gy, gp, idx


def element_columns(Kb, d, circ):
    """[d, 3 K + 1] column of g_params holding each of an element's gradients (-1: a circular dim has no slot)"""
    cols = np.full((d, 3 * Kb + 1), -1, np.int64)
    slot = 0
    for j in range(d):
        for blk in range(3):
            cols[j, blk * Kb:(blk + 1) * Kb] = blk * d * Kb + j * Kb + np.arange(Kb)
        if not circ[j]:
            cols[j, 3 * Kb] = 3 * d * Kb + slot
            slot += 1
    return cols


def row_relative_errors(gy, gp, ref_gy, ref_gp, same_bin, Kb, circ):
    """per row: max |got - ref| / max |ref row|, the larger of the input gradient's and the parameter gradient's figure; elements
    (row, dim) outside ``same_bin`` [B, d] left out of both maxima; rows without a compared element: NaN"""
    B, d = gy.shape
    cols = element_columns(Kb, d, circ)
    keep_p = np.zeros(gp.shape, bool)
    for j in range(d):
        c = cols[j][cols[j] >= 0]
        keep_p[:, c] = same_bin[:, [j]]
    gy, gp, ref_gy, ref_gp = (np.asarray(a, np.float64) for a in (gy, gp, ref_gy, ref_gp))
    out = np.full(B, np.nan)
    for r in range(B):
        if not same_bin[r].any():
            continue
        worst = 0.0
        for got, ref, keep in ((gy[r], ref_gy[r], same_bin[r]), (gp[r], ref_gp[r], keep_p[r])):
            err, scale = np.abs(got - ref)[keep].max(), np.abs(ref)[keep].max()
            worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
        out[r] = worst
    return out
