"""CPU: the references and input builders of the gradient-scale suite (tests/grad_scale_common.py) checked on their own -- the
restatement of h2_pow2_scale against the table in its header comment, a numpy emulation of the f16 hi + lo split against the element
bound the GPU tests derive their tolerances from, and the fixtures of test_gpu_grad_scale.py / test_gpu_rqs_vjp_edges.py against both
precisions of the oracle (so that a GPU failure is a kernel's, not a fixture's)."""
import numpy as np
import pytest

import grad_scale_common as gc


def test_pow2_scale_restatement_against_the_header_table():
    """bgk_mfma_h2.h: 'the power of two that brings a maximum magnitude m >= 0 into [2^14, 2^15), and its reciprocal; 1 for m = 0,
    subnormal or not finite; exponents beyond +-100 are clamped (the reciprocal stays a normal number)'"""
    f = np.float32
    for m, want in ((0.0, 1.0), (1e-40, 1.0), (float(np.finfo(f).tiny) / 2, 1.0), (np.inf, 1.0), (1.0, 2.0 ** 14), (65504.0, 0.5),
                    (3e38, 2.0 ** -100), (float(np.finfo(f).tiny), 2.0 ** 100), (1e-6, 2.0 ** 34), (0.75, 2.0 ** 15), (2.0 ** 14, 1.0),
                    (np.nextafter(f(2.0 ** 15), f(0)), 1.0), (2.0 ** 15, 0.5)):
        sc, inv = gc.pow2_scale(m)
        assert sc.dtype == np.float32 and float(sc) == want, (m, float(sc), want)
        assert float(sc) * float(inv) == 1.0 and np.isfinite(inv) and float(inv) >= float(np.finfo(f).tiny)
    # every maximum whose scale is not clamped (2^-86 <= m < 2^115) lands in [2^14, 2^15): a factor 2 below the f16 maximum
    rng = np.random.default_rng(0)
    ms = np.exp2(rng.uniform(-86, 115, 2000)).astype(f)
    for m in ms:
        sc, _ = gc.pow2_scale(m)
        assert 2.0 ** 14 <= float(m) * float(sc) < 2.0 ** 15


def test_split_emulation_meets_the_element_bound_on_the_mixed_rows():
    """hi + lo of an element under the scale of the governing maximum M is off by at most max(2^-22 |g|, 2^-39 M) -- on exactly the row
    exponents of the GPU test (rows 2^-20, 2^-30, 2^-38, 2^-45 below the maximum).  Worst error / bound: 0.50."""
    g = gc.mixed_cotangent(425, seed=1)
    M = float(np.abs(g).max())
    err = np.abs(gc.split_roundtrip(g, M) - g.astype(np.float64))
    ratio = err / gc.element_bound(g, M)
    print(f"split emulation: worst error / bound {ratio.max():.3f}; per row exponent:",
          {int(s): round(float(ratio[gc.mixed_row_exponents() == s].max()), 3) for s in np.unique(gc.mixed_row_exponents())})
    assert ratio.max() <= 1.0
    assert ratio.max() >= 0.25, "a bound this loose would not see a lost bit"
    # the dynamic range the design accepts: full 22 bits down to 2^-17 of the maximum, nothing left 2^-39 below it
    a = np.abs(g.astype(np.float64))
    s = gc.mixed_row_exponents()
    assert (err[a >= 2.0 ** -17 * M] / a[a >= 2.0 ** -17 * M]).max() <= 2.0 ** -22
    assert (err[s == 20] / a[s == 20]).max() > 2.0 ** -22
    assert np.all(gc.split_roundtrip(g[s == 45], M) == 0.0)
    # a maximum under-reported by more than the margin of 2 overflows the f16 range
    hi, _ = gc.split_f16(g * gc.pow2_scale(M / 4.1)[0])
    assert np.isinf(hi.astype(np.float32)).any()
    hi, _ = gc.split_f16(g * gc.pow2_scale(M / 1.9)[0])
    assert np.isfinite(hi.astype(np.float32)).all()


@pytest.mark.parametrize("P,d_c,periodic", [(425, 17, False), (225, 17, True)])
@pytest.mark.parametrize("act", [1, 3])
def test_emulated_chain_stays_inside_the_stage_bounds(P, d_c, periodic, act):
    """the design restated in numpy -- gradient tiles split under the tensor's (first GEMM) or the 32-row tile's own scale, weights
    split to 22 bits under theirs, exact products -- stays inside dx_chain_reference's bounds at every element of every stage (the f32
    accumulation the bound also allows for is not emulated)"""
    rng = np.random.default_rng(P + act)
    n_in = 2 * d_c if periodic else d_c
    W0, W1, W2 = ((rng.uniform(-1, 1, s) / np.sqrt(s[1])).astype(np.float32) for s in ((128, n_in), (128, 128), (P, 128)))
    b0, b1 = ((rng.uniform(-1, 1, 128) / np.sqrt(128)).astype(np.float32) for _ in range(2))
    x = rng.uniform(0, 1, (gc.B_MIXED, d_c)).astype(np.float32)
    z0, z1 = gc.conditioner_pre_activations(x, W0, b0, W1, b1, act, periodic)
    g = gc.mixed_cotangent(P, seed=2)
    M = float(np.abs(g).max())
    ref = gc.dx_chain_reference(g, M, z1, z0, x, W0, W1, W2, act, periodic)

    def w_split(W):
        return gc.split_roundtrip(W, float(np.abs(W).max()))

    def tiles(a):
        out = np.empty(a.shape)
        for b in range(0, a.shape[0], 32):
            blk = a[b:b + 32].astype(np.float32)
            out[b:b + 32] = gc.split_roundtrip(blk, float(np.abs(blk).max()))
        return out
    g_z1 = ((gc.split_roundtrip(g, M) @ w_split(W2)) * gc.act_f64(z1, act)[1]).astype(np.float32)
    g_z0 = ((tiles(g_z1) @ w_split(W1)) * gc.act_f64(z0, act)[1]).astype(np.float32)
    g_f = (tiles(g_z0) @ w_split(W0)).astype(np.float32).astype(np.float64)
    if periodic:
        c, s = np.cos(2 * np.pi * x.astype(np.float64)), np.sin(2 * np.pi * x.astype(np.float64))
        g_f = 2 * np.pi * (c * g_f[:, d_c:] - s * g_f[:, :d_c])
    for name, got in (("g_z1", g_z1), ("g_z0", g_z0), ("g_x", g_f)):
        want, bound = ref[name]
        ratio = np.abs(got.astype(np.float64) - want) / bound
        print(f"{name}: worst error / bound {ratio.max():.3f} (row {int(ratio.max(1).argmax())})")
        assert np.isfinite(got).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("Kb", [6, 8, 32])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("B", [1, 33])
def test_absmax_fixtures_put_the_maximum_where_they_say(oracle, Kb, inverse, B):
    """put_maximum_first / put_maximum_last against the f32 oracle: the largest |g_params| of the batch is the first float of row 0 /
    the slot of the last non-circular dim in the last row (the very last float), ahead of every other entry by a factor > 2"""
    kw = {k: v for k, v in gc.SETTINGS.items() if k != "enable_identity_init"}
    for put in (gc.put_maximum_first, gc.put_maximum_last):
        y, p, go, gl = gc.rqs_absmax_inputs(Kb, B)
        r, c = put(y, p, go, gl, Kb)
        _, gp = oracle.rqs_backward(y, p, go, gl, is_circular=gc.CIRC7, inverse=inverse, n_bins=Kb, dtype=np.float32, **kw)
        a = np.abs(gp)
        assert np.isfinite(a).all() and np.unravel_index(a.argmax(), a.shape) == (r, c)
        rest = a.copy()
        rest[r, c] = 0.0
        assert a[r, c] > 2.0 * rest.max(), put.__name__


@pytest.mark.parametrize("Kb,inverse,circular,scale,box", gc.VJP_CASES)
def test_vjp_edge_rows_against_both_oracle_precisions(oracle, Kb, inverse, circular, scale, box):
    """the row layout of test_gpu_rqs_vjp_edges.py under the oracle alone: the knot rows sit on the f32 knots bit for bit, both
    precisions are finite on every element whose clamped input lies inside the searched interval (saturated parameters, inputs on
    the ends of minimal-width bins included; outside it -- second box, forward direction -- a bin is extrapolated and f64 itself may be NaN), the two precisions
    pick the same bin everywhere but on the knot rows, and the exact statements the GPU test makes of the kernel hold for the oracle"""
    inp = gc.vjp_edge_inputs(oracle, Kb, inverse, circular, scale, box)
    y, knots = inp["y"], inp["knots"]
    for r in gc.VJP_ROWS["knots"]:
        assert np.array_equal(y[r], knots[r, :, 1 + r % (Kb - 1)])
    for r in gc.VJP_ROWS["knots_ulp"]:
        assert np.all(np.abs(y[r].view(np.int32) - knots[r, :, 1 + r % (Kb - 1)].view(np.int32)) == 1)
    gy32, gp32, i32 = gc.vjp_oracle(oracle, inp, Kb, inverse, np.float32)
    gy64, gp64, i64 = gc.vjp_oracle(oracle, inp, Kb, inverse, np.float64)
    ex = gc.extrapolated(inp, inverse)      # second box, forward direction: inputs clamped to [left, right] but outside [bottom, top]
    fin32, fin64 = (gc.element_finite(a, b, Kb, inp["circ"]) for a, b in ((gy32, gp32), (gy64, gp64)))
    assert fin32[~ex].all() and fin64[~ex].all() and not (fin64 & ~fin32).any()
    assert ex.any() == (box == gc.WIDE_BOX and not inverse) and not ex[np.r_[0:2, 4:6, 8:64]].any()
    other = np.ones(gc.VJP_B, bool)
    other[8:32] = False
    same = (i32 == i64) & ~ex
    assert (i32 == i64)[other].all(), "the precisions disagree on a bin away from the knots"
    R = gc.VJP_ROWS
    for gy, gp in ((gy32, gp32), (gy64, gp64)):
        assert not gy[R["dead"]].any() and not gp[R["dead"]].any()
        assert not gy[[R["below"], R["above"]]].any()
        assert np.array_equal(gp[R["below"]], gp[R["clamp_lo"]], equal_nan=True) and np.array_equal(gp[R["above"]], gp[R["clamp_hi"]], equal_nan=True)
    err = gc.row_relative_errors(gy32, gp32, gy64, gp64, same, Kb, inp["circ"])
    print(f"f32 oracle against f64, same-bin elements: worst row {np.nanmax(err):.2e} (row {int(np.nanargmax(err))}), median {np.nanmedian(err):.2e}")
