"""GPU (-m gpu): the spline VJP (bgk_rqs_vjp.h: hardware rcp / sqrt / exp2 / log2 behind the knots) per element at its edges -- exact
knots, knots +- 1 ulp, the domain's ends, clamped inputs, saturated parameters, dead rows and rows with one cotangent only -- in the
stand-alone kernel (register and memory-walking forms) and in the recompute backward's LDS forms.  Inputs and references:
tests/grad_scale_common.py (checked on the CPU by test_host_grad_scale.py)."""
import numpy as np
import pytest
import torch

import grad_scale_common as gc
from test_gpu_parity import t

pytestmark = pytest.mark.gpu

FLOOR = 2e-5        # the whole-tensor tolerance of test_rqs_backward_kernel
FACTOR = 4.0        # 1-ulp hardware forms against correctly rounded ones
KNOT_SHIFT = 2.4e-7  # how far (unit domain) a hardware-form knot may sit from the deterministic one: the distance __graft_entry__.smoke() allows a bin tie


def _kernel(inp, Kb, inverse, dev):
    from bgflow_amd.transformer import rqs_backward
    from oracle.oracle import nc_slots
    slots = t(nc_slots(inp["circ"], gc.VJP_D), dev)
    gy, gp = rqs_backward(t(inp["y"], dev), t(inp["params"], dev), slots, (Kb, inverse, *inp["box"], gc.SETTINGS), t(inp["g_out"], dev),
                          t(inp["g_dl"], dev))
    return gy.cpu().numpy(), gp.cpu().numpy()


def _judge(tag, gy, gp, oracle, inp, Kb, inverse, near_knot=None):
    """the tolerance of the suite: against the f32 oracle on every row (it picks the kernel's bin by construction), against the f64
    oracle on the rows away from the knots where both precisions pick the same bin -- worst and median row-relative error at most
    FACTOR times the f32 oracle's own against f64, plus FLOOR.  ``near_knot`` [B, d]: elements judged on the input gradient alone (the
    hardware-form knots of the LDS VJP may put them into the neighbouring bin; the spline is C1 there)."""
    gy32, gp32, i32 = gc.vjp_oracle(oracle, inp, Kb, inverse, np.float32)
    gy64, gp64, i64 = gc.vjp_oracle(oracle, inp, Kb, inverse, np.float64)
    circ = inp["circ"]
    # elements whose clamped input lies outside the searched interval (second box, forward direction: [left, right] is not [bottom,
    # top]): a bin's rational function extrapolated, by the forward kernels and the reference alike; the root may not exist (NaN in
    # f64 too).  Nothing is claimed of them beyond the oracles: finite where f64 is, and judged apart from the case's other elements.
    ex = gc.extrapolated(inp, inverse)
    fin64, fin32 = gc.element_finite(gy64, gp64, Kb, circ), gc.element_finite(gy32, gp32, Kb, circ)
    assert fin64[~ex].all() and fin32[~ex].all()
    assert gc.element_finite(gy, gp, Kb, circ)[fin64].all(), "finite wherever the f64 oracle is"
    away = ~ex
    away[8:32] = False                                        # knot rows: the log-det part jumps across a knot, f32 and f64 disagree on the bin
    same = (i32 == i64) & away
    assert 1.0 - same[away].mean() <= 0.02, "share of elements left out for bin disagreement"
    every = ~ex
    if near_knot is not None:
        same, every = same & ~near_knot, every & ~near_knot
    own = gc.row_relative_errors(gy32, gp32, gy64, gp64, same, Kb, circ)
    k64 = gc.row_relative_errors(gy, gp, gy64, gp64, same, Kb, circ)
    k32 = gc.row_relative_errors(gy, gp, gy32, gp32, every, Kb, circ)
    # the f32 oracle's own error where it CAN be measured on the knot rows too: their elements whose bin both precisions agree on (an
    # input on a knot sits on the end of its bin, where f32 is at its worst under saturated parameters)
    own_all = gc.row_relative_errors(gy32, gp32, gy64, gp64, (i32 == i64) & every, Kb, circ)
    print(f"{tag}: against f64 worst {np.nanmax(k64):.2e} (row {int(np.nanargmax(k64))}) median {np.nanmedian(k64):.2e} | f32 oracle's own "
          f"worst {np.nanmax(own):.2e} median {np.nanmedian(own):.2e} | against the f32 oracle, all rows: worst {np.nanmax(k32):.2e} "
          f"(row {int(np.nanargmax(k32))}) median {np.nanmedian(k32):.2e} | f32 oracle's own with the knot rows: worst {np.nanmax(own_all):.2e}")
    if not np.nanmax(k64) <= FACTOR * np.nanmax(own) + FLOOR:         # say where, before failing
        r = int(np.nanargmax(k64))
        cols = gc.element_columns(Kb, gc.VJP_D, circ)
        for j in range(gc.VJP_D):
            c = cols[j][cols[j] >= 0]
            worst = c[np.argsort(np.abs(gp[r, c].astype(np.float64) - gp64[r, c]))[::-1][:3]]
            print(f"  row {r} dim {j}: y {inp['y'][r, j]!r} bins f32 / f64 {i32[r, j]} / {i64[r, j]} knots {inp['knots'][r, j, i32[r, j]:i32[r, j] + 2]} "
                  f"g_y kernel / f32 / f64 {gy[r, j]:.6g} / {gy32[r, j]:.6g} / {gy64[r, j]:.6g}; columns {worst.tolist()}: kernel "
                  f"{gp[r, worst]} f32 {gp32[r, worst]} f64 {gp64[r, worst]}; element's parameters {inp['params'][r, c]}")
    assert np.nanmax(k64) <= FACTOR * np.nanmax(own) + FLOOR
    assert np.nanmedian(k64) <= FACTOR * np.nanmedian(own) + FLOOR
    # two f32 evaluations of one formula are no farther from each other than from the exact value: the same bound over every row, the
    # yardstick being the oracle's own error over every row it can be measured on
    assert np.nanmax(k32) <= FACTOR * np.nanmax(own_all) + FLOOR
    assert np.nanmedian(k32) <= FACTOR * np.nanmedian(own) + FLOOR
    exm = ex & fin64 & fin32 & (i32 == i64)
    if exm.any():         # the extrapolated elements both oracles are finite on: the same rule, with their own yardstick
        own_ex = np.nanmax(gc.row_relative_errors(gy32, gp32, gy64, gp64, exm, Kb, circ))
        k_ex = np.nanmax(gc.row_relative_errors(gy, gp, gy64, gp64, exm, Kb, circ))
        print(f"{tag}: {int(exm.sum())} extrapolated elements: against f64 worst {k_ex:.2e}, f32 oracle's own {own_ex:.2e}")
        assert k_ex <= FACTOR * own_ex + FLOOR
    if near_knot is not None and near_knot.any():
        # The hardware-form knots are ~1e-7 off the deterministic ones, so for the kernel such an input sits up to KNOT_SHIFT to either
        # side of where the reference sees it.  The input gradient is continuous across the knot (C1) but not flat: under saturated
        # parameters the slope of a minimal-width bin goes from its end value d to ~delta = H / W within a few 1e-8 of the knot (f64
        # oracle: g_y changes by orders of magnitude between an input and its neighbour 2e-7 away).  What can be asked: the kernel's
        # value lies between the exact function's smallest and largest value over that interval, widened by the suite's tolerance.
        lo, hi = np.full(gy.shape, np.inf), np.full(gy.shape, -np.inf)
        span = abs(inp["box"][1] - inp["box"][0]) if inverse else abs(inp["box"][3] - inp["box"][2])
        for k in range(-8, 9):
            moved = dict(inp, y=inp["y"].astype(np.float64) + k / 8.0 * KNOT_SHIFT * span)
            g = gc.vjp_oracle(oracle, moved, Kb, inverse, np.float64)[0]
            lo, hi = np.minimum(lo, g), np.maximum(hi, g)
        scale = np.maximum(np.abs(gy64).max(1, keepdims=True), np.finfo(np.float64).tiny)      # (the dead row's is 0; it is no knot row)

        def outside(g):
            return (np.maximum(np.maximum(lo - g, g - hi), 0.0) / scale)[near_knot]
        # the yardstick, measured the same way: the f32 oracle with its input (equivalently: its knots) moved by the hardware forms' 1e-7
        own_near = max(outside(gc.vjp_oracle(oracle, dict(inp, y=(inp["y"].astype(np.float64) + s * 1e-7 * span).astype(np.float32)), Kb, inverse,
                                             np.float32)[0]).max() for s in (-1.0, 0.0, 1.0))
        out = outside(gy)
        print(f"{tag}: input gradient of the {int(near_knot.sum())} elements within 1e-7 of a knot: worst distance from the f64 oracle's "
              f"range over +-{KNOT_SHIFT:g}: {out.max():.2e} of the row's scale (plain distance at the input itself: "
              f"{(np.abs(gy - gy64) / scale)[near_knot].max():.2e}); the f32 oracle's own, input moved by +-1e-7: {own_near:.2e}")
        assert out.max() <= FACTOR * max(np.nanmax(own), own_near) + FLOOR


def _exact_statements(gy, gp, inp, Kb):
    R = gc.VJP_ROWS
    d = gc.VJP_D
    assert not gy[R["dead"]].any() and not gp[R["dead"]].any(), "both cotangents zero: exact zeros"
    assert not gy[[R["below"], R["above"]]].any(), "a clamped input has no gradient"
    for out, end in ((R["below"], R["clamp_lo"]), (R["above"], R["clamp_hi"])):
        assert np.array_equal(gp[out].view(np.uint32), gp[end].view(np.uint32)), "clamped by the kernel = clamped by the caller"
    slopes = gp[:, 2 * d * Kb:3 * d * Kb]
    assert not (np.signbit(slopes) & (slopes == 0.0)).any(), "-0.0 in a slope column"


@pytest.mark.parametrize("Kb,inverse,circular,scale,box", gc.VJP_CASES)
def test_rqs_backward_per_element_at_knots_ends_and_saturation(hip_lib, oracle, dev, Kb, inverse, circular, scale, box):
    """bgk_rqs_backward (K = 8: register form, K = 6: walked), d = 4, B = 64, rows as in grad_scale_common.vjp_edge_inputs.
    Found here: on the bin's upper end (every input clamped from above) the 1-ulp reciprocal made Q = N / den 1 +- 6e-8 instead of 1, and
    A_th inv (Q - 1) -- the cotangent of the knot below the bin, exactly 0 there -- put 0.96 into height gradients of a row whose largest
    true entry is 0.009 (forward direction, parameter scale 4: 1.1e+02 of the row's scale at K = 8, 1.38 at K = 6, both oracle
    precisions agreeing to 1e-7).  Q is exact there now (bgk_rqs_vjp_bin)."""
    inp = gc.vjp_edge_inputs(oracle, Kb, inverse, circular, scale, box)
    gy, gp = _kernel(inp, Kb, inverse, dev)
    _judge(f"K={Kb} {'inv' if inverse else 'fwd'} {'circ' if circular else 'nc'} scale {scale} box {box}", gy, gp, oracle, inp, Kb, inverse)
    _exact_statements(gy, gp, inp, Kb)


@pytest.mark.parametrize("Kb", [8, 6])
@pytest.mark.parametrize("inverse", [False, True])
def test_masked_out_samples_with_garbage_inputs_give_exact_zeros(hip_lib, oracle, dev, Kb, inverse):
    """the `dead` branch of bgk_rqs_vjp_bin ("masked-out sample: exact zeros, never 0 * inf"): a sample whose cotangents are both zero
    -- discarded by the clipped-energy loss -- contributes nothing whatever its input holds (NaN, +-inf, 1e30: everything behind the
    knots is then NaN or inf, and 0 * NaN is no zero); the rows around it are what they are without it, and so is the published
    maximum"""
    from bgflow_amd.transformer import rqs_backward
    from oracle.oracle import nc_slots
    inp = gc.vjp_edge_inputs(oracle, Kb, inverse, False, 0.7)
    slots = t(nc_slots(inp["circ"], gc.VJP_D), dev)
    cfg = (Kb, inverse, *inp["box"], gc.SETTINGS)

    def run(y, g_out, g_dl):
        buf = torch.zeros(1, device=dev)
        gy, gp = rqs_backward(t(y, dev), t(inp["params"], dev), slots, cfg, t(g_out, dev), t(g_dl, dev), absmax=buf)
        return gy.cpu().numpy(), gp.cpu().numpy(), float(buf)

    rows = [43, 44, 45, 46, 63]
    y, g_out, g_dl = inp["y"].copy(), inp["g_out"].copy(), inp["g_dl"].copy()
    g_out[rows], g_dl[rows] = 0.0, 0.0
    clean = run(y, g_out, g_dl)
    for r, v in zip(rows, (np.nan, np.inf, -np.inf, 1e30, np.nan)):
        y[r] = v
    y[63, 1:] = inp["y"][63, 1:]                     # one garbage element in a row of good ones
    gy, gp, m = run(y, g_out, g_dl)
    assert not gy[rows].any() and not gp[rows].any(), "a masked-out sample contributed"
    assert np.array_equal(gy.view(np.uint32), clean[0].view(np.uint32)) and np.array_equal(gp.view(np.uint32), clean[1].view(np.uint32))
    assert m == clean[2] and np.isfinite(m)


@pytest.mark.parametrize("scale", [0.7, 4.0, 12.0])
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_recompute_backward_lds_forms_at_the_same_edges(hip_lib, oracle, dev, monkeypatch, inverse, circular, scale):
    """The VJP from LDS (bgk_rqs_vjp_element_lds inside bgk_coupling_rqs_dense_h2_backward) on the same rows: a fused spline coupling
    whose output layer has zero weights and the parameter row as bias emits one parameter set for the whole batch, whatever the
    conditioning input.  The rows are built on the knots of the parameters the fused forward actually emits (its split-f16 bias).
    Deterministic forms (bgk_set_option(3, 1)): bit-equal to the stand-alone kernel on the saved parameters.  Shipped hardware forms
    (3 = 2): elements within 1e-7 of a knot are judged on the input gradient and finiteness, every other element by the suite's
    tolerance.
    How the near-knot input gradients are judged: see _judge.  MI355X, forward direction, hardware forms: plain distance from the f64
    oracle at the input itself 4.3 (scale 4) / 3.6e+02 (scale 12) of the row's scale -- the exact function's own variation over the
    knots' 1e-7; distance from the f64 oracle's range over that interval 2.8e-5 - 2.8e-2 (scale 4; the f32 oracle with its input moved:
    4.1e-2 - 0.26) and 3.2e+02 at scale 12, where the f32 oracle is the same 3.2e+02 away (f32 has nothing left there)."""
    import bgflow_amd as bg
    from bgflow_amd import dense, transformer, _lib
    from bgflow_amd.utils import hash_init_, synth
    Kb, d, B, d_c = 8, gc.VJP_D, gc.VJP_B, 9
    circ = np.full(d, circular)
    P = gc.n_params(Kb, circ)
    net = bg.DenseNet([d_c, 128, 128, P], activation=torch.nn.SiLU())
    tr = hash_init_(bg.ConditionalSplineTransformer(net, is_circular=torch.tensor(circ))).to(dev)
    with torch.no_grad():
        net._layers[-1].weight.zero_()
        net._layers[-1].bias.copy_(torch.as_tensor(synth(14, 1, P, scale=scale)[0]))
    x = t(synth(31, B, d_c, uniform=True), dev)
    seen = {}
    real_rqs, real_rc = transformer.rqs_backward, dense._rqs_backward_recompute

    def spy_rqs(y, params, *a, **kw):
        res = real_rqs(y, params, *a, **kw)
        seen.update(params=params, g_p=res[1], form="stand-alone")
        return res

    def spy_rc(*a, **kw):
        res = real_rc(*a, **kw)
        seen.update(g_p=res[1], form="recompute")
        return res
    monkeypatch.setattr(transformer, "rqs_backward", spy_rqs)
    monkeypatch.setattr(dense, "_rqs_backward_recompute", spy_rc)
    monkeypatch.setattr(dense, "PACKED_PARAMS", False)

    def run(y_host, g_out, g_dl, recompute, option):
        monkeypatch.setattr(dense, "RECOMPUTE_PARAMS", recompute)
        old = _lib.lib().bgk_set_option(3, option)
        try:
            y = t(y_host, dev).requires_grad_(True)
            out, dl = tr(x, y, inverse=inverse)
            assert tr._fused_cache.get("params_recompute") is recompute, "the fused training forward must have run in the requested form"
            torch.autograd.backward([out, dl], [t(g_out, dev), t(g_dl, dev)[:, None]])
        finally:
            _lib.lib().bgk_set_option(3, old)
        assert seen["form"] == ("recompute" if recompute else "stand-alone")
        return y.grad.cpu().numpy(), seen["g_p"].cpu().numpy()

    probe = gc.vjp_edge_inputs(oracle, Kb, inverse, circular, scale)
    run(probe["y"], probe["g_out"], probe["g_dl"], False, 2)
    emitted = seen["params"].cpu().numpy()
    assert emitted.shape == (B, P) and np.array_equal(emitted, np.repeat(emitted[:1], B, 0)), "one parameter set for the whole batch"
    assert np.abs(emitted[0] - synth(14, 1, P, scale=scale)[0]).max() <= 2.0 ** -21 * np.abs(emitted[0]).max()
    inp = gc.vjp_edge_inputs(oracle, Kb, inverse, circular, scale, params_row=emitted[0])
    # the knot rows carry no log-det cotangent here: the spline is C1, not C2 -- the output's part of the input gradient is continuous
    # across a knot, the log-det's part jumps, and the hardware-form knots may put such an element into the neighbouring bin (the
    # stand-alone kernel's test above has both cotangents on its knot rows, and the deterministic forms are bit-equal to it)
    full = dict(inp, g_dl=inp["g_dl"].copy())
    inp["g_dl"][8:32] = 0.0
    # (the deterministic forms on the unmodified inputs too -- both cotangents on the knot rows: bit-equal to the stand-alone kernel,
    # and judged like it)
    gy_a, gp_a = run(full["y"], full["g_out"], full["g_dl"], False, 2)
    gy_b, gp_b = run(full["y"], full["g_out"], full["g_dl"], True, 1)
    assert np.array_equal(gy_b.view(np.uint32), gy_a.view(np.uint32)) and np.array_equal(gp_b.view(np.uint32), gp_a.view(np.uint32))
    _judge(f"LDS {'inv' if inverse else 'fwd'} {'circ' if circular else 'nc'} scale {scale} exact, both cotangents on the knot rows", gy_b, gp_b, oracle,
           full, Kb, inverse)
    _exact_statements(gy_b, gp_b, full, Kb)
    gy_s, gp_s = run(inp["y"], inp["g_out"], inp["g_dl"], False, 2)
    gy_e, gp_e = run(inp["y"], inp["g_out"], inp["g_dl"], True, 1)
    assert np.array_equal(gy_e.view(np.uint32), gy_s.view(np.uint32)) and np.array_equal(gp_e.view(np.uint32), gp_s.view(np.uint32))
    gy_f, gp_f = run(inp["y"], inp["g_out"], inp["g_dl"], True, 2)
    interior = inp["knots"][:, :, 1:Kb].astype(np.float64)
    near = np.abs(interior - inp["y"].astype(np.float64)[:, :, None]).min(-1) <= 1e-7
    tag = f"LDS {'inv' if inverse else 'fwd'} {'circ' if circular else 'nc'} scale {scale}"
    _judge(tag + " exact", gy_e, gp_e, oracle, inp, Kb, inverse)
    _judge(tag + " hardware", gy_f, gp_f, oracle, inp, Kb, inverse, near_knot=near)
    for gy, gp in ((gy_e, gp_e), (gy_f, gp_f)):
        _exact_statements(gy, gp, inp, Kb)
