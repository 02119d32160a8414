"""GPU (-m gpu): every activation and output-tanh form of the kernels where it saturates or its exp2 overflows -- pre-activations out to
+-1e4 (and +-1e30 for the layer kernel) -- against f64 references of the same ops: torch's SiLU / Tanh / ReLU on f64 tensors, and for
whole couplings the reference's op chain in f64 (oracle/torch_flow.py).  PyTorch (and bgflow) give +-1 and ~0 there; the forms built on
the hardware exp2 + a Newton-refined reciprocal must too (1 + exp2(..) = +inf once exp2 overflows: 44.36 for tanh, 88.72 for SiLU).
Host-side counterparts (the reproducible forms of bgk_detmath.h): tests/test_host_saturation.py."""
import copy
import warnings

import numpy as np
import pytest
import torch

from test_gpu_round4 import _grad_errors
from test_gpu_round5 import _act_ref
from test_gpu_round6 import _affine_layer, _f64_layer_grads

pytestmark = pytest.mark.gpu

SAT = (0.5, 20.0, 44.0, 44.36, 44.5, 45.0, 50.0, 88.0, 88.72, 89.0, 100.0, 1e4)
S = np.array([v for a in SAT for v in (a, -a)], np.float64)           # the saturation grid: thresholds of both exp2 overflows included


def _kernel_names(run):
    """names of the device kernels ``run`` launches, or None where this box has no kernel tracer (the callers then rely on the caches)"""
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
            run()
            torch.cuda.synchronize()
        names = [e.key for e in prof.key_averages()]
    except Exception:
        run()
        return None
    return names if any("kernel" in n for n in names) else None


def _check_act(y, pre, act, scale):
    """y (f32 result) against act(pre) in f64, elementwise bound 6e-7 scale (the layer kernel's bound, per element instead of the global
    max), finite, tanh exactly +-1 from |pre| = 20 on, SiLU |y| <= 1e-30 below -100"""
    y = np.asarray(y, np.float64)
    ref = _act_ref(pre, act)
    assert np.isfinite(y).all(), f"act {act}: {int((~np.isfinite(y)).sum())} non-finite outputs, e.g. at pre = {pre[~np.isfinite(y)][:4]}"
    err = np.abs(y - ref)
    bad = err > 6e-7 * scale
    assert not bad.any(), f"act {act}: {int(bad.sum())} outside the bound, worst at pre = {pre[bad][np.argmax(err[bad] / scale[bad])]:.6g}"
    if act == 3:
        sat = np.abs(pre) >= 20.0
        assert np.array_equal(y[sat], np.sign(pre[sat]))
    if act == 1:
        assert (np.abs(y[pre <= -100.0]) <= 1e-30).all()


# ---- A. bgk_dense_layer's epilogue (hardware exp2 + refined reciprocal) --------------------------------------------------------------
def _sat_linear(n_in, n_out, w_scale):
    """Linear whose bias walks the saturation grid column by column; small weights (the bias decides the pre-activation)"""
    from bgflow_amd.utils import synth
    lin = torch.nn.Linear(n_in, n_out)
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(synth(3 + n_in + n_out, n_out, n_in, scale=w_scale / np.sqrt(n_in))))
        lin.bias.copy_(torch.as_tensor(np.resize(S, n_out), dtype=torch.float32))
    return lin


def _layer_cases(lin, n_in, act, dev, x_scale=None):
    from bgflow_amd import dense
    from bgflow_amd.utils import synth
    W, b = lin.weight.detach().double().numpy(), lin.bias.detach().double().numpy()
    lin_d = copy.deepcopy(lin).to(dev)
    for B in (1, 37, 1037):
        x = synth(11 + B, B, n_in + 1, scale=1.5)
        if x_scale is not None:
            x = (x * np.resize(x_scale, B)[:, None]).astype(np.float32)
        for view in (lambda t: t[:, :n_in], lambda t: t[:, 1:]):       # aligned rows / rows shifted by 4 bytes
            xv = view(torch.as_tensor(x, device=dev))
            with torch.no_grad():
                y = dense.dense_layer(xv, lin_d, act)
            x64 = view(torch.as_tensor(x)).double().numpy()
            pre = x64 @ W.T + b
            scale = np.abs(x64) @ np.abs(W).T + np.abs(b)
            assert y.shape == (B, lin.out_features)
            yield y.cpu().numpy(), pre, scale
    assert "_bgk_layer_ops" in lin_d.__dict__, "the Linear did not run on bgk_dense_layer"


@pytest.mark.parametrize("n_in", [16, 64, 256, 300, 700])
@pytest.mark.parametrize("n_out", [7, 130, 425])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_dense_layer_epilogue_at_saturation(hip_lib, dev, n_in, n_out, act):
    """y = act(x W^T + b) on bgk_dense_layer with pre-activations over the saturation grid (set through the bias, one value per output
    column): single-pass instances and accumulating passes (n_in > 256: the activation runs on the last pass only), one to four 128-row
    groups, partial tiles, aligned and shifted rows; then x scaled per row so that the products themselves reach +-1e4"""
    with np.errstate(over="ignore"):
        for y, pre, scale in _layer_cases(_sat_linear(n_in, n_out, 1e-2), n_in, act, dev):
            _check_act(y, pre, act, scale)
        rows = np.array([1.0, 30.0, 600.0, 3e3, 1e4 * np.sqrt(n_in) / 12.0])
        for y, pre, scale in _layer_cases(_sat_linear(n_in, n_out, 10.0), n_in, act, dev, x_scale=rows):
            _check_act(y, pre, act, scale)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_dense_layer_epilogue_without_the_lds_bias(hip_lib, dev, act):
    """a layer wide enough (256 -> 7800: 61 row groups) that the bias does not fit behind the waves' tiles in LDS: the epilogue's
    per-element bias loads, same saturation grid"""
    n_in, n_out = 256, 7800
    xs, ys = 16 * n_in + 4, 128 + 4                                 # launch_layer (bgk_dense_layer.hip): 4 waves x 32 rows of x / y
    assert 4 * 4 * 32 * max(xs, ys) + 4 * 128 * ((n_out + 127) // 128) > 160 * 1024, "the case must leave the bias in global memory"
    with np.errstate(over="ignore"):
        for y, pre, scale in _layer_cases(_sat_linear(n_in, n_out, 1e-2), n_in, act, dev):
            _check_act(y, pre, act, scale)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_dense_layer_epilogue_at_1e30(hip_lib, dev, act):
    """pre-activations of +-1e30: finite, the sign of torch's result, within 1e-4 (relative above 1) of it"""
    from bgflow_amd import dense
    lin = _sat_linear(64, 130, 1e-2)
    with torch.no_grad():
        lin.bias.copy_(torch.as_tensor(np.resize([1e30, -1e30, 3e29, -5e29], 130), dtype=torch.float32))
    x = torch.randn(37, 64, generator=torch.Generator().manual_seed(5))
    ref = {0: lambda v: v, 1: torch.nn.functional.silu, 2: torch.relu, 3: torch.tanh}[act](x.double() @ lin.weight.double().T + lin.bias.double())
    with torch.no_grad():
        y = dense.dense_layer(x.to(dev), lin.to(dev), act).double().cpu()
    assert torch.isfinite(y).all()
    assert torch.equal(torch.sign(y), torch.sign(ref)) or act == 1                 # (SiLU(-1e30): -0 or a tiny negative, both ~0)
    assert ((y - ref).abs() <= 1e-4 * ref.abs().clamp(min=1.0)).all()


# ---- B. a whole DenseNet outside the fused envelopes: the no-grad epilogue vs the grad-mode _ActFn (bgk_activation) -------------------
def test_densenet_eval_and_train_agree_at_saturation(hip_lib, dev):
    """[23, 300, 96, 51] with SiLU then Tanh, hidden biases over the saturation grid on a subset of units (the next layer's weights from
    those units scaled down so that the Tanh units' pre-activations stay where the biases put them): the no-grad forward (fused epilogue)
    and the grad-mode forward (_ActFn) agree; both match f64; parameter and input gradients match f64 autograd; the saturated Tanh units
    pass exactly zero gradient to their biases, as f64 does"""
    import bgflow_amd as bg
    from bgflow_amd.utils import hash_init_, synth
    net = hash_init_(bg.DenseNet([23, 300, 96, 51], activation=[torch.nn.SiLU(), torch.nn.Tanh()]))
    lin0, lin1 = net._layers[0], net._layers[2]
    u0, u1 = np.arange(0, 300, 7)[:S.size], np.arange(1, 96, 4)[:S.size]
    with torch.no_grad():
        lin0.bias[u0] = torch.as_tensor(S[:u0.size], dtype=torch.float32)
        lin1.weight[:, u0] *= 1e-4
        lin1.bias[u1] = torch.as_tensor(S[:u1.size], dtype=torch.float32)
    net = net.to(dev)
    net64 = copy.deepcopy(net).cpu().double()
    B = 1037
    x = torch.as_tensor(synth(21, B, 23), dtype=torch.float64)
    w = torch.as_tensor(synth(22, B, 51), dtype=torch.float64) / B
    x64 = x.clone().requires_grad_(True)
    y64 = net64(x64)
    (y64 * w).sum().backward()
    with torch.no_grad():
        y_eval = net(x.float().to(dev))
    assert all("_bgk_layer_ops" in m.__dict__ for m in net._layers if isinstance(m, torch.nn.Linear))
    xg = x.float().to(dev).requires_grad_(True)
    names = _kernel_names(lambda: net(xg))
    if names is not None:
        assert any("act_kernel" in n or "act_scalar_kernel" in n for n in names), names          # bgk_activation
    y = net(xg)
    ymax = max(1.0, float(y64.detach().abs().max()))
    assert torch.isfinite(y_eval).all() and torch.isfinite(y).all()
    assert float((y_eval - y.detach()).abs().max()) <= 2e-6 * ymax, "no-grad and grad-mode forward disagree"
    for got in (y_eval, y.detach()):
        assert float((got.double().cpu() - y64.detach()).abs().max()) <= 1e-5 * ymax
    (y * w.float().to(dev)).sum().backward()
    got = {n: p.grad.double().cpu() for n, p in net.named_parameters()}
    ref = {n: p.grad for n, p in net64.named_parameters()}
    assert all(torch.isfinite(g).all() for g in got.values()) and torch.isfinite(xg.grad).all()
    rel, worst = _grad_errors(got, ref)
    ex = float((xg.grad.double().cpu() - x64.grad).norm() / x64.grad.norm())
    assert rel <= 5e-5 and ex <= 5e-5, (rel, worst, ex)
    sat1 = u1[np.abs(S[:u1.size]) >= 44.0]
    assert bool((net64._layers[2].bias.grad[sat1] == 0).all()), "f64 reference: saturated tanh units pass no gradient"
    assert bool((net._layers[2].bias.grad[sat1] == 0).all()), net._layers[2].bias.grad[sat1]


# ---- C. affine couplings whose log sigma saturates (output tanh of the scale network) ------------------------------------------------
LOG_SIGMA_BIAS = (45.0, -60.0, 100.0, -1e4, -45.0, 60.0, -100.0, 1e4)


def _scale_out(tr):
    net = tr._scale_transformation
    return getattr(net, "net", net)._layers[-1]


def _saturate_log_sigma(flow):
    """every other output dim of the scale network gets a bias from LOG_SIGMA_BIAS (the layer's weights stay at the hash-init scale,
    ~0.15: the ratio of its largest to its typical entry stays near 2^16, within the split-f16 operands' shared power-of-two scale)"""
    last = _scale_out(flow[0].transformer)
    sat = np.arange(0, last.out_features, 2)
    with torch.no_grad():
        last.bias[sat] = torch.as_tensor(np.resize(LOG_SIGMA_BIAS, sat.size), dtype=torch.float32)
    return sat


def _mc_affine_layer(n_c, hidden, d, acts, **kw):
    """an affine coupling conditioned on two tensors (n_c and n_c + 3 features): the _mc entry points read them unconcatenated"""
    import bgflow_amd as bg
    from bgflow_amd.utils import hash_init_
    net = lambda a: bg.DenseNet([2 * n_c + 3, *hidden, d], activation=a())           # noqa: E731
    tr = bg.AffineTransformer(shift_transformation=net(acts[0]), scale_transformation=net(acts[1]), **kw)
    return hash_init_(bg.SequentialFlow([bg.CouplingFlow(tr, transformed_indices=[2], cond_indices=[0, 1])]), scale=1.5)


INFER = [
    # (id, n_c, hidden, d, acts, periodic, two conditioning tensors, expected kernel (substring) or None, plan check)
    ("h2-w64", 32, (64, 64), 32, (torch.nn.ReLU, torch.nn.Tanh), False, False, None, lambda p: p["hidden"] == 64 and p["depth"] == 3),
    ("h2-w128-v2", 17, (128, 128), 24, (torch.nn.ReLU, torch.nn.Tanh), False, False, "affine_dense_v2", lambda p: p["depth"] == 3),
    ("h2-w128-stream", 17, (128, 128), 24, (torch.nn.SiLU, torch.nn.Tanh), False, False, "!affine_dense_v2", lambda p: p["depth"] == 3),
    ("h3-w128-v2", 17, (128, 128, 128), 24, (torch.nn.ReLU, torch.nn.Tanh), False, False, "affine_dense_v2", lambda p: p["depth"] == 4),
    ("h3-w128-stream", 17, (128, 128, 128), 24, (torch.nn.SiLU, torch.nn.Tanh), False, False, "!affine_dense_v2",
     lambda p: p["depth"] == 4),
    ("deep-4", 12, (4,), 20, (torch.nn.ReLU, torch.nn.Tanh), False, False, "affine_deep", lambda p: p["anydepth"]),
    ("deep-48x5", 12, (48,) * 5, 20, (torch.nn.ReLU, torch.nn.Tanh), False, False, "affine_deep", lambda p: p["anydepth"]),
    ("mc-w128", 9, (128, 128), 17, (torch.nn.SiLU, torch.nn.SiLU), False, True, None, lambda p: p["hidden"] == 128),
    ("periodic-w128", 17, (128, 128), 66, (torch.nn.SiLU, torch.nn.SiLU), True, False, None, lambda p: p["periodic"]),
    ("periodic-w64", 16, (64, 64), 30, (torch.nn.ReLU, torch.nn.Tanh), True, False, None, lambda p: p["periodic"] and p["hidden"] == 64),
]


def _infer_inputs(n_c, d, periodic, mc, B, seed):
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)) if periodic else \
        (lambda *s: torch.randn(*s, generator=g, dtype=torch.float64))
    cond = [draw(B, n_c), draw(B, n_c + 3)] if mc else [draw(B, n_c)]
    return cond + [torch.randn(B, d, generator=g, dtype=torch.float64)]


def _check_affine_out(out, dl, ref_out, ref_dl, what):
    assert torch.isfinite(out).all() and torch.isfinite(dl).all(), f"{what}: non-finite outputs"
    assert float((out.double().cpu() - ref_out).abs().max()) <= 2e-5 * max(1.0, float(ref_out.abs().max())), what
    assert float((dl.double().cpu() - ref_dl).abs().max()) <= 1e-5 * max(1.0, float(ref_dl.abs().max())), what


@pytest.mark.parametrize("case", INFER, ids=[c[0] for c in INFER])
@pytest.mark.parametrize("preserve_volume", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_affine_inference_with_saturated_log_sigma(hip_lib, dev, case, preserve_volume, inverse):
    """one fused affine coupling per kernel family (no grad) with half of the scale network's outputs at |s| >= 45: y' and dlogp
    against the reference's op chain in f64 (bounds of the training-layer test), all finite"""
    from oracle import torch_flow as tfl
    name, n_c, hidden, d, acts, periodic, mc, kern, plan_ok = case
    flow = (_mc_affine_layer(n_c, hidden, d, acts, preserve_volume=preserve_volume) if mc else
            _affine_layer(n_c, hidden, d, acts, periodic, preserve_volume=preserve_volume))
    _saturate_log_sigma(flow)
    flow_cpu = copy.deepcopy(flow).double()
    flow = flow.to(dev)
    xs = _infer_inputs(n_c, d, periodic, mc, 1037, 17 + d)
    with torch.no_grad():
        ref_outs, ref_dl = tfl.run_flow(flow_cpu, xs, inverse=inverse)
    xd = [v.float().to(dev) for v in xs]
    res = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # a rejection (RuntimeWarning) would mean the unfused path ran
        with torch.no_grad():
            names = _kernel_names(lambda: res.append(flow(*xd, inverse=inverse)))
    *outs, dl = res[-1]
    plan = flow[0].transformer._fused_cache
    assert plan.get("packed") is not None and plan_ok(plan), f"{name}: the fused plan did not run as intended"
    if kern is not None and names is not None:
        hit = any(kern.lstrip("!") in n for n in names)
        assert hit != kern.startswith("!"), (name, [n for n in names if "affine" in n])
    _check_affine_out(outs[-1], dl, ref_outs[-1], ref_dl, name)


TRAIN = [
    # (id, n_c, hidden, d, acts): fwd64 + bwd64 (cfg 2's couplings) / the one-launch width-128 training forward (cfg 5)
    ("fwd64-bwd64", 32, (64, 64), 32, (torch.nn.ReLU, torch.nn.Tanh)),
    ("h2-train", 43, (128, 128), 66, (torch.nn.SiLU, torch.nn.SiLU)),
]


def _train_case(dev, n_c, hidden, d, acts, preserve_volume, inverse, allow_fused=True, B=777):
    flow = _affine_layer(n_c, hidden, d, acts, preserve_volume=preserve_volume)
    sat = _saturate_log_sigma(flow)
    flow_cpu = copy.deepcopy(flow).double()
    flow = flow.to(dev)
    tr = flow[0].transformer
    tr.allow_fused = allow_fused
    g = torch.Generator().manual_seed(B + d)
    x, y = torch.randn(B, n_c, generator=g, dtype=torch.float64), torch.randn(B, d, generator=g, dtype=torch.float64)
    wy = torch.randn(B, d, generator=g, dtype=torch.float64) / B
    wl = torch.randn(B, 1, generator=g, dtype=torch.float64) / B
    ref_out, ref_dl, ref_gx, ref_gy, ref_gp = _f64_layer_grads(flow_cpu, x, y, wy, wl, inverse)
    xg, yg = x.float().to(dev).requires_grad_(True), y.float().to(dev).requires_grad_(True)
    _, out, dl = flow(xg, yg, inverse=inverse)
    used = bool(tr.__dict__.get("_train_cache", {}).get("train_used"))
    _check_affine_out(out.detach(), dl.detach(), ref_out, ref_dl, "training forward")
    ((out * wy.float().to(dev)).sum() + (dl * wl.float().to(dev)).sum()).backward()
    got = {n: p.grad.double().cpu() for n, p in flow.named_parameters() if p.grad is not None}
    assert set(got) == set(ref_gp)
    assert all(torch.isfinite(v).all() for v in got.values()) and torch.isfinite(xg.grad).all() and torch.isfinite(yg.grad).all()
    rel, worst = _grad_errors(got, {n: ref_gp[n] for n in got})
    assert rel <= 5e-5, (rel, worst)
    for name, a, b in (("g_x", xg.grad, ref_gx), ("g_y", yg.grad, ref_gy)):
        err = float((a.double().cpu() - b).norm() / max(float(b.norm()), 1e-30))
        assert err <= 5e-5, f"{name}: relative L2 {err:.2e}"
    # the saturated dims' scale-network outputs receive exactly zero gradient (f64: 1 - tanh^2 = 0 there): their bias and weight rows
    last, last64 = _scale_out(tr), _scale_out(flow_cpu[0].transformer)
    assert bool((last64.bias.grad[sat] == 0).all())
    assert bool((last.bias.grad[sat] == 0).all()) and bool((last.weight.grad[sat] == 0).all()), last.bias.grad[sat]
    return used


@pytest.mark.parametrize("case", TRAIN, ids=[c[0] for c in TRAIN])
@pytest.mark.parametrize("preserve_volume", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_affine_training_with_saturated_log_sigma(hip_lib, dev, case, preserve_volume, inverse):
    """the fused affine training path (forward kernel + hand-written backward) with half of log sigma saturated: outputs, dlogp and
    every gradient against f64 autograd (bounds of test_affine_coupling_training_layer_against_f64_autograd), all finite"""
    name, n_c, hidden, d, acts = case
    assert _train_case(dev, n_c, hidden, d, acts, preserve_volume, inverse), f"{name}: the fused training path did not run"


@pytest.mark.parametrize("preserve_volume", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_affine_unfused_control_with_saturated_log_sigma(hip_lib, dev, preserve_volume, inverse):
    """allow_fused = False: conditioner networks + bgk_affine_transform / bgk_affine_backward, same bounds (a control)"""
    assert not _train_case(dev, 32, (64, 64), 32, (torch.nn.ReLU, torch.nn.Tanh), preserve_volume, inverse, allow_fused=False)


# ---- D. hidden activations of the fused couplings at saturation (believed safe: pinned) ------------------------------------------------
def _saturate_hidden(net, values, damp=1e-3):
    """the first hidden layer's biases on every fifth unit take ``values``; the next layer's weights from those units are scaled by
    ``damp`` so that the downstream parameters stay in the range the unsaturated bounds are set for"""
    net = getattr(net, "net", net)
    lin0, lin1 = net._layers[0], net._layers[2]
    units = np.arange(0, lin0.out_features, 5)
    with torch.no_grad():
        lin0.bias[units] = torch.as_tensor(np.resize(values, units.size), dtype=torch.float32)
        lin1.weight[:, units] *= damp


HIDDEN_VALUES = {torch.nn.SiLU: S, torch.nn.Tanh: S, torch.nn.ReLU: np.array([0.5, -0.5, 20.0, -100.0, 1e3, -1e3, 1e4, -1e4])}


@pytest.mark.parametrize("tag", ["w256", "deep3"])
@pytest.mark.parametrize("act", [torch.nn.SiLU, torch.nn.Tanh, torch.nn.ReLU])
def test_spline_coupling_hidden_activations_at_saturation(hip_lib, dev, tag, act):
    """fused spline couplings (tests/envelope_layers.py: hidden (256, 256) and three hidden layers of 128) with first-layer biases over
    the saturation grid: both directions against the reference's op chain in f64 within the envelope test's bounds, all finite"""
    import envelope_layers as el
    from oracle import torch_flow as tfl
    import bgflow_amd as bg
    hidden = el.SPLINE[tag]
    layer = el.spline_layer(hidden, False, False)
    net = layer.transformer._params_net
    for i, m in enumerate(net._layers):
        if isinstance(m, torch.nn.SiLU):
            net._layers[i] = act()
    _saturate_hidden(net, HIDDEN_VALUES[act])
    flow_cpu = bg.SequentialFlow([copy.deepcopy(layer).double()])
    layer = layer.to(dev)
    c, y = (torch.as_tensor(v) for v in el.spline_inputs(False))
    with torch.no_grad():
        (_, z64), dl64 = tfl.run_flow(flow_cpu, [c.double(), y.double()])
        (_, back64), dli64 = tfl.run_flow(flow_cpu, [c.double(), z64], inverse=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # a rejection (RuntimeWarning) would mean the layer-by-layer path ran
            _, z, dl = layer(c.to(dev), y.to(dev))
            _, yb, dli = layer(c.to(dev), z64.float().to(dev), inverse=True)
    plan = layer.transformer._fused_cache
    assert (plan.get("hidden") == 256) if tag.startswith("w") else (plan.get("deep") == len(hidden)), plan.keys()
    for a in (z, dl, yb, dli):
        assert torch.isfinite(a).all()
    np.testing.assert_allclose(z.cpu().numpy(), z64.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(dl.cpu().numpy(), dl64.numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(yb.cpu().numpy(), back64.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(dli.cpu().numpy(), dli64.numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("case", TRAIN + [("h2-w64-infer", 32, (64, 64), 32, (torch.nn.ReLU, torch.nn.Tanh))], ids=lambda c: c[0])
@pytest.mark.parametrize("act", [torch.nn.SiLU, torch.nn.Tanh, torch.nn.ReLU])
def test_affine_coupling_hidden_activations_at_saturation(hip_lib, dev, case, act):
    """fused affine couplings, inference and training, both conditioners' first hidden layers partly saturated: forward against the
    f64 op chain and gradients against f64 autograd within the training-layer bounds, all finite"""
    name, n_c, hidden, d, _ = case
    flow = _affine_layer(n_c, hidden, d, (act, act))
    tr = flow[0].transformer
    for net in (tr._shift_transformation, tr._scale_transformation):
        _saturate_hidden(net, HIDDEN_VALUES[act])
    flow_cpu = copy.deepcopy(flow).double()
    flow = flow.to(dev)
    B = 513
    g = torch.Generator().manual_seed(B + d)
    x, y = torch.randn(B, n_c, generator=g, dtype=torch.float64), torch.randn(B, d, generator=g, dtype=torch.float64)
    wy, wl = torch.randn(B, d, generator=g, dtype=torch.float64) / B, torch.randn(B, 1, generator=g, dtype=torch.float64) / B
    for inverse in (False, True):
        ref_out, ref_dl, ref_gx, ref_gy, ref_gp = _f64_layer_grads(flow_cpu, x, y, wy, wl, inverse)
        with torch.no_grad():
            _, out_inf, dl_inf = flow(x.float().to(dev), y.float().to(dev), inverse=inverse)
        assert flow[0].transformer._fused_cache.get("packed") is not None
        _check_affine_out(out_inf, dl_inf, ref_out, ref_dl, f"{name} inference")
        if name.endswith("infer"):
            continue
        flow.zero_grad()
        xg, yg = x.float().to(dev).requires_grad_(True), y.float().to(dev).requires_grad_(True)
        _, out, dl = flow(xg, yg, inverse=inverse)
        assert tr._train_cache.get("train_used"), "the fused training path did not run"
        _check_affine_out(out.detach(), dl.detach(), ref_out, ref_dl, f"{name} training")
        ((out * wy.float().to(dev)).sum() + (dl * wl.float().to(dev)).sum()).backward()
        got = {n: p.grad.double().cpu() for n, p in flow.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(v).all() for v in got.values())
        rel, worst = _grad_errors(got, {n: ref_gp[n] for n in got})
        assert rel <= 5e-5, (name, inverse, rel, worst)
        for gname, a, b in (("g_x", xg.grad, ref_gx), ("g_y", yg.grad, ref_gy)):
            err = float((a.double().cpu() - b).norm() / max(float(b.norm()), 1e-30))
            assert err <= 5e-5, f"{name}: {gname}: relative L2 {err:.2e}"
