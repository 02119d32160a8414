"""GPU: a spline coupling layer in which every scalar of the call is distinct -- left, right, bottom, top, min_bin_width,
min_bin_height and min_derivative all differ (the other GPU tests use [0, 1] x [0, 1] and 1e-3 three times, so two of them swapped
anywhere between the C ABI and a kernel would pass there).  Both directions through every path that carries the eight scalars,
against the reference's op chain in f64 (oracle/torch_flow.py) with the bounds the tests of each path already use
(tests/test_gpu_parity.py, test_gpu_spline_regparams.py, test_gpu_round5.py, test_gpu_round6.py); bin indices against the f32 oracle.

d = 7: two parameter chunks of 5 dims, the second one partial; d_c = 6; B = 269: two workgroups of 4 x 32 samples and a ragged tail of
13 rows -- the smallest shapes that reach the chunk loop, the last-tile count and the row guard."""
import copy

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import dense
from bgflow_amd.utils import hash_init_, synth
from test_gpu_parity import assert_bin_ties, rel_per_sample
from test_gpu_round4 import _grad_errors

pytestmark = pytest.mark.gpu

BOX = dict(left=-1.25, right=2.5, bottom=0.5, top=3.0)
SETTINGS = dict(min_bin_width=2e-3, min_bin_height=5e-3, min_derivative=3e-3, enable_identity_init=True)
D, D_C, B = 7, 6, 269
CIRC = np.array([j % 3 != 1 for j in range(D)])

# path -> (hidden layers, bins, conditioning widths, gemm_mode, REGISTER_PARAMS)
PATHS = {
    "f16x2-regparams": ((128, 128), 8, (D_C,), "f16x2", True),
    "f16x2-order1": ((128, 128), 8, (D_C,), "f16x2", False),
    "f16x2-mc": ((128, 128), 8, (2, 4), "f16x2", True),
    "f32": ((128, 128), 8, (D_C,), "f32", True),
    "K4": ((128, 128), 4, (D_C,), "f16x2", True),
    "w256": ((256, 256), 8, (D_C,), "f16x2", True),
    "deep3": ((128, 128, 128), 8, (D_C,), "f16x2", True),
}


def _layer(hidden=(128, 128), K=8, cond_widths=(D_C,), mode="f16x2", dev=None):
    net = bg.DenseNet([sum(cond_widths), *hidden, 3 * K * D + int((~CIRC).sum())], activation=torch.nn.SiLU())
    tr = bg.ConditionalSplineTransformer(params_net=net, is_circular=torch.tensor(CIRC), **BOX)
    tr._default_settings.update(SETTINGS)
    tr.gemm_mode = mode
    layer = hash_init_(bg.CouplingFlow(tr, transformed_indices=[0], cond_indices=list(range(1, 1 + len(cond_widths)))))
    return layer.to(dev) if dev is not None else layer


def _inputs(inverse, cond_widths=(D_C,)):
    """y inside the domain both directions share with the reference -- bgflow's forward searches the heights on [bottom, top] after
    the clamp to [left, right], its inverse the widths on [left, right] -- and a few elements outside [left, right]: clamped"""
    u = synth(B + 11, B, D, uniform=True)
    if inverse:
        y = (BOX["left"] + (BOX["right"] - BOX["left"]) * u).astype(np.float32)
        y[3, 0], y[140, 6], y[268, 3] = -1.5, 2.75, -1.25
    else:
        y = (BOX["bottom"] + (BOX["right"] - BOX["bottom"]) * u).astype(np.float32)
        y[3, 0], y[140, 6], y[268, 3] = 2.625, 2.75, 0.5
    cond = synth(B + 7, B, sum(cond_widths), uniform=True)
    return [y] + [np.ascontiguousarray(c) for c in np.split(cond, np.cumsum(cond_widths)[:-1], axis=1)]


_REF = {}


def _reference(layer_cpu, key, xs, inverse):
    """(out, dlogp) of the reference's op chain in f64 and the f32 oracle's bin indices / knots; computed once per layer and direction"""
    if key not in _REF:
        from oracle import flow_oracle as fo, torch_flow as tfl
        with torch.no_grad():
            outs, dl = tfl.run_block(copy.deepcopy(layer_cpu).double(), [torch.as_tensor(v).double() for v in xs], inverse)
        trace = []
        fo.run_block(layer_cpu, xs, inverse, np.float32, trace)
        _REF[key] = (outs[0].numpy(), dl.numpy(), trace[0])
    return _REF[key]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("path", list(PATHS))
def test_every_inference_path_with_a_distinct_box(hip_lib, dev, path, inverse):
    hidden, K, widths, mode, regp = PATHS[path]
    layer_cpu, layer = _layer(hidden, K, widths, mode), _layer(hidden, K, widths, mode, dev)
    xs = _inputs(inverse, widths)
    out64, dl64, det = _reference(layer_cpu, (hidden, K, widths, mode, inverse), xs, inverse)
    tr = layer.transformer
    tr.return_bin_indices = True
    prev = dense.REGISTER_PARAMS
    try:
        dense.REGISTER_PARAMS = regp
        with torch.no_grad():
            out, *_, dl = layer(*[torch.as_tensor(v).to(dev) for v in xs], inverse=inverse)
    finally:
        dense.REGISTER_PARAMS = prev
    plan = tr._fused_cache
    assert plan.get("mode") == mode and plan.get("n_bins") == K and plan.get("hidden") == max(hidden), "the fused path must have run"
    assert bool(plan.get("deep")) == (len(hidden) == 3)
    if mode == "f16x2" and K == 8 and hidden == (128, 128):
        assert (plan.get("regp_version") == plan["version"]) == regp, "operands in the requested row order must have been used"
    out, dl, idx = out.cpu().numpy(), dl.cpu().numpy(), tr.last_bin_indices.cpu().numpy()
    e_out, e_dl = np.abs(out - out64).max(), rel_per_sample(dl, dl64, floor=1.0).max()
    print(f"{path} inverse={inverse}: outputs {e_out:.2e}, log-det per sample {e_dl:.2e} (absolute {np.abs(dl - dl64).max():.2e})")
    if mode == "f32":                      # tests/test_gpu_parity.py::test_fused_layer_bit_exact_vs_oracle: the f32 oracle bit for bit
        from oracle import flow_oracle as fo
        fo.MFMA_ORDER = True
        try:
            trace = []
            outs_o, dl_o = fo.run_block(layer_cpu, xs, inverse, np.float32, trace)
        finally:
            fo.MFMA_ORDER = False
        assert np.array_equal(idx, trace[0]["bin_idx"]) and np.array_equal(out, outs_o[0]) and np.array_equal(dl, dl_o)
        return
    if path in ("w256", "deep3"):          # tests/test_gpu_round5.py: the width-256 and the any-depth kernel
        np.testing.assert_allclose(out, out64, rtol=0, atol=2e-5)
        np.testing.assert_allclose(dl, dl64, rtol=2e-5, atol=2e-5)
    else:                                  # tests/test_gpu_parity.py, tests/test_gpu_spline_regparams.py
        assert e_out <= 1e-6, f"outputs {e_out:.2e} from the f64 reference"
        assert e_dl <= 1e-5, f"log-det per sample {e_dl:.2e}"
    n_ties = assert_bin_ties(idx, det, xs[0], path)
    assert n_ties <= max(2, idx.size // 10000)


@pytest.mark.parametrize("inverse", [False, True])
def test_stand_alone_spline_kernel_with_a_distinct_box(hip_lib, dev, inverse):
    """bgk_rqs_transform on the parameters of the layer's conditioner: the C oracle's f32 element routine bit for bit, within f32
    conditioning of the f64 reference (tests/test_gpu_round5.py::test_spline_backward_for_any_bin_count)"""
    from bgflow_amd.transformer import rqs_transform
    from oracle import oracle as co
    layer_cpu = _layer()
    xs = _inputs(inverse)
    out64, dl64, _ = _reference(layer_cpu, ("stand-alone", inverse), xs, inverse)
    with torch.no_grad():
        params = layer_cpu.transformer._params_net(torch.as_tensor(xs[1])).numpy()
    slots = np.full(D, -1, np.int32)
    slots[~CIRC] = np.arange(int((~CIRC).sum()), dtype=np.int32)
    z, dl = rqs_transform(torch.as_tensor(xs[0]).to(dev), torch.as_tensor(params).to(dev), torch.as_tensor(slots).to(dev), 8, inverse,
                          BOX["left"], BOX["right"], BOX["bottom"], BOX["top"], SETTINGS)
    z_c, dl_c = co.rqs(xs[0], params, is_circular=CIRC, inverse=inverse, n_bins=8, identity_init=True, **BOX,
                       **{k: v for k, v in SETTINGS.items() if k != "enable_identity_init"})
    assert np.array_equal(z.cpu().numpy(), z_c) and np.array_equal(dl.cpu().numpy().reshape(-1), dl_c.reshape(-1))
    assert np.abs(z.cpu().numpy() - out64).max() < 1e-5


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("recompute", [True, False])
def test_training_layer_with_a_distinct_box_against_f64_autograd(hip_lib, dev, recompute, inverse):
    """the fused training forward and its backward (spline parameters recomputed from z1, or saved): values and every gradient against
    f64 autograd of the reference's op chain with the bounds of tests/test_gpu_round6.py's training layers (5e-5 relative L2)"""
    from oracle import torch_flow as tfl
    layer = _layer(dev=dev)
    ref = copy.deepcopy(layer).cpu().double()
    xs = _inputs(inverse)
    wy, wl = synth(B + 1, B, D) / B, synth(B + 2, B, 1) / B
    xs64 = [torch.as_tensor(v).double().requires_grad_(True) for v in xs]
    with torch.enable_grad():
        outs, dl64 = tfl.run_block(ref, xs64, inverse, grad=True)
        ((outs[0] * torch.as_tensor(wy).double()).sum() + (dl64 * torch.as_tensor(wl).double()).sum()).backward()
    prev = dense.RECOMPUTE_PARAMS
    try:
        dense.RECOMPUTE_PARAMS = recompute
        xg = [torch.as_tensor(v).to(dev).requires_grad_(True) for v in xs]
        out, _, dl = layer(*xg, inverse=inverse)
        plan = layer.transformer._fused_cache
        assert plan.get("train_used") and plan.get("params_recompute") is recompute, "the fused training forward must have run in the requested form"
        ((out * torch.as_tensor(wy).to(dev)).sum() + (dl * torch.as_tensor(wl).to(dev)).sum()).backward()
    finally:
        dense.RECOMPUTE_PARAMS = prev
    ref_out, ref_dl = outs[0].detach(), dl64.detach()
    assert float((out.double().cpu() - ref_out).abs().max()) <= 2e-5 * max(1.0, float(ref_out.abs().max()))
    assert float((dl.double().cpu() - ref_dl).abs().max()) <= 1e-5 * max(1.0, float(ref_dl.abs().max()))
    got = {n: p.grad.double().cpu() for n, p in layer.named_parameters()}
    rel, worst = _grad_errors(got, {n: p.grad for n, p in ref.named_parameters()})
    print(f"training layer recompute={recompute} inverse={inverse}: flat parameter gradient rel L2 {rel:.2e}, worst {worst[1]} {worst[0]:.2e}")
    assert rel <= 5e-5 and worst[0] <= 3e-4
    for name, a, b in (("g_y", xg[0].grad, xs64[0].grad), ("g_x", xg[1].grad, xs64[1].grad)):
        err = float((a.double().cpu() - b).norm() / max(float(b.norm()), 1e-30))
        assert err <= 5e-5, f"{name}: relative L2 {err:.2e}"
    assert float(xg[0].grad[3, 0]) == 0.0, "a clamped input has no gradient"
