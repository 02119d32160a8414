"""GPU (-m gpu): the fused backward of the stochastic layers -- the pair Hessian-vector product bgk_pair_energy_hvp (csrc/bgk_pair.hip), the
recording forward bgk_pair_langevin_record and the adjoint sweep bgk_pair_langevin_backward (csrc/bgk_langevin.hip) behind
``BrownianFlow`` / ``LangevinFlow`` / ``MetropolisMCFlow`` with ``fused_backward = True`` -- against the reference's f64 autograd on fixed
random numbers (tests/golden/stochastic_grad.npz, written by tests/golden/make_stochastic_grad_goldens.py) and bitwise against itself.

Bound of the parity tests, the project's own: |got - f64| <= 4 err_32 + 1e-6 (1 + |f64|), err_32 the error of the reference's own f32
evaluation of the same quantity.  B = 150: several tiles and a partial last one at every tile height (64 rows; 21 / 16 rows at n d = 192)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import particles, stochastic
from bgflow_amd.distributions import Energy, _kernel_plan

from stochastic_backward_common import (HVP_CASES, LAYER_CASES, build_grad, flow_seed, grad_key, philox_normals, same_bits, vectors,
                                        within)
from stochastic_common import B, MC_STEPS, build, case_key, make, normals, start_velocities

pytestmark = pytest.mark.gpu

FN = {"brownian": "_BrownianFnBackward", "langevin": "_LangevinFnBackward"}


def loss_grads(flow, xs):
    """the outputs' grad_fn name and d (dW.sum() + outputs.sum()) / d inputs"""
    *ys, dW = flow(*xs)
    return type(ys[0].grad_fn).__name__, torch.autograd.grad(dW.sum() + sum(y.sum() for y in ys), xs)


def forbid_the_torch_formulas(monkeypatch):
    def raiser(*args, **kwargs):
        raise AssertionError("Energy.energy: the torch formulas of the energy were asked for")
    monkeypatch.setattr(Energy, "energy", raiser)


@pytest.mark.parametrize("kind,n,d", HVP_CASES)
def test_pair_hessian_vector_product(hip_lib, dev, golden, kind, n, d):
    GG, P = golden("stochastic_grad"), golden("particles")
    key = f"hvp_{kind}_{n}_{d}_"
    energy = make(P, kind, n, d).to(dev)
    plan = _kernel_plan(energy, 1.0)
    x = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
    u = torch.tensor(vectors(GG, n, d), device=dev)
    g, hu = particles.pair_energy_hvp(plan, x, u)
    rows = GG[key + "rows"]
    for name, got in (("g", g), ("hu", hu)):
        ratio, in_err = within(got.cpu().numpy()[rows], GG[key + name + "64"], float(GG[key + f"err_{name}32"]))
        print(f"{key}{name}: {ratio:.3f} of the bound, {in_err:.2f} err32")
        assert ratio <= 1.0, (key, name, ratio)
    # g has the bits of the energy kernel's backward; H is linear in u and H 0 = 0
    xg = x.clone().requires_grad_(True)
    (g_bwd,) = torch.autograd.grad(energy.energy(xg).sum(), xg)
    assert torch.equal(g, g_bwd)
    assert not bool(particles.pair_energy_hvp(plan, x, torch.zeros_like(u))[1].any())
    # at temperature 2: both halved, exactly
    g2, hu2 = particles.pair_energy_hvp(_kernel_plan(energy, 2.0), x, u)
    assert torch.equal(g2, 0.5 * g) and torch.equal(hu2, 0.5 * hu)


@pytest.mark.parametrize("source", ["fed", "philox"])
@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_the_recording_forward_has_the_forwards_bits(hip_lib, dev, golden, layer, source):
    """(13, 3) Lennard-Jones and (64, 3) multi-double-well, 7 steps: q, v, dW bitwise those of pair_langevin, the last frame bitwise the
    final state, frame 3 the state of a run of 4 steps"""
    G, P = golden("stochastic"), golden("particles")
    for kind, n, d in (("lj", 13, 3), ("mdw", 64, 3)):
        nd, steps = n * d, 7
        plan = _kernel_plan(make(P, kind, n, d).to(dev), 1.0)
        h = float(G[case_key(layer, kind, n, d, 12) + "stepsize"])
        x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
        v0 = torch.tensor(start_velocities(G, n, d), device=dev) if layer == "langevin" else None
        w1, w2 = (torch.tensor(normals(G, f, n, d, steps), device=dev) for f in (0, 1))
        noise = dict(seed=77, offset=3) if source == "philox" else (dict(w1=w1, w2=w2) if layer == "langevin" else dict(w1=w1))
        settings = (h, 1.3, 0.7, 1.2) if layer == "langevin" else (h, 1.0, 0.0, 1.0)

        def run(k, record):
            q, v, dW = x0.clone(), None if v0 is None else v0.clone(), torch.empty(B, device=dev)
            cut = {key: (val[:k] if torch.is_tensor(val) else val) for key, val in noise.items()}
            if not record:
                stochastic.pair_langevin(plan, q, v, *settings, k, dW, **cut)
                return [q, dW] + ([] if v is None else [v]), None
            tq = torch.full((k, B, nd), float("nan"), device=dev)
            tv = None if v is None else torch.full((k, B, nd), float("nan"), device=dev)
            stochastic.pair_langevin_record(plan, q, v, *settings, k, dW, tq, tv, **cut)
            return [q, dW] + ([] if v is None else [v]), [tq] + ([] if tv is None else [tv])

        plain, _ = run(steps, False)
        rec, traj = run(steps, True)
        assert same_bits(plain, rec)
        short, _ = run(4, False)
        assert torch.equal(traj[0][-1], rec[0]) and torch.equal(traj[0][3], short[0])
        if layer == "langevin":
            assert torch.equal(traj[1][-1], rec[2]) and torch.equal(traj[1][3], short[2])
        assert float((rec[0] - x0).abs().max()) > 1e-4 and all(bool(torch.isfinite(t).all()) for t in traj)


@pytest.mark.parametrize("layer,kind,n,d,nsteps,tag", LAYER_CASES)
def test_layer_gradients_on_recorded_numbers(hip_lib, dev, golden, monkeypatch, layer, kind, n, d, nsteps, tag):
    GG, G, P = golden("stochastic_grad"), golden("stochastic"), golden("particles")
    key = grad_key(layer, kind, n, d, nsteps, tag)
    flow, xs = build_grad(GG, G, P, layer, kind, n, d, nsteps, tag, device=dev)
    assert flow._fused_setup(*xs) is None and flow._fused_train_setup(*xs) is not None
    forbid_the_torch_formulas(monkeypatch)
    before = [x.detach().clone() for x in xs]
    name, grads = loss_grads(flow, xs)
    assert name == FN[layer], "the output comes from the fused Function"
    assert all(torch.equal(a.detach(), b) for a, b in zip(xs, before)) and flow._fed[1] == nsteps
    rows = GG[key + "rows"]
    for g, gname in zip(grads, ("g", "gv")):
        ratio, in_err = within(g.cpu().numpy()[rows], GG[key + gname + "64"], float(GG[key + f"err_{gname}32"]))
        print(f"{key}{gname}: {ratio:.3f} of the bound, {in_err:.2f} err32")
        assert ratio <= 1.0, (key, gname, ratio)


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_the_gradients_do_not_depend_on_the_split_into_launches(hip_lib, dev, golden, monkeypatch, layer):
    """(13, 3), 12 steps: backward launches of at most 2 and of at most 5 steps (and forward launches of 5) give the bits of the sweep in
    one launch; the forward outputs too"""
    GG, G, P = golden("stochastic_grad"), golden("stochastic"), golden("particles")
    assert stochastic.LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH >= 1
    monkeypatch.setattr(stochastic, "LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH", 12)
    flow, xs = build_grad(GG, G, P, layer, "lj", 13, 3, 12, device=dev)
    fed = flow._fed[0]
    _, whole = loss_grads(flow, xs)
    for cap, fwd_cap in ((2, 64), (5, 64), (5, 5)):
        monkeypatch.setattr(stochastic, "LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH", cap)
        monkeypatch.setattr(stochastic, "LANGEVIN_MAX_STEPS_PER_LAUNCH", fwd_cap)
        name, split = loss_grads(flow.feed_noise(*fed), xs)
        assert name == FN[layer] and same_bits(whole, split), (cap, fwd_cap)


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
@pytest.mark.parametrize("kind,n,d", [("mdw", 4, 2), ("lj", 13, 3)])
def test_in_kernel_philox_gradients_equal_those_of_the_same_numbers_handed_in(hip_lib, dev, golden, monkeypatch, layer, kind, n, d):
    GG, G, P = golden("stochastic_grad"), golden("stochastic"), golden("particles")
    torch.manual_seed(1234)
    monkeypatch.setattr(stochastic, "LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH", 2)          # the offsets of the segments too
    drawn, xs = build_grad(GG, G, P, layer, kind, n, d, 3, device=dev, feed=False)
    drawn.nsteps = 5
    drawn.set_philox_stream(41, calls=7)                                                  # continue the stream at step 7
    seed, offset = flow_seed(drawn)
    *ya, dWa = drawn(*xs)
    assert drawn._philox_ids()[1] == 12 and type(dWa.grad_fn).__name__ == FN[layer]
    ga = torch.autograd.grad(dWa.sum() + sum(y.sum() for y in ya), xs)
    w1, w2 = philox_normals(seed, offset, 5, B, n * d, dev)
    fed, _ = build_grad(GG, G, P, layer, kind, n, d, 3, device=dev, feed=False)
    fed.nsteps = 5
    fed.feed_noise(*((w1,) if layer == "brownian" else (w1, w2)))
    *yb, dWb = fed(*xs)
    gb = torch.autograd.grad(dWb.sum() + sum(y.sum() for y in yb), xs)
    assert same_bits(ya + [dWa], yb + [dWb]) and same_bits(ga, gb)
    # ... and the forward is the non-recording one's
    with torch.no_grad():
        plain = fed.feed_noise(*((w1,) if layer == "brownian" else (w1, w2)))(*xs)
    assert same_bits(plain, yb + [dWb])
    assert float(ga[0].abs().max()) > 0


@pytest.mark.parametrize("kind,n,d", [("mdw", 4, 2), ("lj", 13, 3), ("mfn", 64, 3)])
def test_metropolis_gradient(hip_lib, dev, golden, monkeypatch, kind, n, d):
    """g_x = g_y + g_dW (dE/dx(y) - dE/dx(x)) against autograd through the general path in f64 on the same numbers, on the chains the
    fixture keeps; err_32: the general path's own f32 run (torch formulas, no device) against its f64 run"""
    G, P = golden("stochastic"), golden("particles")
    keep = G[case_key("metropolis", kind, n, d, MC_STEPS) + "keep"]

    def general(dtype):
        flow, (x0,) = build(G, P, "metropolis", kind, n, d, MC_STEPS)
        x = x0.to(dtype).requires_grad_(True)
        y, dW = flow(x)
        return torch.autograd.grad(dW.sum() + y.sum(), x)[0].numpy()[keep]

    g64, g32 = general(torch.float64), general(torch.float32)
    err32 = float(np.abs(g32 - g64).max())
    flow, (x0,) = build(G, P, "metropolis", kind, n, d, MC_STEPS, device=dev)
    flow.fused_backward = True
    x = x0.clone().requires_grad_(True)
    forbid_the_torch_formulas(monkeypatch)
    y, dW = flow(x)
    assert type(y.grad_fn).__name__ == "_MetropolisFnBackward"
    (g,) = torch.autograd.grad(dW.sum() + y.sum(), x)
    ratio, in_err = within(g.cpu().numpy()[keep], g64, err32)
    print(f"metropolis_{kind}_{n}_{d}: {ratio:.3f} of the bound, {in_err:.2f} err32 ({err32:.3g}), kept {int(keep.sum())} / {B}")
    assert ratio <= 1.0


def test_kl_step_through_a_coupling_and_a_brownian_layer(hip_lib, dev, golden):
    """SequentialFlow([affine coupling, BrownianFlow]) on the DW4-sized multi-double-well: the parameter gradients of the KL loss with the
    fused backward against the general path (``fused = False``) on the same fed noise; bound, per parameter tensor: 4 x the general path's
    own f32-vs-f64 error on the device + 1e-6 (1 + |g|), around the f64 gradient"""
    torch.manual_seed(21)
    n, d, half, batch, nsteps = 4, 2, 4, B, 5
    target = bg.MultiDoubleWellPotential(n * d, n, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    coupling = [bg.SplitFlow(half),
                bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.ReLU()),
                                                     scale_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.Tanh()))),
                bg.MergeFlow(half)]
    brown = bg.BrownianFlow(target, nsteps=nsteps, stepsize=1e-3)
    flow = bg.SequentialFlow(coupling + [brown]).to(dev)
    z = torch.tensor([2.0, -2.0, 2.0, 2.0, -2.0, 2.0, -2.0, -2.0], device=dev) + 0.3 * torch.randn(batch, n * d, device=dev)
    noise = torch.randn(nsteps, batch, n * d, device=dev)

    def kl_gradients(model, zz, fused_backward, fused=True):
        layer = model._blocks[-1]
        layer.fused, layer.fused_backward = fused, fused_backward
        layer.feed_noise(noise)
        model.zero_grad()
        x, dlogp = model(zz)
        (model._blocks[-1].energy_model.energy(x) - dlogp).mean().backward()
        return type(x.grad_fn).__name__, [p.grad.detach().double().cpu().numpy() for p in model.parameters()]

    def kl_gradients_f64():
        """the general path in f64 on the device; the coupling kernels are f32 only, so the coupling runs as its restatement in torch
        ops (oracle/torch_flow.py), then the layer's general path and the target's torch formulas"""
        from oracle import torch_flow
        model = copy.deepcopy(flow).double()
        layer = model._blocks[-1]
        layer.fused, layer.fused_backward = False, False
        layer.feed_noise(noise)
        (y,), logdet = torch_flow.run_flow(bg.SequentialFlow(list(model._blocks)[:-1]), [z.double()], grad=True)
        x, dW = layer(y)
        assert x.dtype == torch.float64 and x.is_cuda
        (layer.energy_model.energy(x) - (logdet + dW)).mean().backward()
        return [p.grad.detach().cpu().numpy() for p in model.parameters()]

    name, got = kl_gradients(flow, z, True)
    assert name == "_BrownianFnBackward"
    name, general32 = kl_gradients(flow, z, False, fused=False)
    assert name != "_BrownianFnBackward"
    general64 = kl_gradients_f64()
    assert len(got) == len(general64) == 9 and all(np.abs(g).max() > 1e-3 for g in general64)     # 2 x 2 x (weight, bias), log_alpha
    worst = 0.0
    for a, g32, g64 in zip(got, general32, general64):
        err = float(np.abs(g32 - g64).max())
        ratio = float((np.abs(a - g64) / (4 * err + 1e-6 * (1 + np.abs(g64)))).max())
        worst = max(worst, ratio)
        print(f"KL step, parameter {tuple(a.shape)}: {ratio:.3f} of the bound, general path's f32 error {err:.3g}, |g| up to {np.abs(g64).max():.3g}")
        assert ratio <= 1.0, (a.shape, ratio, err)
    print(f"KL step: {worst:.3f} of the bound")


def test_fallbacks(hip_lib, dev, golden, monkeypatch):
    GG, G, P = golden("stochastic_grad"), golden("stochastic"), golden("particles")
    for layer in ("brownian", "langevin"):
        key = grad_key(layer, "lj", 4, 2, 3)
        flow, xs = build_grad(GG, G, P, layer, "lj", 4, 2, 3, device=dev)
        fed = flow._fed[0]

        def check(grads):
            for g, gname in zip(grads, ("g", "gv")):
                ratio, _ = within(g.cpu().numpy()[GG[key + "rows"]], GG[key + gname + "64"], float(GG[key + f"err_{gname}32"]))
                assert ratio <= 1.0, (layer, gname, ratio)

        # the default: today's behaviour, the general path and its twice differentiable backward
        del flow.fused_backward
        assert type(flow).fused_backward is False and flow._fused_setup(*xs) is None
        name, grads = loss_grads(flow, xs)
        assert "Fn" not in name
        check(grads)
        *ys, dW = flow.feed_noise(*fed)(*xs)
        (g1,) = torch.autograd.grad(dW.sum(), xs[0], create_graph=True)
        assert torch.autograd.grad(g1.sum(), xs[0])[0].shape == xs[0].shape
        # opted in, but over the byte budget: the general path and one RuntimeWarning
        flow.fused_backward = True
        monkeypatch.setattr(stochastic, "LANGEVIN_BACKWARD_MAX_BYTES", flow._traj_bytes(B, 8) - 1)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            name, grads = loss_grads(flow.feed_noise(*fed), xs)
        caught = [w for w in caught if issubclass(w.category, RuntimeWarning)]
        assert "Fn" not in name and len(caught) == 1 and "LANGEVIN_BACKWARD_MAX_BYTES" in str(caught[0].message)
        check(grads)
        monkeypatch.setattr(stochastic, "LANGEVIN_BACKWARD_MAX_BYTES", flow._traj_bytes(B, 8))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            name, grads = loss_grads(flow.feed_noise(*fed), xs)
        assert name == FN[layer]
        check(grads)
        # the fused backward is once differentiable
        *ys, dW = flow.feed_noise(*fed)(*xs)
        (g1,) = torch.autograd.grad(dW.sum(), xs[0], create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad(g1.sum(), xs[0])
        # no grad wanted: the plain fused forward; grad disabled: too; f64 on the device: the general path
        with torch.no_grad():
            out = flow.feed_noise(*fed)(*xs)
        assert out[0].grad_fn is None and flow._fed[1] == 3
        out = flow.feed_noise(*fed)(*[x.detach() for x in xs])
        assert out[0].grad_fn is None and not out[-1].requires_grad
        xd = [x.detach().double().requires_grad_(True) for x in xs]
        assert flow._fused_train_setup(*xd) is None
        assert "Fn" not in loss_grads(flow.feed_noise(*fed), xd)[0]
        # fused = False wins over fused_backward
        flow.fused = False
        assert flow._fused_train_setup(*xs) is None and "Fn" not in loss_grads(flow.feed_noise(*fed), xs)[0]
