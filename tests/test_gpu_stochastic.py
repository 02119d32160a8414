"""GPU (-m gpu): the fused stochastic layers -- ``BrownianFlow`` / ``LangevinFlow`` on bgk_pair_langevin (csrc/bgk_langevin.hip) and
``MetropolisMCFlow`` on bgk_pair_energy + bgk_pair_mcmc -- against the reference's recorded f64 runs on fixed random numbers
(tests/golden/stochastic.npz, written by tests/golden/make_stochastic_goldens.py), and bitwise against themselves: in-kernel Philox = the
same numbers handed in, sharded / split runs = the run in one piece, one launch of k steps = k launches of one step.

Bound of the parity tests: |got - f64| <= 4 err_32 + 1e-6 (1 + |f64|), err_32 the error of the reference's own f32 run of the same case --
the rule of the chain kernel's parity test (the kernel's row-sum order and its f64 accumulation differ from the reference's f32 run).
Metropolis: on the chains the fixture keeps (f64 decision margin >= 1e-3 at every step).

B = 150: a partial last tile of every tile height (64 rows; 20 / 16 rows at n d = 192: eight / ten tiles).

dW of a run split into launches is the f32 sum of the launches' dW, so it equals the unsplit run's dW only to rounding: with the dW_k of
the single steps, 2^-22 sum_k |dW_k| bounds every split (each partial sum and each rounding is at most 2^-24 sum_k |dW_k|, fewer than
four of them per launch boundary contribute)."""
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import stochastic
from bgflow_amd.distributions import _kernel_plan, philox_sample

from stochastic_common import (B, GRAD_CASES, GRAD_STEPS, INTEGRATOR_CASES, MC_STEPS, METROPOLIS_CASES, build, case_key, make, normals,
                               start_velocities)

pytestmark = pytest.mark.gpu


def within(got, want, err32):
    """max of |got - want| / (4 err32 + 1e-6 (1 + |want|)), and max |got - want| / err32"""
    diff = np.abs(got.astype(np.float64) - want)
    return float((diff / (4 * err32 + 1e-6 * (1 + np.abs(want)))).max()), float(diff.max() / max(err32, 1e-300))


@pytest.mark.parametrize("layer,kind,n,d,nsteps,tag", INTEGRATOR_CASES)
def test_parity_of_the_integrators_on_recorded_numbers(hip_lib, dev, golden, layer, kind, n, d, nsteps, tag):
    G, P = golden("stochastic"), golden("particles")
    key = case_key(layer, kind, n, d, nsteps, tag)
    flow, xs = build(G, P, layer, kind, n, d, nsteps, tag, device=dev)
    assert flow._fused_setup(*xs) is not None, "the case must take the fused path"
    before = [x.clone() for x in xs]
    *ys, dW = flow(*xs)
    assert all(torch.equal(a, b) for a, b in zip(xs, before)), "the inputs are not modified"
    assert dW.shape == (B, 1) and dW.dtype == torch.float32 and flow._fed[1] == nsteps
    rows = G[key + "rows"]
    report = []
    for y, name in zip(ys + [dW[:, 0]], ("x", "v", "dW") if layer == "langevin" else ("x", "dW")):
        got = y.cpu().numpy()
        want = G[key + name + "64"]
        ratio, in_err = within(got if name == "dW" else got[rows], want, float(G[key + f"err_{name}32"]))
        report.append(f"{name}: {ratio:.3f} of the bound, {in_err:.2f} err_{name}32")
        assert ratio <= 1.0, (key, name, ratio)
    print(f"{key[:-1]}: " + "; ".join(report))


@pytest.mark.parametrize("kind,n,d", METROPOLIS_CASES)
def test_parity_of_metropolis_and_the_energy_kernels_bits(hip_lib, dev, golden, kind, n, d):
    G, P = golden("stochastic"), golden("particles")
    key = case_key("metropolis", kind, n, d, MC_STEPS)
    flow, (x0,) = build(G, P, "metropolis", kind, n, d, MC_STEPS, device=dev)
    assert flow._fused_setup(x0) is not None
    before = x0.clone()
    x, dW = flow(x0)
    assert torch.equal(x0, before) and dW.shape == (B, 1)
    # E0 and the final energies are the energy kernel's bits for the states
    e0, e = flow.energy_model.energy(x0)[:, 0], flow.energy_model.energy(x)[:, 0]
    assert torch.equal(dW[:, 0], e - e0)
    keep, rows = G[key + "keep"], G[key + "rows"]
    report = []
    for name, got, want, err in (("x", x.cpu().numpy()[rows][keep[rows]], G[key + "x64"][keep[rows]], "err_x32"),
                                 ("e", e.cpu().numpy()[keep], G[key + "e64"][keep], "err_e32"),
                                 ("dW", dW[:, 0].cpu().numpy()[keep], G[key + "dW64"][keep], "err_dW32")):
        ratio, in_err = within(got, want, float(G[key + err]))
        report.append(f"{name}: {ratio:.3f} of the bound, {in_err:.2f} {err}")
        assert ratio <= 1.0, (key, name, ratio)
    print(f"{key[:-1]}: kept {int(keep.sum())} / {B}; " + "; ".join(report))
    moved = (x != x0).any(dim=1).cpu().numpy()
    assert np.array_equal(moved[keep], (G[key + "acc"] > 0)[keep])


def philox_normals(seed, offset, n_steps, batch, nd, dev, row0=0):
    """what bgk_philox_fields writes for (seed, offset + s), fields [normal nd, normal nd]"""
    w1, w2 = [], []
    for s in range(n_steps):
        (a, b), _ = philox_sample([(1, nd, None, None, 1.0, 0.0), (1, nd, None, None, 1.0, 0.0)], batch, dev, seed, offset + s, row0=row0)
        w1.append(a)
        w2.append(b)
    return torch.stack(w1), torch.stack(w2)


def flow_seed(flow):
    from bgflow_amd import dp
    st = flow._philox_ids()
    return (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1), st[1]


def integrator(layer, energy, nsteps, h):
    if layer == "brownian":
        return bg.BrownianFlow(energy, nsteps=nsteps, stepsize=h)
    return bg.LangevinFlow(energy, nsteps=nsteps, stepsize=h, mass=1.3, gamma=0.7, kT=1.2)


def inputs(G, P, layer, n, d, dev):
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
    return (x0,) if layer == "brownian" else (x0, torch.tensor(start_velocities(G, n, d), device=dev))


def same_bits(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
@pytest.mark.parametrize("kind,n,d", [("mdw", 4, 2), ("lj", 13, 3)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, layer, kind, n, d):
    G, P = golden("stochastic"), golden("particles")
    torch.manual_seed(1234)
    energy = make(P, kind, n, d).to(dev)
    h = float(G[case_key(layer, kind, n, d, 12) + "stepsize"])
    xs = inputs(G, P, layer, n, d, dev)
    drawn = integrator(layer, energy, 5, h).set_philox_stream(41, calls=7)          # continue the stream at step 7
    seed, offset = flow_seed(drawn)
    assert offset == 7
    a = drawn(*xs)
    assert drawn._philox_ids()[1] == 12                                              # the counter is the index of the next step
    w1, w2 = philox_normals(seed, offset, 5, B, n * d, dev)
    fed = integrator(layer, energy, 5, h)
    fed.feed_noise(*((w1,) if layer == "brownian" else (w1, w2)))
    b = fed(*xs)
    assert same_bits(a, b)
    assert float((a[0] - xs[0]).abs().max()) > 1e-3 and float(a[-1].abs().max()) > 0   # (a run that moves)


def test_philox_layout_at_the_widest_row(hip_lib, dev):
    """n d = 192, from x = 0 (and v = 0) on a mean-free normal, whose force vanishes there: one Brownian step with h = 1/2 leaves
    x = sqrt(2 h) w = w, one Langevin step with h = mass = gamma = kT = 1 leaves q = w1 (vh = 1/2 (2 w1), exact) and, on a target as wide
    as 1e6, v = (w1 + w2) / 1.5 -- against the numpy restatement of the generator (oracle/philox.py) to 4e-6, the project's bound for
    Box-Muller in f32 against f64; w2 = 1.5 v - q carries four more roundings of magnitudes up to |w1| + |w2|: + 2^-22 (|w1| + |w2|)"""
    from oracle import philox
    n, d, rows, row0, offset = 64, 3, 100, 70, 5
    energy = bg.MeanFreeNormalDistribution(n * d, n, std=1e6, two_event_dims=False).to(dev)
    zero = torch.zeros(rows, n * d, device=dev)
    brown = bg.BrownianFlow(energy, nsteps=1, stepsize=0.5).set_philox_stream(3, calls=offset)
    brown.chain_offset = row0
    seed, _ = flow_seed(brown)
    want1 = philox.sample_field(seed, offset, 0, rows, n * d, 1, row0=row0)
    want2 = philox.sample_field(seed, offset, 1, rows, n * d, 1, row0=row0)
    assert brown._fused_setup(zero) is not None
    y, _ = brown(zero)
    np.testing.assert_allclose(y.cpu().numpy(), want1, rtol=0, atol=4e-6)
    lang = bg.LangevinFlow(energy, nsteps=1, stepsize=1.0).set_philox_stream(3, calls=offset)
    lang.chain_offset = row0
    q, v, _ = lang(zero, zero)
    np.testing.assert_allclose(q.cpu().numpy(), want1, rtol=0, atol=4e-6)
    w2 = 1.5 * v.cpu().numpy().astype(np.float64) - q.cpu().numpy()
    assert (np.abs(w2 - want2) <= 4e-6 + 2.0 ** -22 * (np.abs(want1) + np.abs(want2))).all()


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_independence_of_the_split_into_launches_and_of_sharding(hip_lib, dev, golden, monkeypatch, layer):
    """(13, 3), 7 steps on the object's stream: one launch = launches of 4 + 3 and of 3 + 3 + 1 steps = two row halves told where they sit
    = seven calls of one step; states bitwise, dW bitwise where no f32 sum of launches is involved, else to the bound of the docstring"""
    G, P = golden("stochastic"), golden("particles")
    kind, n, d, steps = "lj", 13, 3, 7
    torch.manual_seed(99)
    energy = make(P, kind, n, d).to(dev)
    h = float(G[case_key(layer, kind, n, d, 12) + "stepsize"])
    xs = inputs(G, P, layer, n, d, dev)
    flow = integrator(layer, energy, steps, h)
    assert stochastic.LANGEVIN_MAX_STEPS_PER_LAUNCH >= steps
    *whole, dW = flow.set_philox_stream(51)(*xs)
    # two row halves
    parts = []
    for lo, hi in ((0, 70), (70, B)):
        flow.set_philox_stream(51, calls=0)
        flow.chain_offset = lo
        parts.append(flow(*[x[lo:hi].contiguous() for x in xs]))
    flow.chain_offset = 0
    assert same_bits(whole + [dW], [torch.cat(p) for p in zip(*parts)])
    # one step at a time: the states of the run in one launch (f(y) of a step IS f(x) of the next), and the dW_k of the steps
    flow.set_philox_stream(51, calls=0)
    flow.nsteps = 1
    state, dWk = xs, []
    for _ in range(steps):
        *state, dw = flow(*state)
        dWk.append(dw)
    assert flow._philox_ids()[1] == steps and same_bits(whole, state)
    bound = 2.0 ** -22 * torch.stack(dWk).abs().sum(dim=0)
    assert bool(((torch.stack(dWk).double().sum(dim=0) - dW.double()).abs() <= bound).all())
    # capped launches
    flow.nsteps = steps
    for cap in (4, 3):
        monkeypatch.setattr(stochastic, "LANGEVIN_MAX_STEPS_PER_LAUNCH", cap)
        *split, dWs = flow.set_philox_stream(51, calls=0)(*xs)
        assert same_bits(whole, split)
        assert bool(((dWs.double() - dW.double()).abs() <= bound).all())


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_two_steps_equal_two_calls_of_one_step(hip_lib, dev, golden, layer):
    """reusing f(y) as the next step's f(x) is exact"""
    G, P = golden("stochastic"), golden("particles")
    torch.manual_seed(5)
    energy = make(P, "mdw", 4, 2).to(dev)
    xs = inputs(G, P, layer, 4, 2, dev)
    flow = integrator(layer, energy, 2, 0.01).set_philox_stream(52)
    *two, dW = flow(*xs)
    flow.set_philox_stream(52, calls=0)
    flow.nsteps = 1
    *one, dW1 = flow(*xs)
    *one, dW2 = flow(*one)
    assert same_bits(two, one)
    assert bool(((dW1.double() + dW2.double() - dW.double()).abs() <= 2.0 ** -22 * (dW1.abs() + dW2.abs())).all())


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_more_tiles_than_the_grid(hip_lib, dev, layer):
    """(2, 1), one step, B = 4096 x 64 + 5 rows: the workgroups loop over the tiles; equal to the same rows run in two pieces"""
    torch.manual_seed(8)
    batch = 4096 * 64 + 5
    energy = bg.MultiDoubleWellPotential(2, 2, 0.9, -4.0, 0.1, 4.0, two_event_dims=False).to(dev)
    x = (4.0 + 0.3 * torch.randn(batch, 1, device=dev)) * torch.tensor([[0.5, -0.5]], device=dev)
    xs = (x,) if layer == "brownian" else (x, torch.randn(batch, 2, device=dev))
    flow = integrator(layer, energy, 1, 0.01).set_philox_stream(53)
    assert flow._fused_setup(*xs) is not None
    whole = flow(*xs)
    parts = []
    for lo, hi in ((0, 100001), (100001, batch)):
        flow.set_philox_stream(53, calls=0)
        flow.chain_offset = lo
        parts.append(flow(*[t[lo:hi].contiguous() for t in xs]))
    assert same_bits(whole, [torch.cat(p) for p in zip(*parts)])
    assert all(bool(torch.isfinite(t).all()) for t in whole)


def test_fallbacks_give_the_general_paths_result(hip_lib, dev, golden, monkeypatch):
    G, P = golden("stochastic"), golden("particles")
    n, d, nsteps = 4, 2, 12
    for layer in ("brownian", "langevin"):
        key = case_key(layer, "lj", n, d, nsteps)
        fused, xs = build(G, P, layer, "lj", n, d, nsteps, device=dev)
        fed = fused._fed[0]
        want = fused(*xs)

        def close_to_fused(got):
            for a, b, err in zip(got, want, ("err_x32", "err_dW32") if layer == "brownian" else ("err_x32", "err_v32", "err_dW32")):
                ratio, _ = within(a.reshape(b.shape).cpu().numpy(), b.cpu().numpy().astype(np.float64), 2 * float(G[key + err]))
                assert ratio <= 1.0, (layer, err, ratio)      # two f32 evaluations, each within err of the f64 result

        # fused = False on the instance and on the class: the general path in f32 on the device, with the energy kernels
        plain, _ = build(G, P, layer, "lj", n, d, nsteps, device=dev)
        plain.fused = False
        assert plain._fused_setup(*xs) is None
        close_to_fused(plain(*xs))
        del plain.fused
        assert plain._fused_setup(*xs) is not None
        monkeypatch.setattr(type(plain), "fused", False)
        assert plain._fused_setup(*xs) is None
        general = plain.feed_noise(*fed)(*xs)
        close_to_fused(general)
        monkeypatch.undo()
        # f64 input: the fixture's f64 run to the host test's agreement
        plain.feed_noise(*fed)
        xd = [x.double() for x in xs]
        assert plain._fused_setup(*xd) is None
        *ys, dW = plain(*xd)
        assert dW.dtype == torch.float64 and np.abs(ys[0].cpu().numpy()[G[key + "rows"]] - G[key + "x64"]).max() <= 1e-12
        assert np.max(np.abs(dW[:, 0].cpu().numpy() - G[key + "dW64"]) / (1 + np.abs(G[key + "dW64"]))) <= 1e-12
        # [B, n, d] input of a two_event_dims target
        two = type(plain)(make(P, "lj", n, d, two_event_dims=True).to(dev), nsteps=nsteps, stepsize=plain.stepsize).feed_noise(*fed)
        x3 = [x.reshape(B, n, d) for x in xs]
        assert two._fused_setup(*x3) is None
        got = two(*x3)
        assert got[0].shape == (B, n, d) and got[-1].shape == (B, 1)
        close_to_fused(got)
        # a non-contiguous view
        views = []
        for x in xs:
            wide = torch.zeros(B, 2 * n * d, device=dev)
            wide[:, ::2] = x
            views.append(wide[:, ::2])
        assert not views[0].is_contiguous() and plain._fused_setup(*views) is None
        close_to_fused(plain.feed_noise(*fed)(*views))
    # Metropolis: fused = False takes the fused path's decisions on the kept chains
    key = case_key("metropolis", "mdw", n, d, MC_STEPS)
    fused, (x0,) = build(G, P, "metropolis", "mdw", n, d, MC_STEPS, device=dev)
    plain, _ = build(G, P, "metropolis", "mdw", n, d, MC_STEPS, device=dev)
    plain.fused = False
    (xa, dWa), (xb, dWb) = fused(x0), plain(x0)
    keep = torch.tensor(G[key + "keep"], device=dev)
    assert torch.equal(xa[keep], xb[keep]) and torch.allclose(dWa[keep], dWb[keep], rtol=1e-5, atol=1e-5)
    # 65 particles: outside the kernels' envelope
    big = bg.LennardJonesPotential(65 * 3, 65, two_event_dims=False).to(dev)
    xb = 1.2 * torch.stack(torch.meshgrid(*[torch.arange(5.0, device=dev)] * 3, indexing="ij"), -1).reshape(-1, 3)[:65].reshape(1, -1).repeat(6, 1)
    for flow, xs in ((bg.BrownianFlow(big, nsteps=2, stepsize=1e-5), (xb,)), (bg.LangevinFlow(big, nsteps=2, stepsize=1e-3), (xb, torch.zeros_like(xb))),
                     (bg.MetropolisMCFlow(big, nsteps=2, stepsize=0.01), (xb,))):
        assert _kernel_plan(big, 1.0) is None and flow._fused_setup(*xs) is None
        *ys, dW = flow(*xs)
        assert ys[0].shape == (6, 195) and dW.shape == (6, 1) and bool(torch.isfinite(dW).all()) and not xb.requires_grad


@pytest.mark.parametrize("layer,kind", GRAD_CASES)
def test_an_input_that_requires_grad_takes_the_general_path_and_its_backward(hip_lib, dev, golden, layer, kind):
    """(4, 2), 3 steps, f32 on the device over the torch formulas: the gradient of dW.sum() + outputs.sum() against the reference's f64
    one within 4 err_g32 + 1e-6 (1 + |g|)"""
    G, P = golden("stochastic"), golden("particles")
    flow, xs = build(G, P, layer, kind, 4, 2, 1, device=dev)
    flow.nsteps = GRAD_STEPS
    flow.feed_noise(*[torch.tensor(normals(G, f, 4, 2, GRAD_STEPS), device=dev) for f in range(len(xs))])
    assert flow._fused_setup(*xs) is not None
    xs = [x.clone().requires_grad_(True) for x in xs]
    assert flow._fused_setup(*xs) is None
    with torch.no_grad():
        assert flow._fused_setup(*xs) is not None            # ... unless grad is disabled
    *ys, dW = flow(*xs)
    grads = torch.autograd.grad(dW.sum() + sum(y.sum() for y in ys), xs)
    for g, name in zip(grads, ("g", "gv")):
        ratio, in_err = within(g.cpu().numpy(), G[f"grad_{layer}_{kind}_{name}64"], float(G[f"grad_{layer}_{kind}_err_{name}32"]))
        print(f"grad_{layer}_{kind}_{name}: {ratio:.3f} of the bound, {in_err:.2f} err32")
        assert ratio <= 1.0, (layer, kind, name, ratio)


def test_composition_in_a_boltzmann_generator(hip_lib, dev):
    """SequentialFlow([coupling ..., BrownianFlow]) under BoltzmannGenerator.sample: dlogp = the coupling's log-det + the layer's dW"""
    torch.manual_seed(21)
    n, d, half, batch = 4, 2, 4, 96
    prior = bg.MeanFreeNormalDistribution(n * d, n, std=2.0, two_event_dims=False)
    target = bg.MultiDoubleWellPotential(n * d, n, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    coupling = [bg.SplitFlow(half),
                bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.ReLU()),
                                                     scale_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.Tanh()))),
                bg.SwapFlow(),
                bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.ReLU()),
                                                     scale_transformation=bg.DenseNet([half, 16, half], activation=torch.nn.Tanh()))),
                bg.MergeFlow(half)]
    brown = bg.BrownianFlow(target, nsteps=3, stepsize=1e-3).set_philox_stream(61)
    gen = bg.BoltzmannGenerator(prior, bg.SequentialFlow(coupling + [brown]), target).to(dev)
    with torch.no_grad():
        torch.manual_seed(4)
        x, dlogp = gen.sample(batch, with_dlogp=True)
        assert brown._philox_ids()[1] == 3, "the layer ran fused, on its stream"
        torch.manual_seed(4)
        z = prior.sample(batch)
        y, logdet = bg.SequentialFlow(coupling)(z)
        x2, dW = brown.set_philox_stream(61, calls=0)(y)
    assert x.shape == (batch, n * d) and dlogp.shape == (batch, 1)
    assert torch.equal(x, x2) and torch.allclose(dlogp, logdet + dW, rtol=1e-6, atol=1e-6)
    assert float(dW.abs().max()) > 0


def test_a_resumed_object_continues_the_stream(hip_lib, dev, golden):
    G, P = golden("stochastic"), golden("particles")
    torch.manual_seed(17)
    energy = make(P, "mdw", 4, 2).to(dev)
    for layer in ("brownian", "langevin", "metropolis"):
        xs = inputs(G, P, "langevin" if layer == "langevin" else "brownian", 4, 2, dev)

        def new():
            return bg.MetropolisMCFlow(energy, nsteps=3, stepsize=0.3) if layer == "metropolis" else integrator(layer, energy, 3, 0.01)

        first = new().set_philox_stream(71)
        a = first(*xs)
        sd = first.state_dict()
        assert sd["_philox_state"].tolist() == [71, 3]
        b = first(*xs)
        assert not torch.equal(a[0], b[0])
        resumed = new()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # stream 71 is still held by ``first``
            resumed.load_state_dict(sd)
        assert same_bits(b, resumed(*xs)) and resumed._philox_ids() == [71, 6]
