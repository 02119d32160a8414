"""GPU (-m gpu): ``KernelDynamics`` on bgk_kdyn_eval / bgk_kdyn_eval_backward and ``DiffEqFlow`` on bgk_kdyn_integrate (csrc/bgk_kdyn.hip) through
the public classes, against the reference's recorded f64 results (tests/golden/kernel_dynamics.npz, written by
tests/golden/make_kernel_dynamics_goldens.py).

Bound, as for the particle energies (test_gpu_particles.py): err <= 4 err(reference f32) + 1e-6, with err = max_b |v - v64| / (1 + |v64|) for
per-sample scalars (divergence, dlogp) and max |v - v64| / (1 + max |v64|) for arrays (forces, gradients, positions); the reference's f32
error of an integration is that of the fixture script's own f32 integration.  Per-coordinate arrays are recorded for 40 of the 150 rows
(the first 8 and 118..149: the partial last tile of every tile height is whole); divergence and dlogp are compared on every row.

Shapes are the fixture's: B = 150, n d from 2 to 192 (64, 41/22/20 rows per tile), K = 10 / O = 5 and the envelope's K = 64 / O = 16."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from kdyn_common import CONFIGS, PARAMS, SETS, SHAPES, bound, err_a, err_s, evaluate, flow_of, kernel_set, make_dynamics, scalars

pytestmark = pytest.mark.gpu


def positions(golden, dev, n, d):
    return torch.tensor(golden("particles")[f"x_{n}_{d}"], device=dev).reshape(150, n * d)


@pytest.fixture(scope="module")
def evaluated(hip_lib, dev, golden):
    """forces, divergence and gradients of a golden case at one of its times through the public class, computed once"""
    G = golden("kernel_dynamics")

    @functools.lru_cache(maxsize=None)
    def run(name, n, d, i):
        dyn = make_dynamics(G, name, n, d).to(dev)
        x = positions(golden, dev, n, d)
        assert dyn._kernel_rows(x) is not None, "a golden case must be inside the kernel's envelope"
        return evaluate(dyn, x, float(G["times"][i]))

    return run


@pytest.fixture(scope="module")
def integrated(hip_lib, dev, golden):
    """(y, dlogp) of a golden case and configuration: the fused launch (no grad) or the composition of evaluations (under grad)"""
    G = golden("kernel_dynamics")

    @functools.lru_cache(maxsize=None)
    def run(name, n, d, m, nt, dr, fused):
        dyn = make_dynamics(G, name, n, d).to(dev)
        flow = flow_of(dyn, m, nt)
        x = positions(golden, dev, n, d)
        if fused:
            with torch.no_grad():
                y, dlogp = flow(x, inverse=dr == "i")
        else:
            y, dlogp = flow(x.clone().requires_grad_(True), inverse=dr == "i")
            assert y.requires_grad and dlogp.requires_grad
        assert y.shape == x.shape and dlogp.shape == (150, 1)
        return y.detach().cpu().numpy(), dlogp.detach().cpu().numpy().reshape(-1)

    return run


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_parity(evaluated, golden, name, n, d, i):
    G = golden("kernel_dynamics")
    key = f"{name}_{n}_{d}_"
    rows = G[key + "rows"]
    r = evaluated(name, n, d, i)
    assert all(np.isfinite(v).all() for v in r.values())
    checks = [("div", err_s(r["div"], G[key + "div64"][i]), bound(G, f"{key}err_div32_t{i}"))]
    if f"{key}f64_t{i}" in G.files:
        checks.append(("forces", err_a(r["f"][rows], G[f"{key}f64_t{i}"]), bound(G, f"{key}err_f32_t{i}")))
    if i == 1:
        checks.append(("g_x", err_a(r["gx"][rows], G[key + "gx64"]), bound(G, f"{key}err_gx32_t{i}")))
    for p in PARAMS:
        checks.append(("g" + p, err_a(r["g" + p], G[f"{key}g64{p}"][i]), bound(G, f"{key}err_g32_t{i}{p}")))
    for what, e, b in checks:
        print(f"{key}t{i} {what}: error {e:.3g} (bound {b:.3g})")
    bad = [(what, e, b) for what, e, b in checks if not e <= b]
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_integration(integrated, golden, name, n, d, fused):
    """both methods, both directions, Nt in {1, 4}: the one-launch integration and the composition that trains"""
    G = golden("kernel_dynamics")
    key = f"{name}_{n}_{d}_"
    rows = G[key + "rows"]
    checks = []
    for ci, (m, nt, dr) in enumerate(CONFIGS):
        tag = f"{m}{nt}{dr}"
        y, dlogp = integrated(name, n, d, m, nt, dr, fused)
        assert np.isfinite(y).all() and np.isfinite(dlogp).all()
        checks.append((tag + " dlogp", err_s(dlogp, G[key + "dlogp64"][ci]), bound(G, f"{key}err_dlogp32_{tag}")))
        if f"{key}y64_{tag}" in G.files:
            checks.append((tag + " y", err_a(y[rows], G[f"{key}y64_{tag}"]), bound(G, f"{key}err_y32_{tag}")))
    for what, e, b in checks:
        print(f"{key}{what}: error {e:.3g} (bound {b:.3g})")
    bad = [(what, e, b) for what, e, b in checks if not e <= b]
    assert not bad, bad


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_round_trip(hip_lib, dev, golden, name, n, d):
    """forward then inverse.  The discretisation makes the round trip inexact: the f64 restatement's own round-trip error rt64 is recorded;
    the kernel's may be four times that plus the f32 floor -- the parity bounds of the two integrations it consists of, in units of the
    positions (1 + max |x|)"""
    G = golden("kernel_dynamics")
    key = f"{name}_{n}_{d}_"
    dyn = make_dynamics(G, name, n, d).to(dev)
    x = positions(golden, dev, n, d)
    scale = 1.0 + float(x.abs().max())
    bad = []
    with torch.no_grad():
        for m in ("rk4", "euler"):
            for nt in (1, 4):
                flow = flow_of(dyn, m, nt)
                y, dl = flow(x)
                back, dl_back = flow(y, inverse=True)
                e = float((back - x).abs().max())
                rt64 = scalars(G)[f"{key}rt64_{m}{nt}"]
                b = 4 * rt64 + scale * (bound(G, f"{key}err_y32_{m}{nt}f") + bound(G, f"{key}err_y32_{m}{nt}i"))
                print(f"{key}{m}{nt}: round trip {e:.3g} (f64 restatement {rt64:.3g}, bound {b:.3g})")
                if not e <= b:
                    bad.append((m, nt, e, b))
    assert not bad, bad


@pytest.mark.parametrize("n,d", [(4, 2), (13, 3), (64, 3)])
def test_symmetries(hip_lib, dev, golden, n, d):
    """forces sum to zero over the particles; a mean-free input stays mean-free through the flow; permuting the particles permutes the
    outputs and leaves dlogp"""
    G = golden("kernel_dynamics")
    key = f"ref_{n}_{d}_"
    dyn = make_dynamics(G, "ref", n, d).to(dev)
    x = positions(golden, dev, n, d)
    with torch.no_grad():
        forces, _ = dyn(0.37, x)
        total = forces.view(150, n, d).sum(dim=1)
        b = bound(G, key + "err_f32_t1") * (1.0 + float(forces.abs().max()))
        print(f"{key}: |sum_i force_i| <= {float(total.abs().max()):.3g} (bound {b:.3g})")
        assert float(total.abs().max()) <= b
        flow = flow_of(dyn, "rk4", 4)
        x0 = (x.view(150, n, d) - x.view(150, n, d).mean(dim=1, keepdim=True)).reshape(150, n * d).contiguous()
        y, dlogp = flow(x0)
        by = bound(G, key + "err_y32_rk44f") * (1.0 + float(y.abs().max()))
        centroid = float(y.view(150, n, d).mean(dim=1).abs().max())
        print(f"{key}: centroid after the flow {centroid:.3g} (bound {by:.3g})")
        assert centroid <= by
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).to(dev)
        yp, dlogp_p = flow(x0.view(150, n, d)[:, perm].reshape(150, n * d).contiguous())
        e_y = float((yp.view(150, n, d) - y.view(150, n, d)[:, perm]).abs().max())
        e_l = float(((dlogp_p - dlogp).abs() / (1.0 + dlogp.abs())).max())
        print(f"{key}: permuted outputs differ by {e_y:.3g} (bound {by:.3g}), dlogp by {e_l:.3g} (bound {bound(G, key + 'err_dlogp32_rk44f'):.3g})")
        assert e_y <= by and e_l <= bound(G, key + "err_dlogp32_rk44f")


def test_edge_rows(hip_lib, dev, golden):
    """two coincident particles (rows 0, 1); one particle 100 away, every radial basis function of its pairs underflows (rows 2, 3)"""
    G = golden("kernel_dynamics")
    dyn = make_dynamics(G, "ref", 4, 3, prefix="edge_").to(dev)
    x = torch.tensor(G["edge_x"], device=dev).reshape(8, 12)
    r = evaluate(dyn, x, float(G["times"][1]))
    assert all(np.isfinite(v).all() for v in r.values())
    checks = [("forces", err_a(r["f"], G["edge_f64"]), bound(G, "edge_err_f32")), ("div", err_s(r["div"], G["edge_div64"]), bound(G, "edge_err_div32")),
              ("g_x", err_a(r["gx"], G["edge_gx64"]), bound(G, "edge_err_gx32"))]
    checks += [("g" + p, err_a(r["g" + p], G[f"edge_g64{p}"]), bound(G, f"edge_err_g32{p}")) for p in PARAMS]
    for what, e, b in checks:
        print(f"edge rows {what}: error {e:.3g} (bound {b:.3g})")
    assert not [(what, e, b) for what, e, b in checks if not e <= b]
    with torch.no_grad():
        y, dlogp = flow_of(dyn, "rk4", 4)(x)
    assert torch.isfinite(y).all() and torch.isfinite(dlogp).all()


def test_fallbacks(hip_lib, dev, golden):
    """inputs outside the kernel's envelope are evaluated by the torch formulas and raise nothing"""
    G = golden("kernel_dynamics")
    n, d = 13, 3
    dyn = make_dynamics(G, "ref", n, d).to(dev)
    x = positions(golden, dev, n, d)
    f, nd = dyn(0.37, x)
    ft, ndt = dyn._forward_torch(0.37, x)
    torch.testing.assert_close(f, ft, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(nd, ndt, rtol=1e-4, atol=1e-4)
    assert torch.equal(dyn(0.37, x, compute_divergence=False), f)
    assert torch.equal(dyn(torch.tensor(0.37, device=dev), x.view(150, n, d))[0], f)
    # f64
    dyn64 = make_dynamics(G, "ref", n, d, torch.float64).to(dev)
    f64, nd64 = dyn64(0.37, x.double())
    assert f64.dtype == torch.float64 and torch.equal(f64, dyn64._forward_torch(0.37, x.double())[0])
    torch.testing.assert_close(f.double(), f64, rtol=1e-4, atol=1e-5)
    # a strided view
    wide = torch.cat([x, x], dim=1)[:, :n * d]
    assert not wide.is_contiguous() and dyn._kernel_rows(wide) is None
    torch.testing.assert_close(dyn(0.37, wide)[0], f, rtol=1e-4, atol=1e-5)
    # 65 particles; 65 distance kernels
    gen = torch.Generator().manual_seed(6)
    big = bg.KernelDynamics(65, 3, **kernel_set("ref")).to(dev)
    xb = (torch.randn(4, 65 * 3, generator=gen) * 2).to(dev)
    assert big._kernel_rows(xb) is None
    fb, ndb = big(0.2, xb)
    assert torch.equal(fb, big._forward_torch(0.2, xb)[0]) and torch.isfinite(ndb).all()
    ks = kernel_set("ref")
    ks.update(mus=torch.linspace(0, 8, 65), gammas=torch.full((65,), 0.3))
    many = bg.KernelDynamics(n, d, **ks).to(dev)
    assert many._kernel_rows(x) is None
    fm, _ = many(0.2, x)
    assert torch.equal(fm, many._forward_torch(0.2, x)[0])
    with torch.no_grad():
        y, dlogp = flow_of(many, "rk4", 2)(x)
    assert torch.isfinite(y).all() and dlogp.shape == (150, 1)
    # training the distance bandwidths has no kernel-side gradient: the torch formulas under grad, the kernel without
    ks = kernel_set("ref")
    trained = bg.KernelDynamics(n, d, optimize_d_gammas=True, **ks).to(dev)
    assert trained._kernel_rows(x) is None
    with torch.no_grad():
        assert trained._kernel_rows(x) is not None
    (trained(0.2, x)[0] ** 2).sum().backward()
    assert trained._neg_log_gammas.grad is not None and torch.isfinite(trained._neg_log_gammas.grad).all()
    # no time kernels: the kernel path with tau = 1
    ks = {k: v for k, v in kernel_set("ref").items() if k in ("mus", "gammas")}
    plain = bg.KernelDynamics(n, d, **ks).to(dev)
    with torch.no_grad():
        plain._bias.fill_(0.05)
        plain._importance.fill_(0.3)
    assert plain._kernel_rows(x) is not None
    fp, ndp = plain(0.7, x)
    fpt, ndpt = plain._forward_torch(0.7, x)
    torch.testing.assert_close(fp, fpt, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ndp, ndpt, rtol=1e-4, atol=1e-4)


def test_blocks_that_walk_several_tiles(hip_lib, dev, golden):
    """(4, 2) at B = 4096 x 64 + 5, Nt = 1: the 64-row tiles outnumber the 4096 workgroups of bgk_kdyn_integrate, so the first block takes a
    second, partial tile; its rows and the end of the first pass get the bits the same rows get in a batch of their own"""
    G = golden("kernel_dynamics")
    n, d = 4, 2
    B = 4096 * 64 + 5
    dyn = make_dynamics(G, "ref", n, d).to(dev)
    flow = flow_of(dyn, "rk4", 1)
    x150 = positions(golden, dev, n, d)
    x = x150[torch.arange(B, device=dev) % 150].contiguous()
    tail = slice(4096 * 64 - 3, B)
    with torch.no_grad():
        y, dlogp = flow(x)
        yt, dlogp_t = flow(x[tail].contiguous())
        yh, dlogp_h = flow(x[:64].contiguous())
    assert torch.isfinite(y).all() and torch.isfinite(dlogp).all()
    assert torch.equal(y[tail], yt) and torch.equal(dlogp[tail], dlogp_t)
    assert torch.equal(y[:64], yh) and torch.equal(dlogp[:64], dlogp_h)


def test_kl_training_on_dw4(hip_lib, dev, golden):
    """an equivariant flow (RK4, Nt = 4, K = 10, O = 5) between the mean-free normal prior and the DW4 target: 20 KLTrainer steps at batch 512
    keep the loss finite and lower it from the first to the last five-step mean; the forward and backward kernels run"""
    from bgflow_amd.training import FlatAdam, KLTrainer
    from test_gpu_round6 import _device_kernel_names
    P = golden("particles")
    torch.manual_seed(3)
    n, d = 4, 2
    dyn = bg.KernelDynamics(n, d, **kernel_set("ref"))
    flow = bg.DiffEqFlow(dyn, use_checkpoints=True, Nt=4, method="RK4")
    prior = bg.MeanFreeNormalDistribution(n * d, n, std=2.0, two_event_dims=False)
    a, b, c, off = (float(v) for v in P["mdw_params"])
    target = bg.MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)
    gen = bg.BoltzmannGenerator(prior, flow, target).to(dev)
    opt = FlatAdam([p for p in gen.parameters() if p.requires_grad], lr=5e-3)
    trainer = KLTrainer(gen, optim=opt, train_likelihood=False, train_energy=True)
    trainer.train(20, batchsize=512)
    _, _, ys = trainer.losses()
    kll = np.asarray(ys[0]).reshape(-1)
    print("KL loss:", kll)
    assert len(kll) == 20 and np.isfinite(kll).all(), kll
    assert kll[-5:].mean() < kll[:5].mean(), f"KL loss {kll[:5].mean():.3f} -> {kll[-5:].mean():.3f}"

    def step():
        opt.zero_grad()
        gen.kldiv(512).mean().backward()
    names = _device_kernel_names(step)
    print(sorted(set(k.split("(")[0][-60:] for k in names)))
    assert any("kdyn_eval_kernel" in k for k in names) and any("kdyn_eval_bwd_kernel" in k for k in names)
    with torch.no_grad():
        samples = gen.sample(64)
    assert samples.shape == (64, n * d) and torch.isfinite(samples).all()
    assert float(samples.view(64, n, d).mean(dim=1).abs().max()) < 1e-4
