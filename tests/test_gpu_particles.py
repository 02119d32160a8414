"""GPU (-m gpu): the particle-system energies -- LennardJonesPotential, MultiDoubleWellPotential, MeanFreeNormalDistribution on
bgk_pair_energy / _backward / _kl_sums (csrc/bgk_pair.hip) -- through the public classes, against the reference's recorded f64 results
(tests/golden/particles.npz, written by tests/golden/make_particle_goldens.py).

Bounds: err(v) = max_b |v_b - u64_b| / (1 + |u64_b|) <= 4 err(reference f32) + 1e-6 (the factor: another summation order over up to 2016
pairs; the floor: cases where the reference's f32 happens to be exact); gradients likewise, per case, relative to 1 + max |g64|, against
four times the error of the reference's own f32 autograd.  g64 of the two widest shapes is recorded for 40 of the 150 rows (the first 8
and 118..149: the partial last tile of either tile height is whole); the energies are compared on every row.

Shapes are the fixture's: B = 150 (a partial last tile), n d from 2 to 192 (both tile heights of the backward kernel)."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd.distributions import kl_loss_sums

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (13, 3), (55, 3), (64, 3)]
KINDS = ["lj", "ljn", "mdw", "mfn"]


def make(G, kind, n, d, two_event_dims=True):
    if kind in ("lj", "ljn"):
        eps, rm, osc = (float(v) for v in G["lj_params"])
        return bg.LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=kind == "lj", oscillator_scale=osc, two_event_dims=two_event_dims)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in G["mdw_params"])
        return bg.MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=two_event_dims)
    return bg.MeanFreeNormalDistribution(n * d, n, std=float(G["mfn_std"]), two_event_dims=two_event_dims)


def energy_and_grad(energy, x):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x)
    assert u.shape == (x.shape[0], 1)
    u.sum().backward()
    return u.detach().cpu().numpy().reshape(-1), x.grad.cpu().numpy().reshape(x.shape[0], -1)


def err_u(v, u64):
    return float(np.max(np.abs(v.astype(np.float64) - u64) / (1.0 + np.abs(u64))))


def err_g(v, g64):
    return float(np.max(np.abs(v.astype(np.float64) - g64)) / (1.0 + np.max(np.abs(g64))))


@pytest.fixture(scope="module")
def results(hip_lib, dev, golden):
    """energies and gradients of a golden case through the public class, computed once per case"""
    G = golden("particles")

    @functools.lru_cache(maxsize=None)
    def run(kind, n, d):
        x = torch.tensor(G[f"x_{n}_{d}"], device=dev)
        return energy_and_grad(make(G, kind, n, d).to(dev), x)

    return run


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_energy_parity(results, golden, kind, n, d):
    G = golden("particles")
    key = f"{kind}_{n}_{d}"
    u, _ = results(kind, n, d)
    e, ref = err_u(u, G[key + "_u64"]), float(G[key + "_err_u32"])
    print(f"{key}: energy error {e:.3g} (the reference's f32: {ref:.3g})")
    assert e <= 4 * ref + 1e-6


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_parity(results, golden, kind, n, d):
    G = golden("particles")
    key = f"{kind}_{n}_{d}"
    _, g = results(kind, n, d)
    assert np.isfinite(g).all()
    e, ref = err_g(g[G[key + "_g_rows"]], G[key + "_g64"]), float(G[key + "_err_g32"])
    print(f"{key}: gradient error {e:.3g} (the reference's f32 autograd: {ref:.3g})")
    assert e <= 4 * ref + 1e-6


@pytest.mark.parametrize("kind", ["lj", "mdw"])
def test_coincident_particles(hip_lib, dev, golden, kind):
    """samples 0 and 1 hold two particles at one position"""
    G = golden("particles")
    key = f"edge_{kind}"
    u, g = energy_and_grad(make(G, kind, 4, 3).to(dev), torch.tensor(G[key + "_x"], device=dev))
    if kind == "mdw":
        assert np.isfinite(u).all() and np.isfinite(g).all()
        assert np.isfinite(G[key + "_g32"]).all()           # the reference: cdist's backward gives the coincident pair the gradient 0
        rows = slice(0, 8)                                   # ... so the whole batch is compared
    else:
        assert (np.isfinite(u) == np.isfinite(G[key + "_u32"])).all()
        rows = slice(2, 8)
    assert err_u(u[rows], G[key + "_u64"][rows]) <= 4 * float(G[key + "_err_u32"]) + 1e-6
    assert err_g(g[rows], G[key + "_g64"][rows]) <= 4 * float(G[key + "_err_g32"]) + 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_layouts_and_fallbacks(hip_lib, dev, golden, kind):
    G = golden("particles")
    n, d = 13, 3
    x = torch.tensor(G[f"x_{n}_{d}"], device=dev)
    two, one = make(G, kind, n, d).to(dev), make(G, kind, n, d, two_event_dims=False).to(dev)
    assert tuple(two.event_shape) == (n, d) and tuple(one.event_shape) == (n * d,)
    u = two.energy(x)
    assert torch.equal(u, one.energy(x.reshape(-1, n * d)))
    ref = two._energy(x.double())
    for B in (1, 129):
        rows = torch.arange(B, device=dev) % x.shape[0]
        ub = two.energy(x[rows].contiguous())
        assert ub.shape == (B, 1)
        torch.testing.assert_close(ub.double(), ref[rows], rtol=1e-5, atol=1e-5)
        assert torch.equal(ub, u[rows])
    assert torch.equal(two.energy(x, temperature=2.0), u / 2)
    # outside the kernel: the class's own torch formula, no error
    wide = torch.cat([x, x], dim=-1)[..., :d]                # [B, n, d] view with a row stride of 2 d
    assert not wide.is_contiguous()
    torch.testing.assert_close(two.energy(wide), two._energy(wide), rtol=1e-6, atol=0)
    torch.testing.assert_close(two.energy(x.double()), ref, rtol=1e-12, atol=0)
    assert two.energy(x.double()).dtype == torch.float64
    torch.testing.assert_close(two.energy(x, temperature=torch.tensor(2.0, device=dev)), two._energy(x) / 2, rtol=1e-6, atol=0)
    big = make(G, kind, 65, d).to(dev)
    xb = torch.cat([x + 10.0 * k for k in range(5)], dim=1).contiguous()        # five copies of the cluster, 10 apart
    assert xb.shape[1] == 65
    torch.testing.assert_close(big.energy(xb), big._energy(xb), rtol=1e-6, atol=0)


def test_fused_kl_loss_path(hip_lib, dev, golden):
    """LJ13: the loss sums come out of the energy launch; no aten reduction kernel runs in the step"""
    from test_gpu_round6 import _device_kernel_names
    G = golden("particles")
    n, d, B = 13, 3, 600
    target = make(G, "lj", n, d, two_event_dims=False).to(dev)
    rows = torch.arange(B, device=dev) % 150
    x = torch.tensor(G[f"x_{n}_{d}"], device=dev).reshape(150, -1)[rows].contiguous()
    gen = torch.Generator(device="cpu").manual_seed(5)
    dlogp = torch.randn(B, 1, generator=gen).to(dev)

    xa, da = x.clone().requires_grad_(True), dlogp.clone().requires_grad_(True)
    res = kl_loss_sums(target, (xa,), da)
    assert res is not None, "a pair target over one tensor must give the fused loss sums"
    sums, u = res
    assert sums.dtype == torch.float64 and sums.shape == (2,) and u.shape == (B, 1)
    assert torch.equal(u, target.energy(x))
    expect = float((u.double() - dlogp.double()).mean())
    assert float(sums[1]) == B
    assert abs(float(sums[0] / sums[1]) - expect) <= 1e-6 * abs(expect)
    (sums[0] / sums[1]).backward()
    xb, db = x.clone().requires_grad_(True), dlogp.clone().requires_grad_(True)
    (target.energy(xb) - db).mean().backward()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(da.grad, db.grad, rtol=1e-6, atol=0)

    dl_inf = dlogp.clone()
    dl_inf[7] = -float("inf")
    xc = x.clone().requires_grad_(True)
    s2, _ = kl_loss_sums(target, (xc,), dl_inf, drop_nonfinite=True)
    assert float(s2[1]) == B - 1 and np.isfinite(float(s2[0]))
    s2[0].backward()
    assert float(xc.grad[7].abs().max()) == 0.0 and float(xc.grad[8].abs().max()) > 0.0

    def step():
        xa.grad = da.grad = None
        s, _ = kl_loss_sums(target, (xa,), da, drop_nonfinite=True)
        (s[0] / s[1]).backward()
    names = _device_kernel_names(step)
    print(sorted(set(n.split("(")[0][-70:] for n in names)))
    assert not [k for k in names if "reduce_kernel" in k and "energy_partial_reduce_kernel" not in k], names
    assert any("pair_energy_kernel" in k for k in names) and any("pair_energy_bwd_kernel" in k for k in names)
    assert any("energy_partial_reduce_kernel" in k for k in names)


def test_kl_training_on_dw4(hip_lib, dev, golden):
    """four affine couplings with mean-free shift networks, a mean-free normal prior and the DW4 target: 20 KLTrainer steps at batch
    512 keep the loss finite and lower it from the first to the last five-step mean"""
    from bgflow_amd.training import FlatAdam, KLTrainer
    G = golden("particles")
    torch.manual_seed(3)
    n, d = 4, 2
    half = n * d // 2
    layers = [bg.SplitFlow(half)]
    for _ in range(4):
        layers.append(bg.CouplingFlow(bg.AffineTransformer(
            shift_transformation=bg.MeanFreeDenseNet([half, 32, half], activation=torch.nn.ReLU()),
            scale_transformation=bg.DenseNet([half, 32, half], activation=torch.nn.Tanh()))))
        layers.append(bg.SwapFlow())
    layers.append(bg.MergeFlow(half))
    prior = bg.MeanFreeNormalDistribution(n * d, n, std=2.0, two_event_dims=False)
    target = make(G, "mdw", n, d, two_event_dims=False)
    gen = bg.BoltzmannGenerator(prior, bg.SequentialFlow(layers), target).to(dev)
    assert kl_loss_sums(target, (prior.sample(8),), torch.zeros(8, 1, device=dev)) is not None
    opt = FlatAdam([p for p in gen.parameters() if p.requires_grad], lr=5e-3)
    trainer = KLTrainer(gen, optim=opt, train_likelihood=False, train_energy=True)
    trainer.train(20, batchsize=512)
    _, _, ys = trainer.losses()
    kll = np.asarray(ys[0]).reshape(-1)
    print("KL loss:", kll)
    assert len(kll) == 20 and np.isfinite(kll).all(), kll
    assert kll[-5:].mean() < kll[:5].mean(), f"KL loss {kll[:5].mean():.3f} -> {kll[-5:].mean():.3f}"


def test_blocks_that_walk_several_tiles(hip_lib, dev, golden):
    """bgk_pair_energy_kl_sums with a workspace of two blocks at B = 600: the grid is clamped to nblk, a block walks five 64-row tiles
    and carries its loss partials across them; energies and sums equal those of the ten-block launch (2048-block workspace)"""
    from bgflow_amd import _lib
    G = golden("particles")
    n, d, B = 13, 3, 600
    eps, rm, osc = (float(v) for v in G["lj_params"])
    rows = torch.arange(B, device=dev) % 150
    x = torch.tensor(G[f"x_{n}_{d}"], device=dev).reshape(150, -1)[rows].contiguous()
    dlogp = torch.randn(B, generator=torch.Generator().manual_seed(9)).to(dev)
    dlogp[77] = -float("inf")
    out = []
    for nblk in (2048, 2):
        u = torch.empty(B, device=dev)
        partial = torch.full((nblk, 2), float("nan"), device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        st = hip_lib.bgk_pair_energy_kl_sums(_lib.ptr(x), n * d, B, n, d, 0, eps, rm, 0.0, 0.0, osc, 1.0, _lib.ptr(u), _lib.ptr(dlogp), 1,
                                             _lib.ptr(partial), nblk, _lib.ptr(sums), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_pair_energy_kl_sums")
        out.append((u, sums, partial))
    (u_a, s_a, _), (u_b, s_b, p_b) = out
    assert torch.equal(u_a, u_b) and torch.isfinite(p_b).all()
    assert float(s_b[1]) == B - 1 == float(s_a[1])
    keep = torch.arange(B, device=dev) != 77
    expect = float((u_b.double() - dlogp.double())[keep].sum())
    assert abs(float(s_b[0]) - expect) <= 1e-6 * abs(expect) and abs(float(s_a[0]) - expect) <= 1e-6 * abs(expect)


def test_backward_blocks_that_walk_several_tiles(hip_lib, dev, golden):
    """LJ55 at B = 4097 x 32 + 5: the backward kernel's 32-row tiles outnumber its 4096 workgroups, so the first blocks take a second
    tile (the last one partial); the rows of those tiles get the bits the same rows get in a batch of their own"""
    G = golden("particles")
    n, d = 55, 3
    B = 4097 * 32 + 5
    energy = make(G, "lj", n, d, two_event_dims=False).to(dev)
    x150 = torch.tensor(G[f"x_{n}_{d}"], device=dev).reshape(150, -1)
    x = x150[torch.arange(B, device=dev) % 150].contiguous().requires_grad_(True)
    weights = torch.linspace(0.5, 1.5, B, device=dev)[:, None]
    (g,) = torch.autograd.grad((energy.energy(x) * weights).sum(), x)
    tail = slice(4096 * 32 - 3, B)                       # the end of the first pass over the grid and everything after it
    xt = x.detach()[tail].clone().requires_grad_(True)
    (gt,) = torch.autograd.grad((energy.energy(xt) * weights[tail]).sum(), xt)
    assert torch.isfinite(g).all() and torch.equal(g[tail], gt)
    head = x.detach()[:64].clone().requires_grad_(True)
    (gh,) = torch.autograd.grad((energy.energy(head) * weights[:64]).sum(), head)
    assert torch.equal(g[:64], gh)
