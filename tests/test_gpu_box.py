"""GPU (-m gpu): the particle box -- ``RepulsiveParticles`` / ``HarmonicParticles`` on bgk_box_energy / _backward / _kl_sums / bgk_box_mcmc
(csrc/bgk_pair.hip, bgk_mcmc.hip, bgk_pair_terms.h) -- through the public classes, against the reference's recorded f64 results and chains
(tests/golden/box.npz, written by tests/golden/make_box_goldens.py), and the chains bitwise against themselves.

Bounds, the project's for the pair kernels: err(v) = max_b |v_b - u64_b| / (1 + |u64_b|) <= 4 err(reference f32) + 1e-6; gradients relative
to 1 + max |g64| against four times the error of the reference's f32 autograd (harm: of the fixture's own i < j statement; the reference's
autograd is NaN there); chains on the kept rows (f64 decision margin >= 1e-3): accept counts equal, |x - x64| <= 4 err_x32 + 1e-6, energies
likewise.

Shapes are the fixture's: B = 150 (a partial last tile of either height), 2, 4, 38 and 64 particles (64- and 32-row backward tiles)."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd.distributions import BoxPlan, _kernel_plan, kl_loss_sums

from box_common import B, KINDS, MC_NSOLVENT, NSOLVENT, err_g, err_u, make
from mcmc_common import N_FRAMES, N_STEPS, STRIDE, case_temperatures, random_numbers
from test_gpu_mcmc import fused_sampler, philox_numbers, step_seed

pytestmark = pytest.mark.gpu


def energy_and_grad(energy, x):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x)
    assert u.shape == (x.shape[0], 1)
    u.sum().backward()
    return u.detach().cpu().numpy().reshape(-1), x.grad.cpu().numpy().reshape(x.shape[0], -1)


@pytest.fixture(scope="module")
def results(hip_lib, dev, golden):
    """energies, gradients and forces of a golden case through the public class, computed once per case"""
    G = golden("box")

    @functools.lru_cache(maxsize=None)
    def run(kind, ns):
        x = torch.tensor(G[f"x_{ns}"], device=dev)
        energy = make(G, kind, ns).to(dev)
        assert isinstance(_kernel_plan(energy, 1.0), BoxPlan)
        u, g = energy_and_grad(energy, x)
        return u, g, energy.force(x).cpu().numpy()

    return run


@pytest.mark.parametrize("ns", NSOLVENT)
@pytest.mark.parametrize("kind", KINDS)
def test_energy_parity(results, golden, kind, ns):
    G = golden("box")
    key = f"{kind}_{ns}"
    u = results(kind, ns)[0]
    e, ref = err_u(u, G[key + "_u64"]), float(G[key + "_err_u32"])
    print(f"{key}: energy error {e:.3g} (the reference's f32: {ref:.3g})")
    assert e <= 4 * ref + 1e-6


@pytest.mark.parametrize("ns", NSOLVENT)
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_and_force_parity(results, golden, kind, ns):
    G = golden("box")
    key = f"{kind}_{ns}"
    _, g, force = results(kind, ns)
    assert np.isfinite(g).all() and np.isfinite(force).all()
    rows = G[key + "_g_rows"]
    e, ref = err_g(g[rows], G[key + "_g64"]), float(G[key + "_err_g32"])
    print(f"{key}: gradient error {e:.3g} (f32 autograd: {ref:.3g})")
    assert e <= 4 * ref + 1e-6
    assert np.array_equal(force, -g)                      # the same launch with g_u = -1
    if key + "_force64" in G:                             # the reference's analytic force
        assert err_g(force[rows], G[key + "_force64"]) <= 4 * ref + 1e-6


def test_harmonic_dense_38(hip_lib, dev, golden):
    """The fixture's 38-particle lattice (spacing 1.15) brings only 96 pairs of the whole batch within rc = 0.9.  Scaled by 0.8 (spacing
    0.92, jitter 0.12) about half of the lattice neighbours are: the harmonic pair term and its gradient at the real system's shape, the
    64-row backward tile with S = 77.  No recording of the reference exists for these positions; the yardstick is the class's own torch
    formulas in f64 (test_host_box.py ties them to the reference to 1e-10), and the bound the pair kernels' with those formulas' f32
    error in the reference's place: err <= 4 err(torch f32) + 1e-6, normalised as above."""
    G = golden("box")
    energy = make(G, "harm", 36).to(dev)
    x = torch.tensor(G["x_36"], device=dev) * 0.8
    xp = x.double().reshape(B, 38, 2)
    i, j = torch.triu_indices(38, 38, offset=1, device=dev)
    close = (xp[:, i[1:]] - xp[:, j[1:]]).pow(2).sum(-1).sqrt() < energy.params["rc"]
    per_sample = close.sum(dim=1)
    print(f"pairs within rc: {float(close.double().mean()):.4f} of all, {int(per_sample.min())} .. {int(per_sample.max())} per sample")
    assert int(per_sample.min()) >= 10 and float(close.double().mean()) <= 0.95
    u64, g64 = energy_and_grad(energy, x.double())          # f64: the torch path
    u32, g32 = energy_and_grad(_TorchFormulas(energy).to(dev), x)
    u, g = energy_and_grad(energy, x)
    ref_u, ref_g = err_u(u32, u64), err_g(g32, g64)
    e_u, e_g = err_u(u, u64), err_g(g, g64)
    print(f"harm_36 x 0.8: energy error {e_u:.3g} (torch f32: {ref_u:.3g}), gradient error {e_g:.3g} (torch f32: {ref_g:.3g})")
    assert e_u <= 4 * ref_u + 1e-6
    assert e_g <= 4 * ref_g + 1e-6
    assert np.array_equal(energy.force(x).cpu().numpy(), -g)


class _TorchFormulas(bg.Energy):
    """a target's own torch formulas, whatever the input"""

    def __init__(self, inner):
        super().__init__(inner.dim)
        self.inner = inner

    def _energy(self, x):
        return self.inner._energy(x)


@pytest.mark.parametrize("kind", KINDS)
def test_force_is_one_backward_launch(hip_lib, dev, golden, kind):
    from test_gpu_round6 import _device_kernel_names
    G = golden("box")
    energy = make(G, kind, 36).to(dev)
    x = torch.tensor(G["x_36"], device=dev)
    names = [k for k in _device_kernel_names(lambda: energy.force(x)) if "fill" not in k.lower() and "elementwise" not in k.lower()]
    print(names)
    assert len(names) == 1 and "pair_energy_bwd_kernel" in names[0], names
    names = _device_kernel_names(lambda: energy.energy(x))
    assert len(names) == 1 and "pair_energy_kernel" in names[0], names


@pytest.mark.parametrize("kind", KINDS)
def test_temperature_and_fallbacks(hip_lib, dev, golden, kind):
    G = golden("box")
    ns = 36
    energy = make(G, kind, ns).to(dev)
    x = torch.tensor(G[f"x_{ns}"], device=dev)
    u = energy.energy(x)
    # u = f32(e) * f32(1 / T) against f32(e) / T: the reciprocal's, the product's and the quotient's rounding, 3 x 2^-24 < 2^-22
    ut = energy.energy(x, temperature=2.5)
    assert float(((ut - u / 2.5).abs() / u.abs()).max()) <= 2.0 ** -22
    assert torch.equal(energy.energy(x, temperature=2.0), u / 2)
    for rows in (1, 129):
        idx = torch.arange(rows, device=dev) % B
        assert torch.equal(energy.energy(x[idx].contiguous()), u[idx])
    # outside the kernel: the class's own torch formulas, no error
    ref = energy._energy(x.double())
    u64 = energy.energy(x.double())
    assert u64.dtype == torch.float64
    torch.testing.assert_close(u64, ref, rtol=1e-12, atol=0)
    assert err_u(u64.cpu().numpy().reshape(-1), G[f"{kind}_{ns}_u64"]) <= 1e-10
    torch.testing.assert_close(u.double(), ref, rtol=1e-5, atol=1e-5)
    wide = torch.zeros(B, 2 * x.shape[1], device=dev)
    wide[:, ::2] = x
    view = wide[:, ::2]
    assert not view.is_contiguous()
    torch.testing.assert_close(energy.energy(view), energy._energy(view), rtol=1e-6, atol=0)
    torch.testing.assert_close(energy.energy(view), u, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(energy.force(view), energy.force(x), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(energy.force(x.double()), energy.force(x).double(), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(energy.energy(x, temperature=torch.tensor(2.0, device=dev)), energy._energy(x) / 2, rtol=1e-6, atol=0)
    big = make(G, kind, 63).to(dev)                      # 65 particles
    assert _kernel_plan(big, 1.0) is None
    xb = torch.cat([x[:, :54] + 0.4, x], dim=1).contiguous()
    assert xb.shape[1] == 130
    torch.testing.assert_close(big.energy(xb), big._energy(xb), rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", KINDS)
def test_singular_geometry(hip_lib, dev, golden, kind):
    """samples 0 and 1: two coincident solvent particles; sample 2: the dimer 0.3 apart, which no pair term sees"""
    G = golden("box")
    key = f"edge_{kind}"
    energy = make(G, kind, 2).to(dev)
    x = torch.tensor(G[key + "_x"], device=dev)
    u, g = energy_and_grad(energy, x)
    u64 = G[key + "_u64"]
    fin = np.isfinite(u64)
    assert fin[2] and (np.isfinite(u) == fin).all() and (u[~fin] == np.inf).all()
    assert err_u(u[fin], u64[fin]) <= 4 * float(G[key + "_err_u32"]) + 1e-6
    assert abs(float(u[2]) - u64[2]) / (1 + abs(u64[2])) <= 4 * float(G[key + "_err_u32"]) + 1e-6
    assert err_g(g[fin], G[key + "_g64"][fin]) <= 4 * float(G[key + "_err_g32"]) + 1e-6
    if kind == "harm":
        assert fin.all() and np.isfinite(g).all()        # the coincident pair: the gradient 0, what is left matches g64 (above)
    # the loss sums over this batch
    dlogp = torch.linspace(-1.0, 1.0, 8, device=dev)[:, None]
    sums, uk = kl_loss_sums(energy, (x,), dlogp, drop_nonfinite=True)
    assert int(sums[1]) == int(fin.sum()) == (6 if kind == "rep" else 8)
    want = (u64 - dlogp.cpu().numpy().reshape(-1).astype(np.float64))[fin].sum()
    assert abs(float(sums[0]) - want) <= (4 * float(G[key + "_err_u32"]) + 1e-6) * (1 + np.abs(u64[fin])).sum()


@pytest.mark.parametrize("ns", [2, 36, 62])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_kl_loss_sums(hip_lib, dev, golden, kind, ns):
    G = golden("box")
    key = f"{kind}_{ns}"
    target = make(G, kind, ns).to(dev)
    x = torch.tensor(G[f"x_{ns}"], device=dev)
    dlogp = torch.randn(B, 1, generator=torch.Generator().manual_seed(5)).to(dev)
    xa, da = x.clone().requires_grad_(True), dlogp.clone().requires_grad_(True)
    res = kl_loss_sums(target, (xa,), da, temperature=1.5)
    assert res is not None, "a box target over one tensor must give the fused loss sums"
    sums, u = res
    assert sums.dtype == torch.float64 and sums.shape == (2,) and u.shape == (B, 1) and float(sums[1]) == B
    assert torch.equal(u, target.energy(x, temperature=1.5))
    u64 = G[key + "_u64"] / 1.5
    want = (u64 - dlogp.cpu().numpy().reshape(-1).astype(np.float64)).sum()
    bound = (4 * float(G[key + "_err_u32"]) + 1e-6) * (1 + np.abs(u64)).sum() + 2.0 ** -24 * np.abs(dlogp.cpu().numpy()).sum()
    assert abs(float(sums[0]) - want) <= bound
    (sums[0] / sums[1]).backward()
    xb = x.clone().requires_grad_(True)
    target.energy(xb, temperature=1.5).mean().backward()             # the plain backward: the same arithmetic, g_row = 1 / B
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-6, atol=0)  # the same arithmetic but for the rounding of g_row = 1 / B
    torch.testing.assert_close(da.grad, torch.full_like(dlogp, -1.0 / B), rtol=1e-6, atol=0)


def test_kl_training_keeps_the_fused_loss_path(hip_lib, dev, golden):
    """a RealNVP generator on the 4-particle box: KLTrainer steps run, the loss is finite, and the loss sums come from the pair kernel"""
    from test_gpu_round6 import _device_kernel_names
    from bgflow_amd.training import FlatAdam, KLTrainer
    G = golden("box")
    torch.manual_seed(3)
    target = make(G, "harm", 2)
    dim, half = 8, 4
    layers = [bg.SplitFlow(half)]
    for _ in range(2):
        layers.append(bg.CouplingFlow(bg.AffineTransformer(
            shift_transformation=bg.DenseNet([half, 32, half], activation=torch.nn.ReLU()),
            scale_transformation=bg.DenseNet([half, 32, half], activation=torch.nn.Tanh()))))
        layers.append(bg.SwapFlow())
    layers.append(bg.MergeFlow(half))
    gen = bg.BoltzmannGenerator(bg.NormalDistribution(dim), bg.SequentialFlow(layers), target).to(dev)
    opt = FlatAdam([p for p in gen.parameters() if p.requires_grad], lr=1e-3)
    trainer = KLTrainer(gen, optim=opt, train_likelihood=False, train_energy=True)
    names = _device_kernel_names(lambda: trainer.train(1, batchsize=256))         # (runs its argument three times)
    _, _, ys = trainer.losses()
    kll = np.asarray(ys[0]).reshape(-1)
    assert len(kll) == 3 and np.isfinite(kll).all(), kll
    assert any("pair_energy_kernel" in k for k in names) and any("pair_energy_bwd_kernel" in k for k in names), sorted(set(names))
    assert any("energy_partial_reduce_kernel" in k for k in names)


# ---- chains -------------------------------------------------------------------------------------------------------------------------
def case_numbers(G, ns):
    nd = 2 * (ns + 2)
    noise, unif = random_numbers(int(G["seed_mc"]), nd)
    assert abs(noise.astype(np.float64).sum() - float(G[f"noise_sum_{ns}"])) <= 1e-9 * noise.size
    assert float(np.abs(noise).max()) == float(G[f"noise_absmax_{ns}"])
    assert abs(unif.astype(np.float64).sum() - float(G["unif_sum"])) <= 1e-12 * unif.size and float(unif.max()) == float(G["unif_absmax"])
    return noise, unif


@pytest.fixture(scope="module")
def chains(hip_lib, dev, golden):
    """a fixture case through IterativeSampler.sample(16) on the recorded numbers, computed once per case"""
    G = golden("box")

    @functools.lru_cache(maxsize=None)
    def run(kind, ns):
        key = f"mc_{kind}_{ns}_"
        noise, unif = case_numbers(G, ns)
        energy = make(G, kind, ns).to(dev)
        x0 = torch.tensor(G[f"x_{ns}"], device=dev)
        start = x0.clone()
        sampler, step = fused_sampler(energy, x0, float(G[key + "std"]), case_temperatures(G, key, torch.float32, dev),
                                      torch.tensor(noise, device=dev), torch.tensor(unif, device=dev))
        frames = sampler.sample(N_FRAMES)
        assert torch.equal(x0, start), "the caller's start tensor is not touched"
        state = sampler.state.as_dict()
        return dict(frames=frames, x=state["samples"][0], e=state["energies"], up_to_date=state["energies_up_to_date"],
                    acc=step.n_accepted.clone(), n_proposed=step.n_proposed, energy=energy, i=sampler.i)

    return run


@pytest.mark.parametrize("ns", MC_NSOLVENT)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_parity_on_recorded_numbers(chains, golden, kind, ns):
    G = golden("box")
    key = f"mc_{kind}_{ns}_"
    r = chains(kind, ns)
    keep, rows = G[key + "keep"], G[key + "rows"]
    assert keep.mean() >= 0.85
    assert r["frames"].shape == (N_FRAMES, B, 2 * (ns + 2)) and r["n_proposed"] == N_STEPS and r["i"] == N_FRAMES and r["up_to_date"]
    acc = r["acc"].cpu().numpy()
    assert acc.dtype == np.int32 and np.array_equal(acc[keep], G[key + "acc"][keep])
    x, e, frames = r["x"].cpu().numpy().astype(np.float64), r["e"].cpu().numpy().astype(np.float64), r["frames"].cpu().numpy().astype(np.float64)
    bound_x, bound_e = 4 * float(G[key + "err_x32"]) + 1e-6, 4 * float(G[key + "err_e32"]) + 1e-6
    err_x = np.abs(x[rows] - G[key + "x64"])[keep[rows]].max()
    err_f = np.abs(frames[:, :8] - G[key + "frames64"])[:, keep[:8]].max()
    err_e = (np.abs(e - G[key + "e64"]) / (1 + np.abs(G[key + "e64"])))[keep].max()
    print(f"{key[:-1]}: kept {int(keep.sum())} / {B}; |dx| {err_x:.3g}, frames {err_f:.3g} (bound {bound_x:.3g}); energy {err_e:.3g} (bound {bound_e:.3g})")
    assert err_x <= bound_x and err_f <= bound_x and err_e <= bound_e
    assert np.array_equal(frames[-1], x)


@pytest.mark.parametrize("ns", MC_NSOLVENT)
@pytest.mark.parametrize("kind", KINDS)
def test_returned_energies_are_the_energy_kernels_bits(chains, kind, ns):
    r = chains(kind, ns)
    assert torch.equal(r["e"], r["energy"].energy(r["x"])[:, 0])


@pytest.mark.parametrize("kind,ns", [("harm", 2), ("rep", 36)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, kind, ns):
    G = golden("box")
    torch.manual_seed(1234)
    energy = make(G, kind, ns).to(dev)
    x0 = torch.tensor(G[f"x_{ns}"], device=dev)
    std = float(G[f"mc_{kind}_{ns}_std"])
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    drawn, step_a = fused_sampler(energy, x0, std, temps, stream=40)
    step_a.set_philox_stream(40, calls=7)
    seed, offset = step_seed(step_a)
    fa = drawn.sample(N_FRAMES)
    noise, unif = philox_numbers(seed, offset, N_STEPS, B, x0.shape[1], dev)
    fed, step_b = fused_sampler(energy, x0, std, temps, noise, unif)
    fb = fed.sample(N_FRAMES)
    a, b = drawn.state.as_dict(), fed.state.as_dict()
    assert torch.equal(fa, fb) and torch.equal(a["samples"][0], b["samples"][0]) and torch.equal(a["energies"], b["energies"])
    assert torch.equal(step_a.n_accepted, step_b.n_accepted)
    rate = float(step_a.n_accepted.float().mean()) / N_STEPS
    assert 0.1 < rate < 0.95, rate
    assert torch.equal(a["energies"], energy.energy(a["samples"][0])[:, 0])


@pytest.mark.parametrize("kind,ns", [("rep", 2), ("harm", 62)])
def test_independence_of_sharding_and_the_split_into_launches(hip_lib, dev, golden, monkeypatch, kind, ns):
    G = golden("box")
    torch.manual_seed(99)
    energy = make(G, kind, ns).to(dev)
    x0 = torch.tensor(G[f"x_{ns}"], device=dev)
    std = float(G[f"mc_{kind}_{ns}_std"])
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    whole, step_w = fused_sampler(energy, x0, std, temps, stream=50)
    fw = whole.sample(N_FRAMES)
    xw, ew = whole.state.as_dict()["samples"][0], whole.state.as_dict()["energies"]
    # chains 64..149 alone, told where they sit in the whole (row0)
    part, step_p = fused_sampler(energy, x0[64:].contiguous(), std, temps[64:].contiguous(), stream=50)
    step_p.chain_offset = 64
    fp = part.sample(N_FRAMES)
    assert torch.equal(fp, fw[:, 64:]) and torch.equal(part.state.as_dict()["energies"], ew[64:])
    assert torch.equal(step_p.n_accepted, step_w.n_accepted[64:])
    # 48 steps in one launch = two launches of 24 steps, accept counts accumulated
    step_1 = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=std), target_temperatures=temps, n_steps=N_STEPS).set_philox_stream(50)
    one = step_1(bg.SamplerState(samples=x0)).as_dict()
    step_2 = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=std), target_temperatures=temps, n_steps=N_STEPS // 2).set_philox_stream(50)
    many = step_2(step_2(bg.SamplerState(samples=x0))).as_dict()
    for got in (one, many):
        assert got["energies_up_to_date"] and torch.equal(got["samples"][0], xw) and torch.equal(got["energies"], ew)
    assert torch.equal(step_1.n_accepted, step_w.n_accepted) and torch.equal(step_2.n_accepted, step_w.n_accepted)
    # the step cap splits a run the same way
    monkeypatch.setattr(sampling, "MCMC_MAX_STEPS_PER_LAUNCH", 5)
    capped, step_c = fused_sampler(energy, x0, std, temps, stream=50)
    assert torch.equal(capped.sample(N_FRAMES), fw) and torch.equal(step_c.n_accepted, step_w.n_accepted)


def test_sample_is_one_launch_of_the_chain_kernel(hip_lib, dev, golden):
    from test_gpu_round6 import _device_kernel_names
    G = golden("box")
    energy = make(G, "rep", 36).to(dev)
    sampler, _ = fused_sampler(energy, torch.tensor(G["x_36"], device=dev), 0.02, 1.0, stream=60)
    names = _device_kernel_names(lambda: sampler.sample(N_FRAMES))
    assert len(names) == 1 and "pair_mcmc_kernel" in names[0], names
    assert bg.GaussianMCMCSampler(energy, torch.tensor(G["x_36"], device=dev), noise_std=0.02)._fused_setup() is not None


def test_stochastic_layers_take_their_torch_paths_on_the_device(hip_lib, dev, golden):
    G = golden("box")
    rep = make(G, "rep", 2).to(dev)
    x = torch.tensor(G["x_2"], device=dev)[:16].contiguous()
    torch.manual_seed(3)
    for flow in (bg.BrownianFlow(rep, nsteps=2, stepsize=1e-4), bg.MetropolisMCFlow(rep, nsteps=2, stepsize=0.02)):
        assert flow._fused_setup(x) is None
        y, dW = flow(x)
        assert y.shape == x.shape and torch.isfinite(y).all() and torch.isfinite(dW).all()
    xg = x.clone().requires_grad_(True)
    y, dW = bg.BrownianFlow(rep, nsteps=2, stepsize=1e-4)(xg)
    (g,) = torch.autograd.grad(y.sum() + dW.sum(), xg)
    assert torch.isfinite(g).all()
