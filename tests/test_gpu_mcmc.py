"""GPU (-m gpu): the fused Metropolis chains -- ``MCMCStep`` / ``IterativeSampler`` on bgk_pair_mcmc (csrc/bgk_mcmc.hip) -- against the
reference's recorded f64 chains on fixed random numbers (tests/golden/mcmc.npz, written by tests/golden/make_mcmc_goldens.py), and
bitwise against itself: in-kernel Philox = the same numbers handed in, sharded / chunked / capped runs = the run in one piece, returned
energies = ``energy.energy`` of the returned states.

Bounds of the parity test, on the chains the fixture keeps (f64 decision margin >= 1e-3 at every step; below it an f32 evaluation may
decide otherwise): accept counts equal; |x - x64| <= 4 err_x32 + 1e-6 and |e - e64| / (1 + |e64|) <= 4 err_e32 + 1e-6, err_* the errors of
the reference's own f32 run of the same chains -- the project's bound for the pair kernels (another summation order over up to 2016 pairs;
the floor for cases where the reference's f32 happens to be exact).

B = 150 (a partial last tile of either tile height: 64 rows, 41 rows at n d = 192; three workgroups)."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd.distributions import _kernel_plan, philox_sample

from mcmc_common import (B, CASES, N_FRAMES, N_STEPS, STRIDE, case_numbers, case_temperatures, make, random_numbers, recorded_uniforms,
                         run_general)

pytestmark = pytest.mark.gpu


def fused_sampler(energy, x0, std, temps, noise=None, unif=None, stride=STRIDE, n_steps=1, stream=None, **kwargs):
    step = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=std), target_temperatures=temps, n_steps=n_steps)
    if noise is not None:
        step.feed_noise(noise, unif)
    if stream is not None:
        step.set_philox_stream(stream)
    sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=stride, **kwargs)
    assert sampler._fused_setup() is not None, "the case must take the fused path"
    return sampler, step


@pytest.fixture(scope="module")
def chains(hip_lib, dev, golden):
    """a fixture case through IterativeSampler.sample(16) on the recorded numbers, computed once per case"""
    G, P = golden("mcmc"), golden("particles")

    @functools.lru_cache(maxsize=None)
    def run(kind, n, d):
        key = f"{kind}_{n}_{d}_"
        noise, unif = case_numbers(G, n, d)
        energy = make(P, kind, n, d).to(dev)
        x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
        start = x0.clone()
        sampler, step = fused_sampler(energy, x0, float(G[key + "std"]), case_temperatures(G, key, torch.float32, dev),
                                      torch.tensor(noise, device=dev), torch.tensor(unif, device=dev))
        frames = sampler.sample(N_FRAMES)
        assert torch.equal(x0, start), "the caller's start tensor is not touched"
        state = sampler.state.as_dict()
        return dict(frames=frames, x=state["samples"][0], e=state["energies"], up_to_date=state["energies_up_to_date"],
                    acc=step.n_accepted.clone(), n_proposed=step.n_proposed, energy=energy, i=sampler.i)

    return run


@pytest.mark.parametrize("kind,n,d", CASES)
def test_parity_on_recorded_numbers(chains, golden, kind, n, d):
    G = golden("mcmc")
    key = f"{kind}_{n}_{d}_"
    r = chains(kind, n, d)
    keep, rows = G[key + "keep"], G[key + "rows"]
    assert keep.mean() >= 0.85
    assert r["frames"].shape == (N_FRAMES, B, n * d) and r["n_proposed"] == N_STEPS and r["i"] == N_FRAMES and r["up_to_date"]
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


@pytest.mark.parametrize("kind,n,d", CASES)
def test_returned_energies_are_the_energy_kernels_bits(chains, kind, n, d):
    r = chains(kind, n, d)
    assert torch.equal(r["e"], r["energy"].energy(r["x"])[:, 0])


def philox_numbers(seed, offset, n_steps, batch, nd, dev):
    """what bgk_philox_fields writes for (seed, offset + s), fields [normal nd, uniform 1]"""
    noise, unif = [], []
    for s in range(n_steps):
        (eps, r), _ = philox_sample([(1, nd, None, None, 1.0, 0.0), (0, 1, None, None, 1.0, 0.0)], batch, dev, seed, offset + s)
        noise.append(eps)
        unif.append(r[:, 0])
    return torch.stack(noise), torch.stack(unif)


def step_seed(step):
    from bgflow_amd import dp
    st = step._philox_ids()
    return (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1), st[1]


# (53, 3): n d = 159, the widest row bgk_philox_fields writes (its LDS tile holds 160 columns) and, like (64, 3), a tile of fewer than 64
# rows (49); the counter layout at n d = 192 is checked against the numpy generator in test_philox_layout_at_the_widest_row
@pytest.mark.parametrize("kind,n,d", [("mdw", 4, 2), ("lj", 53, 3)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, kind, n, d):
    P = golden("particles")
    torch.manual_seed(1234)
    energy = make(P, kind, n, d).to(dev)
    if (n, d) == (53, 3):
        x0 = torch.tensor(P["x_55_3"], device=dev)[:, :53].reshape(B, -1).contiguous()
        std = 0.015
    else:
        x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
        std = 0.3
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    drawn, step_a = fused_sampler(energy, x0, std, temps, stream=40)
    step_a.set_philox_stream(40, calls=7)                                          # continue the stream at step 7
    seed, offset = step_seed(step_a)
    assert offset == 7
    fa = drawn.sample(N_FRAMES)
    assert step_a._philox_ids()[1] == 7 + N_STEPS                                  # the counter is the index of the next step
    noise, unif = philox_numbers(seed, offset, N_STEPS, B, n * d, dev)
    fed, step_b = fused_sampler(energy, x0, std, temps, noise, unif)
    fb = fed.sample(N_FRAMES)
    a, b = drawn.state.as_dict(), fed.state.as_dict()
    assert torch.equal(fa, fb) and torch.equal(a["samples"][0], b["samples"][0]) and torch.equal(a["energies"], b["energies"])
    assert torch.equal(step_a.n_accepted, step_b.n_accepted)
    rate = float(step_a.n_accepted.float().mean()) / N_STEPS
    assert 0.1 < rate < 0.95, rate                                                 # (a run that moves: the comparison is not of frozen chains)
    assert torch.equal(a["energies"], energy.energy(a["samples"][0])[:, 0])


def test_philox_layout_at_the_widest_row(hip_lib, dev):
    """n d = 192: one step from x = 0 with noise_std = 1 at a temperature that accepts everything leaves x = eps, the in-kernel normals
    -- the numpy restatement of the generator (oracle/philox.py) to 4e-6, the project's bound for Box-Muller in f32 against f64"""
    from oracle import philox
    n, d, rows, row0, offset = 64, 3, 100, 70, 5
    energy = bg.MeanFreeNormalDistribution(n * d, n, std=1.0, two_event_dims=False).to(dev)
    step = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=1.0), target_temperatures=1e30)
    step.set_philox_stream(3, calls=offset)
    step.chain_offset = row0
    seed, _ = step_seed(step)
    out = step(bg.SamplerState(samples=torch.zeros(rows, n * d, device=dev))).as_dict()
    assert int(step.n_accepted.sum()) == rows
    want = philox.sample_field(seed, offset, 0, rows, n * d, 1, row0=row0)
    np.testing.assert_allclose(out["samples"][0].cpu().numpy(), want, rtol=0, atol=4e-6)


@pytest.mark.parametrize("kind,n,d", [("lj", 13, 3), ("mdw", 64, 3)])
def test_independence_of_sharding_chunking_and_the_step_cap(hip_lib, dev, golden, monkeypatch, kind, n, d):
    G, P = golden("mcmc"), golden("particles")
    key = f"{kind}_{n}_{d}_"
    torch.manual_seed(99)
    energy = make(P, kind, n, d).to(dev)
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
    std = float(G[key + "std"])
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    whole, step_w = fused_sampler(energy, x0, std, temps, stream=50)
    fw = whole.sample(N_FRAMES)
    xw, ew = whole.state.as_dict()["samples"][0], whole.state.as_dict()["energies"]
    # chains 64..149 alone, told where they sit in the whole
    part, step_p = fused_sampler(energy, x0[64:].contiguous(), std, temps[64:].contiguous(), stream=50)     # the whole run's stream
    step_p.chain_offset = 64
    fp = part.sample(N_FRAMES)
    assert torch.equal(fp, fw[:, 64:]) and torch.equal(part.state.as_dict()["energies"], ew[64:])
    assert torch.equal(step_p.n_accepted, step_w.n_accepted[64:])
    # 48 steps in one launch = 16 launches of 3 steps, accept counts accumulated
    step_1 = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=std), target_temperatures=temps, n_steps=N_STEPS).set_philox_stream(50)
    one = step_1(bg.SamplerState(samples=x0)).as_dict()
    step_16 = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=std), target_temperatures=temps, n_steps=STRIDE).set_philox_stream(50)
    state = bg.SamplerState(samples=x0)
    for _ in range(N_FRAMES):
        state = step_16(state)
    many = state.as_dict()
    for got in (one, many):
        assert got["energies_up_to_date"]
        assert torch.equal(got["samples"][0], xw) and torch.equal(got["energies"], ew)
    assert torch.equal(step_1.n_accepted, step_w.n_accepted) and torch.equal(step_16.n_accepted, step_w.n_accepted)
    assert step_1.n_proposed == step_16.n_proposed == N_STEPS
    # a step cap of 5 (launches of 3 steps; with a stride of 7: pieces of 5 + 2) = the uncapped run
    wide, step_wide = fused_sampler(energy, x0, std, temps, stride=7, stream=50)
    f7 = wide.sample(4)
    monkeypatch.setattr(sampling, "MCMC_MAX_STEPS_PER_LAUNCH", 5)
    for stride, n_frames, want, want_acc in ((STRIDE, N_FRAMES, fw, step_w.n_accepted), (7, 4, f7, step_wide.n_accepted)):
        capped, step_c = fused_sampler(energy, x0, std, temps, stride=stride, stream=50)
        assert torch.equal(capped.sample(n_frames), want) and torch.equal(step_c.n_accepted, want_acc)


def test_sample_is_one_launch(hip_lib, dev, golden):
    from test_gpu_round6 import _device_kernel_names
    P = golden("particles")
    energy = make(P, "lj", 13, 3).to(dev)
    x0 = torch.tensor(P["x_13_3"], device=dev).reshape(B, -1)
    sampler, _ = fused_sampler(energy, x0, 0.03, 1.0, stream=60)
    names = _device_kernel_names(lambda: sampler.sample(N_FRAMES))
    print(names)
    assert len(names) == 1 and "pair_mcmc_kernel" in names[0], names


def test_coincident_particles_are_rejected(hip_lib, dev, golden):
    """explicit noise that puts particle 1 of chain 0 onto particle 0: the proposal's energy is huge (non-finite for eps -> 0), never accepted"""
    P = golden("particles")
    n, d = 4, 2
    energy = make(P, "lj", n, d).to(dev)
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)[:8].contiguous()
    steps = 6
    noise = torch.zeros(steps, 8, n * d, device=dev)
    noise[:, 0, 2:4] = x0[0, 0:2] - x0[0, 2:4]              # noise_std = 1: x_1 + (x_0 - x_1) = x_0
    noise[:, 1:] = 0.01 * torch.tensor(random_numbers(5, n * d, steps, 8)[0], device=dev)[:, 1:]
    unif = torch.full((steps, 8), 1e-30, device=dev)        # log r = -69: anything but a wall is accepted
    step = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=1.0), n_steps=steps).feed_noise(noise, unif)
    e0 = energy.energy(x0)[:, 0]
    out = step(bg.SamplerState(samples=x0)).as_dict()
    assert int(step.n_accepted[0]) == 0 and torch.equal(out["samples"][0][0], x0[0]) and torch.equal(out["energies"][0], e0[0])
    assert torch.isfinite(out["energies"]).all()
    assert (step.n_accepted[1:] == steps).all()             # the other chains moved
    # a start state that is itself non-finite in energy stays put under NaN proposals
    nan_noise = torch.full((1, 8, n * d), float("nan"), device=dev)
    stuck = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=1.0)).feed_noise(nan_noise, unif[:1].contiguous())
    out = stuck(bg.SamplerState(samples=x0)).as_dict()
    assert int(stuck.n_accepted.sum()) == 0 and torch.equal(out["samples"][0], x0)


def test_stationary_distribution_with_in_kernel_philox(hip_lib, dev):
    """mean-free normal of 4 particles in 2 dimensions, std 0.8: the variance of a centred coordinate at temperature T is
    T std^2 (n - 1) / n.  4096 chains at temperatures alternating 1 and 4, 500 burn-in steps, 50 frames 10 steps apart: 3 %"""
    torch.manual_seed(7)
    n_chains = 4096
    target = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False).to(dev)
    temps = torch.tensor([1.0, 4.0], device=dev).repeat(n_chains // 2)
    sampler, step = fused_sampler(target, torch.zeros(n_chains, 8, device=dev), 0.4, temps, stride=10, n_burnin=50, stream=70)
    assert sampler.i == 50 and step.n_proposed == 500
    frames = sampler.sample(50)
    assert frames.shape == (50, n_chains, 8) and step.n_proposed == 1000
    x = frames.reshape(50, n_chains, 4, 2)
    x = x - x.mean(dim=2, keepdim=True)
    for k, temp in enumerate((1.0, 4.0)):
        var = float(x[:, k::2].double().pow(2).mean())
        want = temp * 0.64 * 3 / 4
        print(f"T = {temp}: variance {var:.5f}, expected {want:.5f} ({var / want - 1:+.2%})")
        assert abs(var / want - 1) <= 0.03


def test_fallbacks_agree_with_the_general_rule(hip_lib, dev, golden, monkeypatch):
    G, P = golden("mcmc"), golden("particles")
    n, d = 4, 2
    key = f"mdw_{n}_{d}_"
    noise_np, unif_np = case_numbers(G, n, d)
    std = float(G[key + "std"])
    energy = make(P, "mdw", n, d).to(dev)
    x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
    noise, unif = torch.tensor(noise_np, device=dev), torch.tensor(unif_np, device=dev)
    ref_frames, ref_sampler, ref_step = run_general(energy, x0, noise, unif, std, 1.0)           # the general path in f32 on the device
    keep = torch.tensor(G[key + "keep"], device=dev)

    def same_as_general(frames, step):
        assert torch.equal(step.n_accepted[keep], ref_step.n_accepted[keep])
        assert torch.equal(frames[:, keep], ref_frames[:, keep])       # the same decisions on the same f32 operations: the same bits

    # the fused path itself takes the general path's decisions
    fused, step = fused_sampler(energy, x0, std, 1.0, noise, unif)
    same_as_general(fused.sample(N_FRAMES), step)
    # fused = False, on an instance and on the class, for a step that is otherwise fused: the general path runs (its acceptance draw,
    # torch.rand_like, is called once per step; the kernel never calls it)
    state = bg.SamplerState(samples=x0)

    def runs_general(step, st, n_steps=3):
        assert step._fused_setup(st) is None
        with recorded_uniforms(unif) as count:
            out = step(st).as_dict()
        assert count[0] == n_steps and step.n_proposed == n_steps
        assert out["samples"][0].shape == st.as_dict()["samples"][0].shape and out["samples"][0].dtype == st.as_dict()["samples"][0].dtype
        assert torch.isfinite(out["samples"][0]).all() and torch.isfinite(out["energies"]).all() and out["energies_up_to_date"]
        return out

    plain = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=3)
    assert plain._fused_setup(state) is not None
    with recorded_uniforms(unif) as count:
        plain(state)
    assert count[0] == 0 and plain.n_proposed == 3                     # fused: no torch.rand_like
    plain.fused = False
    plain.n_accepted, plain.n_proposed = None, 0
    runs_general(plain, state)
    assert bg.IterativeSampler(state, [plain])._fused_setup() is None
    del plain.fused
    assert plain._fused_setup(state) is not None
    monkeypatch.setattr(bg.MCMCStep, "fused", False)
    other = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=3)
    runs_general(other, state)
    assert bg.IterativeSampler(state, [other])._fused_setup() is None
    frames, sampler, step = run_general(energy, x0, noise, unif, std, 1.0)
    assert torch.equal(frames, ref_frames)
    monkeypatch.undo()
    assert other._fused_setup(state) is not None
    # f64 input with a plain GaussianProposal
    out = runs_general(bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=3), bg.SamplerState(samples=x0.double()))
    assert out["samples"][0].dtype == torch.float64 and out["energies"].dtype == torch.float64
    # a subclassed proposal

    class MyProposal(bg.GaussianProposal):
        pass

    step = bg.MCMCStep(energy, proposal=MyProposal(std))
    assert step._fused_setup(bg.SamplerState(samples=x0)) is None
    out = step(bg.SamplerState(samples=x0)).as_dict()
    assert out["samples"][0].shape == x0.shape and torch.isfinite(out["energies"]).all()
    # f64 input on recorded numbers: the fixture's chains to 1e-12
    frames, sampler, step = run_general(energy, x0.double(), noise, unif, std, 1.0)
    assert frames.dtype == torch.float64 and np.array_equal(step.n_accepted.cpu().numpy(), G[key + "acc"])
    assert np.abs(frames[:, :8].cpu().numpy() - G[key + "frames64"]).max() <= 1e-12
    # a non-contiguous view
    wide = torch.zeros(B, 2 * n * d, device=dev)
    wide[:, ::2] = x0
    view = wide[:, ::2]
    plain = bg.MCMCStep(energy, proposal=bg.GaussianProposal(std), n_steps=3)
    assert not view.is_contiguous() and plain._fused_setup(bg.SamplerState(samples=view)) is None
    out = plain(bg.SamplerState(samples=view)).as_dict()
    assert out["samples"][0].shape == x0.shape
    assert torch.allclose(out["energies"], energy.energy(out["samples"][0])[:, 0], rtol=1e-5, atol=1e-5)
    # 65 particles: outside the kernel's envelope
    big = bg.LennardJonesPotential(65 * 3, 65, two_event_dims=False).to(dev)
    xb = 1.2 * torch.stack(torch.meshgrid(*[torch.arange(5.0, device=dev)] * 3, indexing="ij"), -1).reshape(-1, 3)[:65].reshape(1, -1).repeat(6, 1)
    step = bg.MCMCStep(big, proposal=bg.GaussianProposal(0.01), n_steps=2)
    assert _kernel_plan(big, 1.0) is None and step._fused_setup(bg.SamplerState(samples=xb)) is None
    out = step(bg.SamplerState(samples=xb)).as_dict()
    assert out["samples"][0].shape == (6, 195) and torch.isfinite(out["energies"]).all()
    # a box constraint (a samples hook)
    boxed = bg.GaussianMCMCSampler(energy, x0, noise_std=std, box_constraint=lambda t: t.clamp(-6.0, 6.0))
    assert boxed._fused_setup() is None
    res = boxed.sample(2)
    assert res.shape == (2 * B, n * d) and float(res.abs().max()) <= 6.0
    # ... and without one the shortcut class is fused
    assert bg.GaussianMCMCSampler(energy, x0, noise_std=std)._fused_setup() is not None
    # the reference's own test shape (tests/distribution/sampling/test_mcmc.py): a NormalDistribution target over the last dimension,
    # samples [B, 3, 4], temperatures [3] broadcast against energies [B, 3]; mean and per-temperature std to that test's tolerances
    torch.manual_seed(11)
    normal = bg.NormalDistribution(4, mean=3.0 * torch.ones(4)).to(dev)
    temps = torch.tensor([1.0, 2.0, 4.0], device=dev)
    sampler = bg.IterativeSampler(bg.SamplerState(samples=torch.zeros(512, 3, 4, device=dev)),
                                  [bg.MCMCStep(normal, proposal=bg.GaussianProposal(noise_std=0.5), target_temperatures=temps)],
                                  stride=2, n_burnin=100)
    assert sampler._fused_setup() is None
    res = sampler.sample(100)
    assert res.shape == (100, 512, 3, 4) and torch.isfinite(res).all()
    assert sampler.sampler_steps[0].n_accepted.shape == (512, 3)
    assert torch.allclose(res.mean(dim=(0, 1, 3)), torch.full((3,), 3.0, device=dev), atol=0.1)
    assert torch.allclose(res.std(dim=(0, 1, 3)), temps.sqrt(), rtol=0.05, atol=0.0)


def test_progress_bar_counts_iterations_on_the_fused_path(hip_lib, dev, golden, monkeypatch):
    """``progress_bar`` is handed range(n) and advanced once per iteration, as on the general path, however the run is split into launches"""
    P = golden("particles")
    energy = make(P, "mdw", 4, 2).to(dev)
    x0 = torch.tensor(P["x_4_2"], device=dev).reshape(B, -1)
    seen = []

    def bar(it):
        seen.append([len(it), 0])
        for v in it:
            seen[-1][1] += 1
            yield v

    monkeypatch.setattr(sampling, "MCMC_MAX_STEPS_PER_LAUNCH", 4)
    sampler, step = fused_sampler(energy, x0, 0.3, 1.0, stream=90, n_burnin=2, progress_bar=bar)
    assert sampler.sample(5).shape == (5, B, 8)
    next(sampler)
    assert seen == [[2, 2], [5, 5]] and sampler.i == 8 and step.n_proposed == 8 * STRIDE


def test_three_dimensional_samples_and_carried_energies(hip_lib, dev, golden):
    """samples [B, n, d] of a two_event_dims target take the fused path; up-to-date energies of the state are used, not recomputed"""
    P = golden("particles")
    n, d = 13, 3
    torch.manual_seed(5)
    two = make(P, "lj", n, d, two_event_dims=True).to(dev)
    flat = make(P, "lj", n, d).to(dev)
    x3 = torch.tensor(P[f"x_{n}_{d}"], device=dev)
    assert x3.shape == (B, n, d)
    s3, st3 = fused_sampler(two, x3, 0.03, 2.0, stream=80)
    s2, st2 = fused_sampler(flat, x3.reshape(B, -1), 0.03, 2.0, stream=80)
    f3, f2 = s3.sample(4), s2.sample(4)
    assert f3.shape == (4, B, n, d) and torch.equal(f3.reshape(4, B, -1), f2)
    assert s3.state.as_dict()["samples"][0].shape == (B, n, d)
    # carried energies: a state whose (wrong) energies are marked up to date starts from them -- at +1e4 every first proposal is accepted
    step = bg.MCMCStep(flat, proposal=bg.GaussianProposal(0.03)).set_philox_stream(82)
    lifted = bg.SamplerState(samples=x3.reshape(B, -1)).replace(energies=torch.full((B,), 1e4, device=dev))
    assert lifted.as_dict()["energies_up_to_date"]
    out = step(lifted).as_dict()
    assert int(step.n_accepted.sum()) == B and torch.equal(out["energies"], flat.energy(out["samples"][0])[:, 0])
    # the stream and its position travel in the state dict
    sd = st3.state_dict()
    assert sd["_philox_state"].tolist() == [80, 4 * STRIDE]
