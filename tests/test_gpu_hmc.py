"""GPU (-m gpu): the fused Hamiltonian Monte Carlo chains -- ``HMCStep`` / ``IterativeSampler`` on bgk_pair_hmc / bgk_box_hmc
(csrc/bgk_hmc.hip) -- against the recorded f64 chains on fixed random numbers (tests/golden/hmc.npz, written by
tests/golden/make_hmc_goldens.py), and bitwise against itself: in-kernel Philox = the same numbers handed in, sharded / chunked / capped
runs = the run in one piece, a row alone = the row in its batch, returned energies = ``energy.energy`` of the returned states.

Bounds of the parity test, on the chains the fixture keeps (f64 decision margin >= 1e-3 at every step; below it an f32 evaluation may
decide otherwise): accept counts equal; |x - x64| <= 4 err_x32 + 1e-6 and |e - e64| / (1 + |e64|) <= 4 err_e32 + 1e-6, err_* the errors of
the fixture script's own f32 run of the same chains -- the project's bound for the pair kernels.

B = 150 (a partial last tile of every tile height: 64 rows, 16 rows at n d = 192, 24 rows for the box of 64)."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd.distributions import _kernel_plan

from hmc_common import B, CASES, IDS, N_FRAMES, N_STEPS, STRIDE, case_numbers, case_settings, key_of, make, recorded_normals
from mcmc_common import make as make_pair
from mcmc_common import random_numbers, recorded_uniforms
from test_gpu_mcmc import philox_numbers, step_seed

pytestmark = pytest.mark.gpu


def fused_sampler(energy, x0, settings, noise=None, unif=None, stride=STRIDE, n_steps=1, stream=None, fused="always", **kwargs):
    h, L, m, temps = settings
    step = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, target_temperatures=temps, n_steps=n_steps)
    step.fused = fused                 # "always": the kernel also at the shapes where it is not the default
    if noise is not None:
        step.feed_noise(noise, unif)
    if stream is not None:
        step.set_philox_stream(stream)
    sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=stride, **kwargs)
    assert sampler._fused_setup() is not None, "the case must take the fused path"
    return sampler, step


@pytest.fixture(scope="module")
def chains(hip_lib, dev, golden):
    """a fixture case through IterativeSampler.sample(6) on the recorded numbers, computed once per case"""
    G = golden("hmc")

    @functools.lru_cache(maxsize=None)
    def run(case):
        key = key_of(case)
        energy, x_np = make(golden, case)
        energy = energy.to(dev)
        noise, unif = case_numbers(golden, case, x_np.shape[1])
        x0 = torch.tensor(x_np, device=dev)
        start = x0.clone()
        sampler, step = fused_sampler(energy, x0, case_settings(G, key, torch.float32, dev), torch.tensor(noise, device=dev),
                                      torch.tensor(unif, device=dev))
        frames = sampler.sample(N_FRAMES)
        assert torch.equal(x0, start), "the caller's start tensor is not touched"
        state = sampler.state.as_dict()
        return dict(frames=frames, x=state["samples"][0], e=state["energies"], up_to_date=state["energies_up_to_date"],
                    acc=step.n_accepted.clone(), n_proposed=step.n_proposed, energy=energy, i=sampler.i)

    return run


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_on_recorded_numbers(chains, golden, case):
    G, key = golden("hmc"), key_of(case)
    r = chains(case)
    keep, rows = G[key + "keep"], G[key + "rows"]
    assert keep.mean() >= 0.85
    nd = r["x"].shape[1]
    assert r["frames"].shape == (N_FRAMES, B, nd) and r["n_proposed"] == N_STEPS == 12 and r["i"] == N_FRAMES and r["up_to_date"]
    acc = r["acc"].cpu().numpy()
    x, e, frames = r["x"].cpu().numpy().astype(np.float64), r["e"].cpu().numpy().astype(np.float64), r["frames"].cpu().numpy().astype(np.float64)
    bound_x, bound_e = 4 * float(G[key + "err_x32"]) + 1e-6, 4 * float(G[key + "err_e32"]) + 1e-6
    err_x = np.abs(x[rows] - G[key + "x64"])[keep[rows]].max()
    err_f = np.abs(frames[:, :8] - G[key + "frames64"])[:, keep[:8]].max()
    err_e = (np.abs(e - G[key + "e64"]) / (1 + np.abs(G[key + "e64"])))[keep].max()
    print(f"{key[:-1]}: kept {int(keep.sum())} / {B}, accept counts differ on {int((acc[keep] != G[key + 'acc'][keep]).sum())} kept chains; "
          f"|dx| {err_x:.3g}, frames {err_f:.3g} (bound {bound_x:.3g}); energy {err_e:.3g} (bound {bound_e:.3g})")
    assert acc.dtype == np.int32 and np.array_equal(acc[keep], G[key + "acc"][keep])
    assert err_x <= bound_x and err_f <= bound_x and err_e <= bound_e
    assert np.array_equal(frames[-1], x)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_returned_energies_are_the_energy_kernels_bits(chains, case):
    r = chains(case)
    assert torch.equal(r["e"], r["energy"].energy(r["x"])[:, 0])


@pytest.mark.parametrize("kind,n,d,h", [("mdw", 4, 2, 0.15), ("lj", 53, 3, 0.03)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, kind, n, d, h):
    P = golden("particles")
    torch.manual_seed(1234)
    if (n, d) == (53, 3):
        energy = make_pair(P, kind, n, d).to(dev)
        x0 = torch.tensor(P["x_55_3"], device=dev)[:, :53].reshape(B, -1).contiguous()
    else:
        energy, x_np = make(golden, (kind, n, d))
        energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    settings = (h, 5, 1.0, temps)
    drawn, step_a = fused_sampler(energy, x0, settings, stream=40)
    step_a.set_philox_stream(40, calls=7)                                          # continue the stream at step 7
    seed, offset = step_seed(step_a)
    assert offset == 7
    fa = drawn.sample(N_FRAMES)
    assert step_a._philox_ids()[1] == 7 + N_STEPS                                  # the counter is the index of the next step
    noise, unif = philox_numbers(seed, offset, N_STEPS, B, n * d, dev)
    fed, step_b = fused_sampler(energy, x0, settings, noise, unif)
    fb = fed.sample(N_FRAMES)
    a, b = drawn.state.as_dict(), fed.state.as_dict()
    assert torch.equal(fa, fb) and torch.equal(a["samples"][0], b["samples"][0]) and torch.equal(a["energies"], b["energies"])
    assert torch.equal(step_a.n_accepted, step_b.n_accepted)
    rate = float(step_a.n_accepted.float().mean()) / N_STEPS
    assert 0.1 < rate < 1.0, rate                                                  # (a run that moves and rejects: not frozen chains)
    assert torch.equal(a["energies"], energy.energy(a["samples"][0])[:, 0])


@pytest.mark.parametrize("case", [("lj", 13, 3), ("mdw", 64, 3)], ids=["lj_13_3", "mdw_64_3"])
def test_independence_of_sharding_chunking_and_the_step_cap(hip_lib, dev, golden, monkeypatch, case):
    G, key = golden("hmc"), key_of(case)
    torch.manual_seed(99)
    energy, x_np = make(golden, case)
    energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    h, L, m, _ = case_settings(G, key, torch.float32, dev)
    temps = torch.tensor([1.0, 2.0], device=dev).repeat(B // 2)
    whole, step_w = fused_sampler(energy, x0, (h, L, m, temps), stream=50)
    fw = whole.sample(N_FRAMES)
    xw, ew = whole.state.as_dict()["samples"][0], whole.state.as_dict()["energies"]
    assert 0 < int(step_w.n_accepted.sum()) < B * N_STEPS
    # chains 64..149 alone, told where they sit in the whole
    part, step_p = fused_sampler(energy, x0[64:].contiguous(), (h, L, m, temps[64:].contiguous()), stream=50)
    step_p.chain_offset = 64
    fp = part.sample(N_FRAMES)
    assert torch.equal(fp, fw[:, 64:]) and torch.equal(part.state.as_dict()["energies"], ew[64:])
    assert torch.equal(step_p.n_accepted, step_w.n_accepted[64:])
    # chunked sample calls
    chunked, step_c = fused_sampler(energy, x0, (h, L, m, temps), stream=50)
    fc = torch.cat([chunked.sample(2), chunked.sample(1), chunked.sample(3)])
    assert torch.equal(fc, fw) and torch.equal(chunked.state.as_dict()["energies"], ew) and torch.equal(step_c.n_accepted, step_w.n_accepted)
    # 12 steps in one forward = 6 forwards of 2 steps, accept counts accumulated
    step_1 = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, target_temperatures=temps, n_steps=N_STEPS).set_philox_stream(50)
    step_1.fused = "always"
    one = step_1(bg.SamplerState(samples=x0)).as_dict()
    step_6 = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, target_temperatures=temps, n_steps=STRIDE).set_philox_stream(50)
    step_6.fused = "always"
    state = bg.SamplerState(samples=x0)
    for _ in range(N_FRAMES):
        state = step_6(state)
    for got in (one, state.as_dict()):
        assert got["energies_up_to_date"] and torch.equal(got["samples"][0], xw) and torch.equal(got["energies"], ew)
    assert torch.equal(step_1.n_accepted, step_w.n_accepted) and torch.equal(step_6.n_accepted, step_w.n_accepted)
    # the per-launch cap at 1 step and at 3 steps (a stride of 2: pieces of 1 + 1, launches of 2; a stride of 5: 3 + 2) = the uncapped run
    wide, step_wide = fused_sampler(energy, x0, (h, L, m, temps), stride=5, stream=50)
    f5 = wide.sample(2)
    for cap in (1, 3):
        monkeypatch.setattr(sampling, "hmc_max_steps_per_launch", lambda n_leapfrog: cap)
        for stride, n_frames, want, want_acc in ((STRIDE, N_FRAMES, fw, step_w.n_accepted), (5, 2, f5, step_wide.n_accepted)):
            capped, step_k = fused_sampler(energy, x0, (h, L, m, temps), stride=stride, stream=50)
            assert step_k._launch_cap() == cap
            assert torch.equal(capped.sample(n_frames), want) and torch.equal(step_k.n_accepted, want_acc)


@pytest.mark.parametrize("case,height,h", [(("lj", 64, 3), 16, 0.03), (("rep", 36), 41, 0.01), (("lj", 13, 3), 64, 0.06)],
                         ids=["16_rows", "41_rows", "64_rows"])
def test_a_row_alone_gets_the_bits_it_gets_in_its_batch(hip_lib, dev, golden, case, height, h):
    """rows 0, height - 1, height and B - 1 of a batch of 97: the last row of the first tile, the first of the second, the partial last tile"""
    batch = 97
    energy, x_np = make(golden, case)
    energy, x0 = energy.to(dev), torch.tensor(x_np[:batch], device=dev)
    assert sampling.hmc_tile_rows(x0.shape[1]) == height
    torch.manual_seed(5)
    settings = (h, 5, 1.0, 1.0)
    whole, step_w = fused_sampler(energy, x0, settings, stream=30)
    fw = whole.sample(3)
    ew = whole.state.as_dict()["energies"]
    assert 0 < int(step_w.n_accepted.sum()) < batch * 3 * STRIDE
    for row in (0, height - 1, height, batch - 1):
        alone, step_a = fused_sampler(energy, x0[row:row + 1].contiguous(), settings, stream=30)
        step_a.chain_offset = row
        assert torch.equal(alone.sample(3), fw[:, row:row + 1]), row
        assert torch.equal(alone.state.as_dict()["energies"], ew[row:row + 1]) and torch.equal(step_a.n_accepted, step_w.n_accepted[row:row + 1])


def test_sample_is_one_launch(hip_lib, dev, golden):
    from test_gpu_round6 import _device_kernel_names
    energy, x_np = make(golden, ("lj", 13, 3))
    energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    sampler, step = fused_sampler(energy, x0, (0.06, 5, 1.0, 1.0), stride=3, stream=60)
    assert step._launch_cap() >= 12
    names = _device_kernel_names(lambda: sampler.sample(4))
    print(names)
    assert len(names) == 1 and "pair_hmc_kernel" in names[0], names


def test_a_trajectory_that_blows_up_is_rejected(hip_lib, dev, golden):
    energy, x_np = make(golden, ("lj", 4, 2))
    energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    sampler, step = fused_sampler(energy, x0, (10.0, 5, 1.0, 1.0), stream=61)
    frames = sampler.sample(3)
    state = sampler.state.as_dict()
    assert int(step.n_accepted.sum()) == 0 and step.n_proposed == 3 * STRIDE
    assert torch.equal(state["samples"][0], x0) and torch.equal(frames, x0.expand(3, -1, -1))
    assert torch.isfinite(state["samples"][0]).all() and torch.isfinite(state["energies"]).all()
    assert torch.equal(state["energies"], energy.energy(x0)[:, 0])


def test_coincident_particles_are_rejected(hip_lib, dev, golden):
    """explicit normals that put particle 1 of chain 0 onto particle 0 after the one drift of a MALA step: the proposal's energy is
    huge, never accepted; chain 1 next to it moves"""
    n, d, h, steps = 4, 2, 0.01, 4
    energy, x_np = make(golden, ("lj", n, d))
    energy = energy.to(dev)
    x0 = torch.tensor(x_np, device=dev)[:8].contiguous()
    force = energy.force(x0.clone()).detach()
    noise = torch.tensor(random_numbers(5, n * d, steps, 8)[0], device=dev)
    target = x0.clone()
    target[0, 2:4] = x0[0, 0:2]
    noise[:, 0] = ((target - x0) / h - (h / 2) * force)[0]                     # x + h (xi + (h / 2) f(x)) = target
    unif = torch.full((steps, 8), 1e-30, device=dev)                           # log r = -69: anything but a wall is accepted
    step = bg.HMCStep(energy, h, n_leapfrog=1, n_steps=steps).feed_noise(noise, unif)
    e0 = energy.energy(x0)[:, 0]
    out = step(bg.SamplerState(samples=x0)).as_dict()
    assert int(step.n_accepted[0]) == 0 and torch.equal(out["samples"][0][0], x0[0]) and torch.equal(out["energies"][0], e0[0])
    assert torch.isfinite(out["energies"]).all() and torch.isfinite(out["samples"][0]).all()
    assert (step.n_accepted[1:] == steps).all()                                # the other chains moved
    assert torch.equal(out["energies"], energy.energy(out["samples"][0])[:, 0])
    # NaN normals are rejected, too
    stuck = bg.HMCStep(energy, h, n_leapfrog=1).feed_noise(torch.full((1, 8, n * d), float("nan"), device=dev), unif[:1].contiguous())
    out = stuck(bg.SamplerState(samples=x0)).as_dict()
    assert int(stuck.n_accepted.sum()) == 0 and torch.equal(out["samples"][0], x0)


def test_stationary_distribution_with_in_kernel_philox(hip_lib, dev):
    """mean-free normal of 4 particles in 2 dimensions, std 0.8: the variance of a centred coordinate at temperature T is
    T std^2 (n - 1) / n.  4096 chains at temperatures alternating 1 and 4, 500 burn-in steps, 50 frames 10 steps apart: 3 % -- the setup,
    sample sizes and tolerance of test_gpu_mcmc.py's test.  5 leapfrog steps of 0.8: on the CPU general path in f64 (seed 7) the
    acceptance is 0.77 at T = 1 and 0.97 at T = 4, 0.87 overall, and the variances are +0.18 % and -0.07 % off."""
    torch.manual_seed(7)
    n_chains = 4096
    target = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False).to(dev)
    temps = torch.tensor([1.0, 4.0], device=dev).repeat(n_chains // 2)
    sampler, step = fused_sampler(target, torch.zeros(n_chains, 8, device=dev), (0.8, 5, 1.0, temps), stride=10, n_burnin=50, stream=70)
    assert sampler.i == 50 and step.n_proposed == 500
    frames = sampler.sample(50)
    assert frames.shape == (50, n_chains, 8) and step.n_proposed == 1000
    rate = float(step.n_accepted.double().mean()) / step.n_proposed
    print(f"acceptance {rate:.3f}")
    assert 0.6 <= rate <= 0.95
    x = frames.reshape(50, n_chains, 4, 2)
    x = x - x.mean(dim=2, keepdim=True)
    for k, temp in enumerate((1.0, 4.0)):
        var = float(x[:, k::2].double().pow(2).mean())
        want = temp * 0.64 * 3 / 4
        print(f"T = {temp}: variance {var:.5f}, expected {want:.5f} ({var / want - 1:+.2%})")
        assert abs(var / want - 1) <= 0.03


def test_fallbacks_agree_with_the_fused_path(hip_lib, dev, golden):
    """f64 samples, a strided view, a tensor-valued step size and a temperature mismatch run the general path on the same fed numbers:
    the fused path's accept counts on the kept chains, positions to the parity bound; 65 particles are outside the envelope"""
    G, case = golden("hmc"), ("mdw", 4, 2)
    key = key_of(case)
    energy, x_np = make(golden, case)
    energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    noise_np, unif_np = case_numbers(golden, case, x_np.shape[1])
    noise, unif = torch.tensor(noise_np, device=dev), torch.tensor(unif_np, device=dev)
    h, L, m, _ = case_settings(G, key, torch.float32, dev)
    keep, rows = G[key + "keep"], G[key + "rows"]
    bound_x = 4 * float(G[key + "err_x32"]) + 1e-6
    fused, step_f = fused_sampler(energy, x0, (h, L, m, 1.0), noise, unif)
    fused.sample(N_FRAMES)
    acc_f = step_f.n_accepted.cpu().numpy()
    assert np.array_equal(acc_f[keep], G[key + "acc"][keep])

    def general(name, x_start, step):
        """one forward of all 12 steps on the general path (a state the general path hands on may itself be fusable)"""
        state = bg.SamplerState(samples=x_start)
        assert step._fused_setup(state) is None and step._n_steps == N_STEPS, name
        with recorded_normals(noise) as drawn, recorded_uniforms(unif) as count:
            out = step(state).as_dict()
        assert count[0] == N_STEPS and drawn[0] == N_STEPS and step.n_proposed == N_STEPS, name
        x = out["samples"][0]
        assert x.shape == x_start.shape and x.dtype == x_start.dtype and out["energies_up_to_date"], name
        assert np.array_equal(step.n_accepted.cpu().numpy()[keep], acc_f[keep]), name
        err = np.abs(x.cpu().numpy().astype(np.float64)[rows] - G[key + "x64"])[keep[rows]].max()
        print(f"{name}: |dx| {err:.3g} (bound {bound_x:.3g})")
        assert err <= bound_x, name

    general("f64 samples", x0.double(), bg.HMCStep(energy, h, n_leapfrog=L, mass=m, n_steps=N_STEPS))
    wide = torch.zeros(B, 2 * x0.shape[1], device=dev)
    wide[:, ::2] = x0
    assert not wide[:, ::2].is_contiguous()
    general("a strided view", wide[:, ::2], bg.HMCStep(energy, h, n_leapfrog=L, mass=m, n_steps=N_STEPS))
    general("a tensor-valued step size", x0, bg.HMCStep(energy, torch.tensor(h, device=dev), n_leapfrog=L, mass=m, n_steps=N_STEPS))
    ones = torch.ones(B, device=dev)
    general("a temperature mismatch", x0, bg.MCMCStep(energy, proposal=bg.HamiltonianProposal(energy, h, n_leapfrog=L, mass=m, temperature=1.0),
                                                      target_temperatures=ones, n_steps=N_STEPS))
    off = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, n_steps=N_STEPS)
    off.fused = False
    general("fused = False", x0, off)
    # the fused path never calls torch.rand_like
    plain = bg.HMCStep(energy, h, n_leapfrog=L, mass=m, n_steps=3)
    with recorded_uniforms(unif) as count:
        plain(bg.SamplerState(samples=x0))
    assert count[0] == 0 and plain.n_proposed == 3
    # 65 particles: outside the kernel's envelope
    big = bg.LennardJonesPotential(65 * 3, 65, two_event_dims=False).to(dev)
    xb = 1.2 * torch.stack(torch.meshgrid(*[torch.arange(5.0, device=dev)] * 3, indexing="ij"), -1).reshape(-1, 3)[:65].reshape(1, -1).repeat(6, 1)
    step = bg.HMCStep(big, 0.001, n_leapfrog=2, n_steps=2)
    assert _kernel_plan(big, 1.0) is None and step._fused_setup(bg.SamplerState(samples=xb)) is None
    out = step(bg.SamplerState(samples=xb)).as_dict()
    assert out["samples"][0].shape == (6, 195) and torch.isfinite(out["energies"]).all() and step.n_proposed == 2
    # the shortcut class is fused, and not with a box constraint
    assert bg.HamiltonianMCSampler(energy, x0, step_size=h)._fused_setup() is not None
    assert bg.HamiltonianMCSampler(energy, x0, step_size=h, box_constraint=lambda t: t.clamp(-6.0, 6.0))._fused_setup() is None


def test_burn_in_progress_bar_three_dimensional_samples_and_carried_energies(hip_lib, dev, golden, monkeypatch):
    """what the fused path keeps of ``MCMCStep``'s: burn-in, the progress bar per iteration, samples [B, n, d], carried energies"""
    P = golden("particles")
    n, d = 13, 3
    torch.manual_seed(5)
    two, flat = make_pair(P, "lj", n, d, two_event_dims=True).to(dev), make_pair(P, "lj", n, d).to(dev)
    x3 = torch.tensor(P[f"x_{n}_{d}"], device=dev)
    settings = (0.06, 5, 1.0, 2.0)
    seen = []

    def bar(it):
        seen.append([len(it), 0])
        for v in it:
            seen[-1][1] += 1
            yield v

    monkeypatch.setattr(sampling, "hmc_max_steps_per_launch", lambda n_leapfrog: 3)
    s3, st3 = fused_sampler(two, x3, settings, stream=80, n_burnin=2, progress_bar=bar)
    s2, st2 = fused_sampler(flat, x3.reshape(B, -1), settings, stream=80, n_burnin=2)
    f3, f2 = s3.sample(4), s2.sample(4)
    assert seen == [[2, 2], [4, 4]] and s3.i == 6 and st3.n_proposed == 6 * STRIDE
    assert f3.shape == (4, B, n, d) and torch.equal(f3.reshape(4, B, -1), f2)
    assert s3.state.as_dict()["samples"][0].shape == (B, n, d)
    assert st3.state_dict()["_philox_state"].tolist() == [80, 6 * STRIDE]
    # carried energies: a state whose (wrong) energies are marked up to date starts from them -- at +1e4 every first proposal is accepted
    step = bg.HMCStep(flat, 0.01, n_leapfrog=5).set_philox_stream(82)      # a step size at which the change of the kinetic energy is small
    lifted = bg.SamplerState(samples=x3.reshape(B, -1)).replace(energies=torch.full((B,), 1e4, device=dev))
    out = step(lifted).as_dict()
    assert int(step.n_accepted.sum()) == B and torch.equal(out["energies"], flat.energy(out["samples"][0])[:, 0])


def test_the_default_takes_the_kernel_where_it_was_measured_faster(hip_lib, dev, golden):
    """``fused = True``: pair targets whose tile is a full wave; elsewhere -- shorter tiles, the box -- the general path runs unless
    ``fused = "always"``"""
    for case, default in ((("lj", 13, 3), True), (("mdw", 4, 2), True), (("lj", 64, 3), False), (("rep", 36), False), (("harm", 2), False)):
        energy, x_np = make(golden, case)
        energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
        plan = _kernel_plan(energy, 1.0)
        assert sampling.hmc_fused_by_default(plan) == default, case
        state = bg.SamplerState(samples=x0)
        step = bg.HMCStep(energy, 0.01, n_leapfrog=2)
        assert step.fused is True and (step._fused_setup(state) is not None) == default, case
        step.fused = "always"
        assert step._fused_setup(state) is not None, case
        step.fused = False
        assert step._fused_setup(state) is None, case
        assert (bg.HamiltonianMCSampler(energy, x0)._fused_setup() is not None) == default, case
    # the default on a box target runs the general path: torch.rand_like is called once per step
    energy, x_np = make(golden, ("rep", 2))
    energy, x0 = energy.to(dev), torch.tensor(x_np, device=dev)
    unif = torch.tensor(random_numbers(5, 8, 3, B)[1], device=dev)
    step = bg.HMCStep(energy, 0.01, n_leapfrog=2, n_steps=3)
    with recorded_uniforms(unif) as count:
        out = step(bg.SamplerState(samples=x0)).as_dict()
    assert count[0] == 3 and step.n_proposed == 3 and torch.isfinite(out["energies"]).all()
    # a Gaussian proposal is not concerned
    assert bg.MCMCStep(energy, proposal=bg.GaussianProposal(0.05))._fused_setup(bg.SamplerState(samples=x0)) is not None
