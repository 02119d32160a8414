"""GPU (-m gpu): replica exchange inside the chain kernel -- ``ReplicaExchangeMCMCStep`` / ``IterativeSampler`` on bgk_pair_remc /
bgk_box_remc (csrc/bgk_mcmc.hip) -- against the reference's recorded f64 ladders (tests/golden/remc.npz, written by
tests/golden/make_remc_goldens.py), bitwise against launches of the plain kernel with the rule in torch ops between them, and bitwise
against itself: in-kernel Philox = the same numbers handed in, split / sharded runs = the run in one piece, ``sample(n)`` = repeated
``forward``.

Bounds of the parity test, on the ladders the fixture keeps (every f64 Metropolis and exchange margin >= 1e-3): counts equal;
|x - x64| <= 4 err_x32 + 1e-6 and |e - e64| / (1 + |e64|) <= 4 err_e32 + 1e-6, err_* the errors of the reference's own f32 run -- the
bound of test_gpu_mcmc.py."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd.distributions import _kernel_plan, philox_sample

import box_common
import remc_common as C
from mcmc_common import make
from test_gpu_mcmc import step_seed
from test_host_remc import start_states

pytestmark = pytest.mark.gpu


def remc_step(energy, temps, std, n_steps=1, every=1, numbers=None, stream=None):
    step = bg.ReplicaExchangeMCMCStep(energy, temps, proposal=bg.GaussianProposal(noise_std=std), n_steps=n_steps, exchange_every=every)
    if numbers is not None:
        step.feed_noise(*numbers)
    if stream is not None:
        step.set_philox_stream(stream)
    return step


def fused_sampler(step, x0, stride=1, **kwargs):
    sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=stride, **kwargs)
    assert sampler._fused_setup() is not None, "the case must take the fused path"
    return sampler


# ---- 1. parity with the reference's ladders
@pytest.mark.parametrize("case", list(C.CASES))
def test_parity_on_recorded_numbers(hip_lib, dev, golden, case):
    G, P = golden("remc"), golden("particles")
    kind, n, d, std, temps = C.CASES[case]
    key = case + "_"
    keep, rows = G[key + "keep"], G[key + "rows"]
    assert keep.mean() >= 2 / 3
    kc = np.repeat(keep, C.K)
    numbers = tuple(torch.tensor(a, device=dev) for a in C.recorded_numbers(n * d))
    energy = make(P, kind, n, d).to(dev)
    x0 = torch.tensor(start_states(P, n, d), device=dev)
    # frames: sample(10) of a stride of one epoch, written by the kernel before each exchange
    step = remc_step(energy, temps, std, every=C.EVERY, numbers=numbers)
    frames = fused_sampler(step, x0, stride=C.EVERY).sample(C.N_EXCHANGES).cpu().numpy().astype(np.float64)
    # final state: one forward of 30 steps and the exchange that is due after the last
    whole = remc_step(energy, temps, std, n_steps=C.N_STEPS, every=C.EVERY, numbers=numbers)
    state = whole.apply_pending_exchange(whole(bg.SamplerState(samples=x0))).as_dict()
    assert whole.steps_done == C.N_STEPS and whole.n_exchange_attempts == C.N_EXCHANGES and state["energies_up_to_date"]
    for s in (step, whole):
        assert np.array_equal(s.n_accepted.cpu().numpy()[kc], G[key + "acc"][kc])
        assert np.array_equal(s.n_exchanged.cpu().numpy()[kc], G[key + "exch"][kc])
    x, e, e64 = state["samples"][0].cpu().numpy().astype(np.float64), state["energies"].cpu().numpy().astype(np.float64), G[key + "e64"]
    bound_x, bound_e = 4 * float(G[key + "err_x32"]) + 1e-6, 4 * float(G[key + "err_e32"]) + 1e-6
    fr = C.FRAME_LADDERS * C.K
    err_x = np.abs(x[rows] - G[key + "x64"])[kc[rows]].max()
    err_f = np.abs(frames[:, :fr] - G[key + "frames64"])[:, kc[:fr]].max()
    err_e = (np.abs(e - e64) / (1 + np.abs(e64)))[kc].max()
    print(f"{case}: kept {int(keep.sum())} / {C.L} ladders; |dx| {err_x:.3g}, frames {err_f:.3g} (bound {bound_x:.3g}); energy {err_e:.3g} (bound {bound_e:.3g})")
    assert err_x <= bound_x and err_f <= bound_x and err_e <= bound_e
    assert torch.equal(state["energies"], energy.energy(state["samples"][0])[:, 0])


# ---- 2. bitwise against the plain kernel
def shape_case(name, golden, dev):
    """(energy, x0 [B, n d], noise_std) of a shape of the table; B = L K rows of the stored start states (repeated beyond their 150)"""
    P = golden("particles")
    if name == "box":
        G = golden("box")
        return box_common.make(G, "rep", 36).to(dev), torch.tensor(G["x_36"], device=dev), float(G["mc_rep_36_std"])
    if name == "lj53":          # n d = 159, the widest row bgk_philox_fields writes; a tile of 49 rows, 45 with ladders of 5
        return make(P, "lj", 53, 3).to(dev), torch.tensor(P["x_55_3"], device=dev)[:, :53].reshape(150, -1).contiguous(), 0.02
    kind, n, d, std = {"mdw": ("mdw", 4, 2, 0.3), "lj": ("lj", 64, 3, 0.02), "mfn": ("mfn", 13, 3, 0.2)}[name]
    return make(P, kind, n, d).to(dev), torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(150, -1), std


def ladder(K):
    return torch.tensor(np.geomspace(1.0, 2.5, K), dtype=torch.float32)


def emulate(plan, x0, temps, std, noise, unif, exch, K, every, n_steps):
    """the exchange launch made of launches of the plain kernel, one per epoch, and the rule in f32 torch ops between them (1 / T on the
    host: a correctly rounded division).  Also per ladder: every margin |-log r - c|, in f64 from these f32 energies, >= 1e-5 (1 + |c|)"""
    B, dev = x0.shape[0], x0.device
    x, e = x0.clone(), torch.empty(B, device=dev)
    acc, nex = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    walkers = torch.arange(K, dtype=torch.int32, device=dev).repeat(B // K)
    beta = (1.0 / temps.cpu()).to(dev)
    clear = torch.ones(B // K, dtype=torch.bool, device=dev)
    done = j = parity = 0
    while done < n_steps:
        k = min(every - done % every, n_steps - done)
        sampling.pair_mcmc(plan, x, e, done > 0, temps, std, k, noise[done:done + k].contiguous(), unif[done:done + k].contiguous(),
                           n_accepted=acc, accumulate=done > 0)
        done += k
        if done % every == 0:
            lower = (torch.arange(0, B, K, device=dev)[:, None] + torch.arange(parity, K - 1, 2, device=dev)[None, :]).reshape(-1)
            upper = lower + 1
            c = -(e[upper] - e[lower]) * (beta[upper] - beta[lower])
            swap = -torch.log(exch[j][lower]) > c
            c64 = -(e[upper].double() - e[lower].double()) * (beta[upper].double() - beta[lower].double())
            tight = (-torch.log(exch[j][lower].double()) - c64).abs() < 1e-5 * (1 + c64.abs())
            clear[(lower // K)[tight]] = False
            perm = torch.arange(B, device=dev)
            perm[lower], perm[upper] = torch.where(swap, upper, lower), torch.where(swap, lower, upper)
            x, e, walkers = x[perm].contiguous(), e[perm].contiguous(), walkers[perm]
            nex[lower] += swap.to(torch.int32)
            parity ^= 1
            j += 1
    return x, e, acc, nex, walkers, clear


@pytest.mark.parametrize("every,n_steps", [(1, 5), (3, 8)])
@pytest.mark.parametrize("name,K,L", [("mdw", 5, 27), ("lj", 5, 27), ("lj", 41, 3), ("mdw", 64, 3), ("mfn", 2, 40), ("box", 3, 30)])
def test_one_launch_equals_plain_launches_with_the_rule_between(hip_lib, dev, golden, name, K, L, every, n_steps):
    energy, start, std = shape_case(name, golden, dev)
    B, nd = K * L, start.shape[1]
    x0 = start[torch.arange(B, device=dev) % start.shape[0]].contiguous()
    temps = ladder(K).to(dev).repeat(L)
    plan = _kernel_plan(energy, 1.0)
    noise, unif, exch = (torch.tensor(a, device=dev) for a in C.recorded_numbers(nd, C.SEED + K, n_steps, B, 1, every))
    assert exch.shape == (n_steps // every, B)
    want_x, want_e, want_acc, want_nex, want_w, clear = emulate(plan, x0, temps, std, noise, unif, exch, K, every, n_steps)
    x, e = x0.clone(), torch.empty(B, device=dev)
    acc, nex = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    walkers = torch.arange(K, dtype=torch.int32, device=dev).repeat(L)
    sampling.pair_mcmc(plan, x, e, False, temps, std, n_steps, noise, unif, n_accepted=acc, n_replicas=K, exchange_every=every,
                       exchange_uniforms=exch, n_exchanged=nex, walkers=walkers)
    assert float(clear.float().mean()) >= 0.9
    rows = clear.repeat_interleave(K)
    pairs = sum(len(range(j & 1, K - 1, 2)) for j in range(n_steps // every)) * L
    print(f"{name} K={K} L={L} every={every}: {int(clear.sum())} / {L} ladders compared, {int(want_nex.sum())} of {pairs} exchanges, "
          f"acceptance {float(want_acc.float().mean()) / n_steps:.2f}")
    assert torch.equal(x[rows], want_x[rows]) and torch.equal(e[rows], want_e[rows])
    assert torch.equal(acc[rows], want_acc[rows]) and torch.equal(nex[rows], want_nex[rows]) and torch.equal(walkers[rows], want_w[rows])
    assert 0 < int(want_nex.sum()) <= pairs and not torch.equal(want_w, torch.arange(K, dtype=torch.int32, device=dev).repeat(L))
    assert torch.equal(e, energy.energy(x)[:, 0])


def test_kernel_hand_cases_equal_temperatures_and_nan(hip_lib, dev, golden):
    """one step with noise_std = 0 from handed energies, K = 4, equal temperatures: c = 0 < -log r, so every pair (0,1), (2,3) exchanges
    -- but for the pair with a NaN energy (c is NaN: the comparison is false), whichever side holds it"""
    energy, start, _ = shape_case("mdw", golden, dev)
    K, L = 4, 3
    B = K * L
    x0 = start[:B].contiguous()
    plan = _kernel_plan(energy, 1.0)
    e0 = energy.energy(x0)[:, 0].contiguous()
    e0[0], e0[7] = float("nan"), float("nan")                  # ladder 0: the lower slot of (0,1); ladder 1: the upper slot of (2,3)
    x, e = x0.clone(), e0.clone()
    nex = torch.empty(B, dtype=torch.int32, device=dev)
    walkers = torch.arange(K, dtype=torch.int32, device=dev).repeat(L)
    sampling.pair_mcmc(plan, x, e, True, torch.ones(B, device=dev), 0.0, 1, seed=5, n_replicas=K, exchange_every=1, n_exchanged=nex,
                       walkers=walkers)
    assert walkers.tolist() == [0, 1, 3, 2, 1, 0, 2, 3, 1, 0, 3, 2] and nex.tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0]
    perm = torch.tensor([0, 1, 3, 2, 5, 4, 6, 7, 9, 8, 11, 10], device=dev)
    assert torch.equal(x, x0[perm]) and torch.equal(e.isnan(), e0[perm].isnan()) and torch.equal(e[~e.isnan()], e0[perm][~e.isnan()])
    # the next parity: (1,2) alone
    sampling.pair_mcmc(plan, x, e, True, torch.ones(B, device=dev), 0.0, 1, seed=5, offset=1, n_replicas=K, exchange_every=1,
                       exchange_parity=1, n_exchanged=nex, walkers=walkers)
    assert walkers.tolist() == [0, 3, 1, 2, 1, 2, 0, 3, 1, 3, 0, 2] and nex.tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0]


def test_fused_envelope_on_the_device(hip_lib, dev, golden):
    energy, start, std = shape_case("lj", golden, dev)
    for K, fused in ((41, True), (43, False)):
        step = remc_step(energy, torch.linspace(1.0, 2.0, K), std)
        setup = step._fused_setup(bg.SamplerState(samples=start[:2 * K].contiguous()))
        assert (setup is not None) is fused
    with pytest.raises(ValueError, match="whole number of ladders"):
        remc_step(energy, [1.0, 2.0, 3.0], std)._fused_setup(bg.SamplerState(samples=start[:10].contiguous()))
    step = remc_step(energy, [1.0, 2.0, 3.0], std)
    step.chain_offset = 4
    with pytest.raises(ValueError, match="chain_offset"):
        step(bg.SamplerState(samples=start[:9].contiguous()))
    # beyond the tile height the general path runs, without an error
    out = remc_step(energy, torch.linspace(1.0, 2.0, 43), std, n_steps=2)(bg.SamplerState(samples=start[:86].contiguous())).as_dict()
    assert out["samples"][0].shape == (86, 192) and torch.isfinite(out["energies"]).all()


# ---- 3. in-kernel Philox
def philox_numbers(seed, offset, n_steps, batch, nd, dev, every, steps_done=0):
    """what bgk_philox_fields writes for (seed, offset + s), fields [normal nd, uniform 1, uniform 1]; the third at the exchange steps"""
    noise, unif, exch = [], [], []
    for s in range(n_steps):
        (eps, r, rx), _ = philox_sample([(1, nd, None, None, 1.0, 0.0), (0, 1, None, None, 1.0, 0.0), (0, 1, None, None, 1.0, 0.0)], batch, dev,
                                        seed, offset + s)
        noise.append(eps)
        unif.append(r[:, 0])
        if (steps_done + s + 1) % every == 0:
            exch.append(rx[:, 0])
    return torch.stack(noise), torch.stack(unif), torch.stack(exch)


@pytest.mark.parametrize("name,K,L", [("mdw", 5, 27), ("lj53", 5, 27)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, name, K, L):
    torch.manual_seed(1234)
    energy, start, std = shape_case(name, golden, dev)
    x0 = start[:K * L].contiguous()
    every, stride, n = 3, 2, 6                                                       # 12 steps: exchanges after steps 3, 6, 9, 12
    step_a = remc_step(energy, ladder(K), std, every=every, stream=41)
    step_a.set_philox_stream(41, calls=7)
    seed, offset = step_seed(step_a)
    assert offset == 7
    drawn = fused_sampler(step_a, x0, stride=stride)
    fa = drawn.sample(n)
    assert step_a._philox_ids()[1] == 7 + stride * n
    step_b = remc_step(energy, ladder(K), std, every=every, numbers=philox_numbers(seed, offset, stride * n, K * L, x0.shape[1], dev, every))
    fed = fused_sampler(step_b, x0, stride=stride)
    fb = fed.sample(n)
    a, b = drawn.state.as_dict(), fed.state.as_dict()
    assert torch.equal(fa, fb) and torch.equal(a["samples"][0], b["samples"][0]) and torch.equal(a["energies"], b["energies"])
    assert torch.equal(step_a.n_accepted, step_b.n_accepted) and torch.equal(step_a.n_exchanged, step_b.n_exchanged)
    assert torch.equal(step_a.walkers, step_b.walkers) and step_a.n_exchange_attempts == step_b.n_exchange_attempts == 4
    assert 0 < int(step_a.n_exchanged.sum()) < 4 * L * (K // 2)


# ---- 4. split and sharding
def test_independence_of_the_step_cap_and_of_sharding(hip_lib, dev, golden, monkeypatch):
    torch.manual_seed(99)
    energy, start, std = shape_case("lj", golden, dev)
    K, L, L1 = 5, 27, 5                                                             # tiles of 40 rows: the shard boundary is inside the first
    x0 = start[:K * L].contiguous()

    def run(x, every, stride, n, offset=0):
        step = remc_step(energy, ladder(K), std, every=every, stream=51)
        step.chain_offset = offset
        frames = fused_sampler(step, x, stride=stride).sample(n)
        return frames, step

    for every, stride, n in ((1, 3, 6), (4, 9, 3)):
        whole, step_w = run(x0, every, stride, n)
        first, step_1 = run(x0[:L1 * K].contiguous(), every, stride, n)
        rest, step_2 = run(x0[L1 * K:].contiguous(), every, stride, n, offset=L1 * K)
        assert torch.equal(torch.cat([first, rest], dim=1), whole)
        for name in ("n_accepted", "n_exchanged", "walkers"):
            assert torch.equal(torch.cat([getattr(step_1, name), getattr(step_2, name)]), getattr(step_w, name)), name
        monkeypatch.setattr(sampling, "MCMC_MAX_STEPS_PER_LAUNCH", 7)
        capped, step_c = run(x0, every, stride, n)
        monkeypatch.undo()
        assert torch.equal(capped, whole) and step_c.steps_done == step_w.steps_done == stride * n
        for name in ("n_accepted", "n_exchanged", "walkers"):
            assert torch.equal(getattr(step_c, name), getattr(step_w, name)), name
        assert step_c.n_exchange_attempts == step_w.n_exchange_attempts == stride * n // every and int(step_w.n_exchanged.sum()) > 0


# ---- 5. the sampler's in-kernel recording
@pytest.mark.parametrize("every", [1, 2, 3])
def test_sample_equals_repeated_forward(hip_lib, dev, golden, every):
    torch.manual_seed(3)
    energy, start, std = shape_case("mdw", golden, dev)
    K, L, n = 5, 27, 5
    x0 = start[:K * L].contiguous()
    keep = x0.clone()
    step_s = remc_step(energy, ladder(K), std, n_steps=2, every=every, stream=61)
    sampler = fused_sampler(step_s, x0)
    frames = sampler.sample(n)
    step_f = remc_step(energy, ladder(K), std, n_steps=2, every=every, stream=61)
    state, states = bg.SamplerState(samples=x0), []
    for _ in range(n):
        state = step_f(state)
        states.append(state.as_dict())
    assert torch.equal(x0, keep), "the caller's start tensor is not touched"
    assert torch.equal(frames, torch.stack([s["samples"][0] for s in states]))
    final = sampler.state.as_dict()
    assert torch.equal(frames[-1], final["samples"][0]) and final["energies_up_to_date"]
    assert torch.equal(final["energies"], states[-1]["energies"])
    for s in states:
        assert torch.equal(s["energies"], energy.energy(s["samples"][0])[:, 0])
    for step in (step_s, step_f):
        assert step.steps_done == 2 * n and step.n_exchange_attempts == 2 * n // every
        w = step.walkers.reshape(L, K).sort(dim=1).values
        assert torch.equal(w, torch.arange(K, dtype=torch.int32, device=dev).repeat(L, 1))
    assert torch.equal(step_s.walkers, step_f.walkers) and torch.equal(step_s.n_exchanged, step_f.n_exchanged)
    assert not torch.equal(step_s.walkers, torch.arange(K, dtype=torch.int32, device=dev).repeat(L))
    # the exchange due after the last step is in the working chains of the state handed out, by the sampler as by ``forward``:
    # ``apply_pending_exchange`` returns those chains and leaves the counters and ``walkers``, which already have it, as they are
    if (2 * n) % every == 0:
        before = [(s.n_exchange_attempts, s.n_exchanged.clone(), s.walkers.clone()) for s in (step_s, step_f)]
        after = step_f.apply_pending_exchange(state).as_dict()
        after_s = step_s.apply_pending_exchange(sampler.state).as_dict()
        for s, (attempts, nex, w) in zip((step_s, step_f), before):
            assert s.n_exchange_attempts == attempts == 2 * n // every and torch.equal(s.n_exchanged, nex) and torch.equal(s.walkers, w)
        assert torch.equal(after_s["samples"][0], after["samples"][0]) and torch.equal(after_s["energies"], after["energies"])
        assert torch.equal(step_s.walkers, step_f.walkers) and torch.equal(step_s.n_exchanged, step_f.n_exchanged)
        assert torch.equal(after["energies"], energy.energy(after["samples"][0])[:, 0])
        assert torch.equal(after["energies"].reshape(L, K).sort(dim=1).values, states[-1]["energies"].reshape(L, K).sort(dim=1).values)
        assert not torch.equal(after["samples"][0], states[-1]["samples"][0])
        # ... and both go on from there alike: the sampler from its own chains, ``forward`` from the exchanged state
        more = sampler.sample(1)
        assert torch.equal(more[0], step_f(bg.SamplerState(samples=after["samples"][0])).as_dict()["samples"][0])
        assert step_s.n_exchange_attempts == step_f.n_exchange_attempts and torch.equal(step_s.walkers, step_f.walkers)


def test_a_state_from_elsewhere_gets_the_due_exchange_once(hip_lib, dev, golden):
    """a fused ``forward`` that ends with an exchange, then a state that is NOT the one handed out: the kernel's exchange leaves
    ``walkers`` and the counters again and the exchange is made in torch ops on that state -- here with every draw tiny, so that every
    pair (0,1), (2,3) exchanges and the result is known"""
    torch.manual_seed(4)
    energy, start, std = shape_case("mdw", golden, dev)
    K, L = 5, 27
    x0 = start[:K * L].contiguous()
    step = remc_step(energy, ladder(K), std, n_steps=3, every=1, stream=62)
    out = step(bg.SamplerState(samples=x0))
    assert step.n_exchange_attempts == 3 and step._exchange_due()
    w_before, n_before = step._handed.walkers.clone(), step._handed.n_exchanged.clone()      # as they were after two exchanges
    assert not torch.equal(w_before, step.walkers)
    other = bg.SamplerState(samples=out.as_dict()["samples"][0].clone())
    original = torch.rand_like
    torch.rand_like = lambda like: torch.full_like(like, 1e-30)
    try:
        after = step.apply_pending_exchange(other).as_dict()
    finally:
        torch.rand_like = original
    swap = torch.tensor([1, 0, 3, 2, 4], device=dev)
    perm = (torch.arange(0, K * L, K, device=dev)[:, None] + swap[None, :]).reshape(-1)
    lower = torch.tensor([1, 0, 1, 0, 0], dtype=torch.int32, device=dev).repeat(L)
    assert step.n_exchange_attempts == 3 and not step._exchange_due() and step._handed is None
    assert torch.equal(step.walkers, w_before[perm]) and torch.equal(step.n_exchanged, n_before + lower)
    assert torch.equal(after["samples"][0], out.as_dict()["samples"][0][perm])
    assert step.apply_pending_exchange(other) is other                              # nothing is due any more
    # the general path on the device after a fused run: the same bookkeeping
    step2 = remc_step(energy, ladder(K), std, n_steps=3, every=1, stream=63)
    out2 = step2(bg.SamplerState(samples=x0))
    step2.fused = False
    step2(out2)
    assert step2.steps_done == 6 and step2.n_exchange_attempts == 5 and step2._exchange_due()     # 3 in the kernel, then after steps 4 and 5


# ---- 6. stationarity
def test_stationary_distribution_of_every_slot(hip_lib, dev):
    """Mean-free normal of n = 4 particles in d = 2 dimensions, std 0.8, temperatures (1, 2, 4), L = 2048 ladders started from exact
    samples of each slot's distribution: parallel tempering leaves every slot's distribution invariant.  Per sample the sum of the centred
    coordinates' squares over (n - 1) d = 6 is std^2 T chi^2_6 / 6, so the mean over L independent ladders has the relative standard
    deviation sqrt(2 / (6 L)) = 1.28 %; the bound is 5 of them, 6.4 %.  (A sign error in the rule drives the low energies to the hot slots:
    the cold slot heats far beyond that.)"""
    torch.manual_seed(11)
    n, d, std, L, temps = 4, 2, 0.8, 2048, (1.0, 2.0, 4.0)
    K = len(temps)
    target = bg.MeanFreeNormalDistribution(n * d, n, std=std, two_event_dims=False).to(dev)
    z = torch.randn(L, K, n, d, device=dev) * std * torch.tensor(temps, device=dev).sqrt()[None, :, None, None]
    x0 = (z - z.mean(dim=2, keepdim=True)).reshape(L * K, n * d).contiguous()
    step = remc_step(target, temps, 0.4, n_steps=30, every=1, stream=71)
    assert step._fused_setup(bg.SamplerState(samples=x0)) is not None
    x = step(bg.SamplerState(samples=x0)).as_dict()["samples"][0].reshape(L, K, n, d).double()
    x = x - x.mean(dim=2, keepdim=True)
    bound = 5 * (2 / (L * (n - 1) * d)) ** 0.5
    for k, temp in enumerate(temps):
        var = float(x[:, k].pow(2).sum(dim=(1, 2)).mean()) / ((n - 1) * d)
        want = std * std * temp
        print(f"T = {temp}: variance {var:.5f}, expected {want:.5f} ({var / want - 1:+.2%}, bound {bound:.2%})")
        assert abs(var / want - 1) <= bound
    pairs = sum(len(range(j & 1, K - 1, 2)) for j in range(30)) * L
    rate = int(step.n_exchanged.sum()) / pairs
    print(f"exchange rate {rate:.2f}, acceptance {float(step.n_accepted.float().mean()) / 30:.2f}")
    assert 0.10 <= rate <= 0.90
