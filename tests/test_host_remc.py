"""Host: replica exchange -- the numpy class ``ReplicaExchangeMetropolisGauss`` against the reference's seeded run, the general path of
``ReplicaExchangeMCMCStep`` (torch ops) against the reference's f64 ladders on recorded numbers (tests/golden/remc.npz, written by
tests/golden/make_remc_goldens.py), the rule's hand cases, the schedule, the signatures and the argument checks of the new entries."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import sampling
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols

import remc_common as C
from mcmc_common import RecordedProposal, make, recorded_uniforms


def start_states(P, n, d):
    """x_{n}_{d}[0:L] of particles.npz, each tiled K times: [B, n d], ladder-major"""
    return np.repeat(P[f"x_{n}_{d}"].reshape(-1, n * d)[:C.L], C.K, axis=0)


def general_rows(unif, exch, every=C.EVERY):
    """the rows ``torch.rand_like`` hands out on the general path: the acceptance draw of every step and, before the step that follows
    an epoch's last (or at ``apply_pending_exchange``), the exchange's"""
    rows = []
    for s in range(unif.shape[0]):
        rows.append(unif[s])
        if (s + 1) % every == 0:
            rows.append(exch[(s + 1) // every - 1])
    return torch.stack(rows)


def run_general(energy, x0, noise, unif, exch, std, temps):
    """the general path on recorded numbers: (frames [N_EXCHANGES, B, n d], final state after the last exchange, step)"""
    step = bg.ReplicaExchangeMCMCStep(energy, temps, proposal=RecordedProposal(noise, std), exchange_every=C.EVERY)
    with recorded_uniforms(general_rows(unif, exch)) as count:
        sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step], stride=C.EVERY)
        frames = sampler.sample(C.N_EXCHANGES)
        assert count[0] == C.N_STEPS + C.N_EXCHANGES - 1 and step.n_exchange_attempts == C.N_EXCHANGES - 1
        final = step.apply_pending_exchange(sampler.state)
        assert step.apply_pending_exchange(final) is final
    assert count[0] == C.N_STEPS + C.N_EXCHANGES and step.steps_done == C.N_STEPS and step.n_exchange_attempts == C.N_EXCHANGES
    return frames, final, step


def test_numpy_class_reproduces_the_seeded_reference_run(golden):
    G = golden("remc")
    np.random.seed(C.A_SEED)
    re = bg.ReplicaExchangeMetropolisGauss(C.double_well, C.A_X0, C.A_TEMPS, noise=C.A_NOISE, burnin=C.A_BURNIN, stride=C.A_STRIDE)
    re.run(nepochs=C.A_EPOCHS, nsteps_per_epoch=C.A_STEPS)
    traj, etraj = np.array(re.sampler.traj_), np.array(re.sampler.etraj_)
    assert traj.shape == G["a_traj"].shape and np.abs(traj - G["a_traj"]).max() <= 1e-12 and np.abs(etraj - G["a_etraj"]).max() <= 1e-12
    assert re.toggle == int(G["a_toggle"])
    assert len(re.trajs) == 5 and re.trajs[0].dtype == np.float32 and re.trajs[0].shape == (traj.shape[0], 2) and len(re.etrajs) == 5
    assert isinstance(re.sampler, bg.MetropolisGauss) and re.sampler.nwalkers == 5
    with pytest.raises(ValueError, match="odd number of temperatures"):
        bg.ReplicaExchangeMetropolisGauss(C.double_well, C.A_X0, np.array([1.0, 2.0, 3.0, 4.0]))


@pytest.mark.parametrize("case", list(C.CASES))
def test_general_path_reproduces_the_reference_ladders(golden, case):
    """f64 on the CPU, the fixture's random numbers: the same decisions, and states to 1e-12, on EVERY ladder"""
    G, P = golden("remc"), golden("particles")
    kind, n, d, std, temps = C.CASES[case]
    key = case + "_"
    assert float(G[key + "std"]) == std and tuple(G[key + "temps"]) == temps
    noise, unif, exch = (torch.from_numpy(a) for a in C.recorded_numbers(n * d))
    energy = make(P, kind, n, d)
    frames, final, step = run_general(energy, torch.tensor(start_states(P, n, d)).double(), noise, unif, exch, std, temps)
    assert frames.shape == (C.N_EXCHANGES, C.B, n * d) and frames.dtype == torch.float64
    assert np.array_equal(step.n_accepted.numpy(), G[key + "acc"]) and np.array_equal(step.n_exchanged.numpy(), G[key + "exch"])
    assert step.n_exchanged.dtype == torch.int32 and step.n_proposed == C.N_STEPS
    state = final.as_dict()
    assert state["energies_up_to_date"]
    x, e, e64 = state["samples"][0].numpy(), state["energies"].numpy(), G[key + "e64"]
    assert np.abs(x[G[key + "rows"]] - G[key + "x64"]).max() <= 1e-12
    assert np.max(np.abs(e - e64) / (1 + np.abs(e64))) <= 1e-12
    fr = C.FRAME_LADDERS * C.K
    assert np.abs(frames[:, :fr].numpy() - G[key + "frames64"]).max() <= 1e-12
    walkers = step.walkers.numpy().reshape(C.L, C.K)
    assert np.array_equal(np.sort(walkers, axis=1), np.tile(np.arange(C.K), (C.L, 1)))
    assert 0.10 <= step.n_exchanged.sum().item() / (C.L * C.N_EXCHANGES) <= 0.90


def test_rule_hand_cases():
    e = torch.tensor([3.0, -1.0, 2.0, 7.0, 0.5, 0.25], dtype=torch.float64)          # two ladders of three
    r = torch.full((6,), 0.999999, dtype=torch.float64)
    # equal temperatures: c = 0 < -log r for every r < 1 -- always exchanged
    perm, lower, swap = sampling.exchange_permutation(e, torch.ones(6, dtype=torch.float64), r, 3, 0)
    assert lower.tolist() == [0, 3] and swap.tolist() == [True, True] and perm.tolist() == [1, 0, 2, 4, 3, 5]
    perm, lower, swap = sampling.exchange_permutation(e, torch.ones(6, dtype=torch.float64), r, 3, 1)
    assert lower.tolist() == [1, 4] and swap.tolist() == [True, True] and perm.tolist() == [0, 2, 1, 3, 5, 4]
    # the rule itself: c = -(e1 - e0) (1 / T1 - 1 / T0); the hot slot holding the LOWER energy always exchanges (c < 0)
    temps = torch.tensor([1.0, 2.0, 4.0] * 2, dtype=torch.float64)
    c0 = -(-1.0 - 3.0) * (0.5 - 1.0)               # ladder 0, pair (0, 1): -2, exchanged whatever r
    c1 = -(0.5 - 7.0) * (0.5 - 1.0)                # ladder 1, pair (0, 1): -3.25 ... also c < 0
    assert c0 < 0 and c1 < 0
    _, _, swap = sampling.exchange_permutation(e, temps, r, 3, 0)
    assert swap.tolist() == [True, True]
    # ... and the cold slot holding the lower energy exchanges iff -log r > c: pair (1, 2) of ladder 0, c = -(2 + 1) (0.25 - 0.5) = 0.75
    for rr, want in ((np.exp(-0.76), True), (np.exp(-0.74), False)):
        _, lower, swap = sampling.exchange_permutation(e, temps, torch.full((6,), rr, dtype=torch.float64), 3, 1)
        assert lower.tolist() == [1, 4] and bool(swap[0]) is want
    # a NaN energy on either side never exchanges
    for bad in (0, 1):
        en = e.clone()
        en[bad] = float("nan")
        _, _, swap = sampling.exchange_permutation(en, torch.ones(6, dtype=torch.float64), torch.full((6,), 1e-300, dtype=torch.float64), 3, 0)
        assert swap.tolist() == [False, True]
    # K = 2, odd parity: no pair
    perm, lower, swap = sampling.exchange_permutation(e, torch.ones(6, dtype=torch.float64), r, 2, 1)
    assert lower.numel() == 0 and perm.tolist() == list(range(6))


@pytest.mark.parametrize("K,after_two,after_three", [(5, [1, 0, 3, 2, 4], [1, 3, 0, 4, 2]), (4, [1, 0, 3, 2], [1, 3, 0, 2])])
def test_pairs_alternate_and_a_frame_precedes_its_exchange(K, after_two, after_three):
    """every draw tiny (everything accepted): pairs (0,1),(2,3) then (1,2),(3,4); the state ``forward`` returns after a step -- the frame an
    ``IterativeSampler`` records -- does not have that step's exchange yet"""
    energy = bg.NormalDistribution(2)
    torch.manual_seed(2)
    noise = torch.randn(3, K, 2)                          # the recorded proposals: with every draw accepted, x' = x + 0.1 noise[step]
    step = bg.ReplicaExchangeMCMCStep(energy, [1.0 + k for k in range(K)], proposal=RecordedProposal(noise, 0.1))
    x0 = torch.arange(2.0 * K).reshape(K, 2) / K
    original = torch.rand_like
    torch.rand_like = lambda like: torch.full_like(like, 1e-30)
    try:
        sampler = bg.IterativeSampler(bg.SamplerState(samples=x0), [step])
        f1 = sampler.sample(1)
        assert step.steps_done == 1 and step.n_exchange_attempts == 0 and step.walkers is None       # due, not applied: the frame is before it
        f2 = sampler.sample(1)
        assert step.walkers.tolist() == after_two and step.n_exchange_attempts == 1
        f3 = sampler.sample(1)
        assert step.walkers.tolist() == after_three and step.n_exchange_attempts == 2
        want = [1 if k % 2 == 0 and k + 1 < K else 0 for k in range(K)]
        want = [w + (1 if k % 2 == 1 and k + 1 < K else 0) for k, w in enumerate(want)]
        assert step.n_exchanged.tolist() == want
        final = step.apply_pending_exchange(sampler.state)
        assert step.n_exchange_attempts == 3 and step.walkers.tolist() != after_three
    finally:
        torch.rand_like = original
    assert f1.shape == f2.shape == f3.shape == (1, K, 2) and final.as_dict()["samples"][0].shape == (K, 2)
    # what the frames hold: frame 1 is the first step's result in the start order; frame 2 is the second step applied to frame 1 with the
    # pairs (0,1), (2,3) exchanged -- itself not yet exchanged by (1,2), (3,4); that exchange shows in frame 3, and the last one only in
    # the state ``apply_pending_exchange`` returns
    even = torch.tensor([k + 1 if k % 2 == 0 and k + 1 < K else k - 1 if k % 2 == 1 else k for k in range(K)])
    odd = torch.tensor([k + 1 if k % 2 == 1 and k + 1 < K else k - 1 if k % 2 == 0 and k >= 1 else k for k in range(K)])
    assert torch.equal(f1[0], x0 + 0.1 * noise[0])
    assert torch.equal(f2[0], f1[0][even] + 0.1 * noise[1]) and not torch.equal(f2[0], f1[0] + 0.1 * noise[1])
    assert torch.equal(f3[0], f2[0][odd] + 0.1 * noise[2])
    assert torch.equal(final.as_dict()["samples"][0], f3[0][even])
    assert step.n_accepted.tolist() == [3] * K            # acceptance counts belong to the slot


def test_split_forward_calls_give_the_same_chain():
    energy = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    torch.manual_seed(5)
    x0 = torch.randn(12, 8, dtype=torch.float64)
    out = []

    def new(n_steps):
        return bg.ReplicaExchangeMCMCStep(energy, [1.0, 2.0, 4.0], proposal=bg.GaussianProposal(0.3), n_steps=n_steps, exchange_every=3)

    for calls in ("one", "seven", "two objects"):
        torch.manual_seed(17)
        state = bg.SamplerState(samples=x0)
        if calls == "one":
            step = new(7)
            state = step(state)
        elif calls == "seven":
            step = new(1)
            for _ in range(7):
                state = step(state)
        else:                                      # 3 steps, then another object told where the run stands: it makes the exchange due after step 3
            first, step = new(3), new(4)
            state = first(state)
            assert first.n_exchange_attempts == 0
            step.steps_done = first.steps_done
            state = step(state)
        assert step.steps_done == 7 and step.n_exchange_attempts == 2
        out.append(state.as_dict()["samples"][0])
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    assert out[0].shape == (12, 8) and not torch.equal(out[0], x0)
    with pytest.raises(ValueError, match="whole number of ladders"):
        bg.ReplicaExchangeMCMCStep(energy, [1.0, 2.0, 4.0])(bg.SamplerState(samples=x0[:10]))
    for bad in ([1.0], [1.0, -2.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            bg.ReplicaExchangeMCMCStep(energy, bad)
    with pytest.raises(ValueError):
        bg.ReplicaExchangeMCMCStep(energy, [1.0, 2.0], exchange_every=0)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_signatures_symbols_and_import_paths(hip_lib):
    E = inspect.Parameter.empty
    sig = _params(bg.ReplicaExchangeMCMCStep.__init__)
    assert [n for n, _ in sig] == ["target_energy", "temperatures", "proposal", "n_steps", "exchange_every"]
    assert isinstance(sig[2][1], bg.GaussianProposal) and sig[3][1] == 1 and sig[4][1] == 1 and issubclass(bg.ReplicaExchangeMCMCStep, bg.MCMCStep)
    assert _params(bg.ReplicaExchangeSampler.__init__)[:7] == [("energy", E), ("init_state", E), ("temperatures", E), ("noise_std", .1),
                                                                ("stride", 1), ("n_burnin", 0), ("exchange_every", 1)]
    assert _params(bg.ReplicaExchangeMetropolisGauss.__init__) == [("energy_function", E), ("x0", E), ("temperatures", E), ("noise", 0.1),
                                                                   ("burnin", 0), ("stride", 1), ("mapper", None)]
    assert _params(bg.ReplicaExchangeMetropolisGauss.run) == [("nepochs", 1), ("nsteps_per_epoch", 1), ("verbose", 0)]
    assert _params(sampling.pair_mcmc)[-7:] == [("n_replicas", 0), ("exchange_every", 1), ("exchange_phase", 0), ("exchange_parity", 0),
                                                ("exchange_uniforms", None), ("n_exchanged", None), ("walkers", None)]
    assert [n for n, _ in _params(bg.ReplicaExchangeMCMCStep.feed_noise)] == ["noise", "uniforms", "exchange_uniforms"]
    sigs = abi_signatures()
    i32, p = ctypes.c_int32, ctypes.c_void_p
    for plain, name in (("bgk_pair_mcmc", "bgk_pair_remc"), ("bgk_box_mcmc", "bgk_box_remc")):
        assert name in abi_symbols() and sigs[name] == (ctypes.c_int, sigs[plain][1] + [i32, i32, i32, i32, p, p, p])
        assert list(getattr(hip_lib, name).argtypes) == sigs[name][1]
    for path in ("distribution.sampling._mcmc.metropolis", "distribution.sampling._mcmc"):
        mod = importlib.import_module("bgflow_amd." + path)
        assert mod.ReplicaExchangeMetropolisGauss is bg.ReplicaExchangeMetropolisGauss and mod.MetropolisGauss is bg.MetropolisGauss
    for path in ("distribution.sampling", "distribution.sampling.mcmc"):
        mod = importlib.import_module("bgflow_amd." + path)
        assert mod.ReplicaExchangeMCMCStep is bg.ReplicaExchangeMCMCStep and mod.ReplicaExchangeSampler is bg.ReplicaExchangeSampler
    # the shortcut class
    energy = bg.DoubleWellEnergy(2)
    torch.manual_seed(0)
    s = bg.ReplicaExchangeSampler(energy, torch.randn(6, 2), [1.0, 2.0, 3.0], noise_std=0.3, stride=2, n_burnin=3, exchange_every=2)
    assert s.sample(4).shape == (4, 6, 2)
    step = s.sampler_steps[0]
    assert isinstance(step, bg.ReplicaExchangeMCMCStep) and step.steps_done == 14 and step.n_exchange_attempts == 6 and step.exchange_every == 2
    assert step.n_exchanged.shape == (6,) and step.walkers.shape == (6,) and step.n_proposed == 14


def test_tile_heights_and_the_envelope_of_the_entries(hip_lib):
    """the heights of csrc/bgk_mcmc.hip's table; K beyond them is BGK_EUNSUPPORTED (-2), a batch or row0 that is no multiple of K and a
    missing temperature tensor BGK_EINVAL (-1) -- argument checks, before any launch; on the CPU the fused setup is None"""
    assert [sampling.mcmc_tile_rows(nd) for nd in (192, 39, 8, 76, 128)] == [41, 64, 64, 64, 61]
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def pair(batch=0, n=64, K=41, every=1, phase=0, parity=0, row0=0, temps=fake, noise=None, exu=None, d=3):
        return hip_lib.bgk_pair_remc(fake, batch, n, d, 0, 1.0, 1.0, 0.0, 0.0, 0.0, fake, 0, 1.0, temps, 0.1, 2, noise, noise, 1, 0, row0,
                                     None, None, 0, None, 0, None, K, every, phase, parity, exu, None, None)

    prm = (ctypes.c_float * 12)(0.7, 1.21, 0.9, 0.81, 150.0, -1.0, 25.0, 10.0, 1.5, 20.0, 3.0, 100.0)

    def box(batch=0, n=64, K=61):
        return hip_lib.bgk_box_remc(fake, batch, n, 3, prm, 12, fake, 0, 1.0, fake, 0.1, 2, None, None, 1, 0, 0, None, None, 0, None, 0, None,
                                    K, 1, 0, 0, None, None, None)

    assert pair() == 0 and box() == 0                                              # an empty batch: nothing to do
    assert pair(batch=84, K=42) == -2 and b"replicas" in hip_lib.bgk_last_error()
    assert pair(batch=130, n=13, K=65) == -2 and box(batch=124, K=62) == -2
    assert pair(batch=83) == -1 and pair(batch=82, row0=40) == -1 and pair(batch=82, temps=None) == -1
    for bad in (dict(K=1), dict(K=0), dict(K=-3), dict(every=0), dict(every=2, phase=2), dict(phase=-1), dict(parity=2)):
        assert pair(**bad) == -1, bad
    assert pair(noise=fake) == -1 and pair(exu=fake) == -1                         # explicit numbers: all or none
    # the Python restatement of the tile height against the C side, for every shape of the envelope: K = the height passes the argument
    # checks (an empty batch: no launch), K = the height + 1 is BGK_EUNSUPPORTED
    for n in range(2, 65):
        for d in (1, 2, 3):
            rows = sampling.mcmc_tile_rows(n * d)
            assert pair(n=n, d=d, K=rows) == 0 and pair(n=n, d=d, K=rows + 1) == -2, (n, d, rows)
        rows = sampling.mcmc_tile_rows(2 * n)
        assert box(n=n, K=rows) == 0 and box(n=n, K=rows + 1) == -2, (n, rows)
    # so K = 43 at n d = 192 is beyond the kernel and the step takes the general path, without an error (on the device:
    # test_gpu_remc.py::test_fused_envelope_on_the_device; here, without one, the general path runs whatever K)
    assert sampling.mcmc_tile_rows(192) == 41 < 43
    lj = bg.LennardJonesPotential(192, 64, two_event_dims=False)
    step = bg.ReplicaExchangeMCMCStep(lj, torch.linspace(1.0, 2.0, 43))
    assert step._fused_setup(bg.SamplerState(samples=torch.zeros(86, 192))) is None


def test_due_exchange_is_counted_once_with_the_launch_stubbed(monkeypatch):
    """the fused path's bookkeeping without a device: the launch is a stub that advances x by 1 per step, writes the frames and, after
    every step that completes an epoch, makes an "exchange" the way the kernel does -- x negated, ``n_exchanged[0]`` counted, ``walkers``
    reversed.  After ``sample(4)`` at ``exchange_every = 1`` the last exchange is in the working chains and in the counters: asking for
    it -- through the sampler's state, or for a state from elsewhere -- must not count or apply it a second time."""
    K, L = 3, 2
    B = K * L
    energy = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    launches = []

    def stub(plan, x, e, e_valid, temperature, noise_std, n_steps, noise=None, uniforms=None, seed=0, offset=0, row0=0, traj=None,
             traj_e=None, traj_every=0, n_accepted=None, accumulate=False, n_replicas=0, exchange_every=1, exchange_phase=0,
             exchange_parity=0, exchange_uniforms=None, n_exchanged=None, walkers=None):
        launches.append((n_steps, exchange_phase, exchange_parity))
        if not accumulate:
            n_accepted.zero_()
            n_exchanged.zero_()
        frame = 0
        for s in range(n_steps):
            x += 1
            if traj is not None and (s + 1) % traj_every == 0:
                traj[frame], traj_e[frame] = x, e
                frame += 1
            if (exchange_phase + s + 1) % exchange_every == 0:
                x.neg_()
                n_exchanged[0] += 1
                walkers.copy_(walkers.flip(0))

    monkeypatch.setattr(sampling, "pair_mcmc", stub)
    monkeypatch.setattr(bg.ReplicaExchangeMCMCStep, "_fused_setup", lambda self, state: (None, B, None))

    def run():
        step = bg.ReplicaExchangeMCMCStep(energy, [1.0, 2.0, 4.0], proposal=bg.GaussianProposal(0.1))
        sampler = bg.IterativeSampler(bg.SamplerState(samples=torch.zeros(B, 8)), [step])
        frames = sampler.sample(4)
        assert frames[:, 0, 0].tolist() == [1.0, 0.0, 1.0, 0.0] and step.steps_done == 4 and step.n_exchange_attempts == 4
        assert int(step.n_exchanged[0]) == 4 and step._exchange_due()
        return step, sampler

    # the sampler's own state: the working chains, no counter moves
    step, sampler = run()
    assert launches[-2:] == [(3, 0, 0), (1, 0, 1)]                       # the run's last step is a launch of its own
    walkers = step.walkers.clone()
    after = step.apply_pending_exchange(sampler.state)
    assert step.n_exchange_attempts == 4 and int(step.n_exchanged[0]) == 4 and torch.equal(step.walkers, walkers)
    assert not step._exchange_due() and float(after.as_dict()["samples"][0][0, 0]) == 0.0 and float(sampler.state.as_dict()["samples"][0][0, 0]) == 0.0
    assert float(sampler.sample(1)[0, 0, 0]) == 1.0 and step.n_exchange_attempts == 5      # goes on from the exchanged chains: -0 + 1
    # a state from elsewhere: the stub's last exchange leaves the counters, the rule's (torch ops, every draw tiny) comes in
    step, sampler = run()
    other = bg.SamplerState(samples=sampler.state.as_dict()["samples"][0].clone())
    original = torch.rand_like
    torch.rand_like = lambda like: torch.full_like(like, 1e-30)
    try:
        after = step.apply_pending_exchange(other)
    finally:
        torch.rand_like = original
    assert step.n_exchange_attempts == 4 and not step._exchange_due() and step._handed is None
    assert step.n_exchanged.tolist() == [3, 1, 0, 0, 1, 0]               # three of the stub, then pair (1, 2) of either ladder
    assert step.walkers.tolist() == [2, 0, 1, 2, 0, 1]                  # reversed three times = [2,1,0,2,1,0]; then slots 1 and 2 swapped
    assert after.as_dict()["samples"][0].shape == (B, 8)
    # ... and continuing from a state from elsewhere, inside the next run
    step, sampler = run()
    sampler.state = bg.SamplerState(samples=sampler.state.as_dict()["samples"][0].clone())
    sampler.sample(1)
    assert step.n_exchange_attempts == 5 and step.steps_done == 5       # 3 + the torch exchange + the next run's own
