"""GPU (-m gpu): the fused annealed switching -- ``AnnealedSwitching`` / ``AnnealedMCFlow`` on bgk_pair_anneal / bgk_box_anneal
(csrc/bgk_anneal.hip) -- against the reference's ``MCMCStep`` driven stage by stage in f64 on fixed random numbers
(tests/golden/anneal.npz, written by tests/golden/make_anneal_goldens.py), and bitwise against itself and against the Metropolis chain
kernel: in-kernel Philox = the same numbers handed in, sharded / capped runs = the run in one piece, a constant schedule = bgk_pair_mcmc,
returned energies = ``energy.energy`` of the returned states.

Bounds of the parity test, on the chains the fixture keeps (f64 decision margin >= 1e-3 at every step): accept counts equal;
|x - x64| <= 4 err_x32 + 1e-6, |W - W64| / (1 + |W64|) <= 4 err_w32 + 1e-6 and |e - e64| / (1 + |e64|) <= 4 err_e32 + 1e-6 for either end,
err_* the errors of the reference's own f32 run of the same chains -- the project's bound for the pair kernels.

B = 150 (a partial last tile of either tile height: 64 rows, 41 rows at n d = 192; three or four workgroups).  Every protocol here runs
with ``fused = "always"``: the tests are of the kernel, whatever ``fused = True`` chooses."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import annealing

from anneal_common import B, CASES, bar_check, make_end, start_state, switching
from mcmc_common import random_numbers

pytestmark = pytest.mark.gpu


def always(sw, x0=None):
    sw.fused = "always"
    if x0 is not None:
        assert sw._fused_setup(x0) is not None, "the case must take the fused path"
    return sw


def philox_numbers(seed, offset, n_steps, batch, nd, dev):
    """what bgk_philox_fields writes for (seed, offset + s), fields [normal nd, uniform 1]"""
    from bgflow_amd.distributions import philox_sample
    noise, unif = [], []
    for s in range(n_steps):
        (eps, r), _ = philox_sample([(1, nd, None, None, 1.0, 0.0), (0, 1, None, None, 1.0, 0.0)], batch, dev, seed, offset + s)
        noise.append(eps)
        unif.append(r[:, 0])
    return torch.stack(noise), torch.stack(unif)


def stream_seed(obj):
    from bgflow_amd import dp
    st = obj._philox_ids()
    return (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1), st[1]


@pytest.fixture(scope="module")
def runs(hip_lib, dev, golden):
    """a fixture case through the kernel on the recorded numbers, computed once per case"""

    @functools.lru_cache(maxsize=None)
    def run(key):
        sw, x0 = switching(golden, key, device=dev)
        always(sw, x0)
        start = x0.clone()
        x, work = sw(x0)
        assert torch.equal(x0, start), "the caller's start tensor is not touched"
        return dict(x=x, work=work, e_a=sw.e_a, e_b=sw.e_b, acc=sw.n_accepted, n_proposed=sw.n_proposed, sw=sw)

    return run


@pytest.mark.parametrize("key", list(CASES))
def test_parity_on_recorded_numbers(runs, golden, key):
    G = golden("anneal")
    r = runs(key)
    keep = G[key + "_keep"]
    assert keep.mean() >= 0.85 and r["n_proposed"] == 12
    assert r["work"].dtype == torch.float64 and r["work"].shape == (B,) and r["x"].dtype == torch.float32
    acc = r["acc"].cpu().numpy()
    assert acc.dtype == np.int32 and np.array_equal(acc[keep], G[key + "_acc"][keep])
    x, w = r["x"].cpu().numpy().astype(np.float64), r["work"].cpu().numpy()
    bound_x, bound_w, bound_e = (4 * float(G[key + f"_err_{q}32"]) + 1e-6 for q in "xwe")
    err_x = np.abs(x[:8] - G[key + "_x64"])[keep[:8]].max()
    w64 = G[key + "_work64"]
    err_w = (np.abs(w - w64) / (1 + np.abs(w64)))[keep].max()
    err_e = 0.0
    for got, want in ((r["e_a"], G[key + "_e_a64"]), (r["e_b"], G[key + "_e_b64"])):
        err_e = max(err_e, (np.abs(got.cpu().numpy().astype(np.float64) - want) / (1 + np.abs(want)))[keep].max())
    print(f"{key}: kept {int(keep.sum())} / {B}; |dx| {err_x:.3g} (bound {bound_x:.3g}); work {err_w:.3g} (bound {bound_w:.3g}); "
          f"energies {err_e:.3g} (bound {bound_e:.3g})")
    assert err_x <= bound_x and err_w <= bound_w and err_e <= bound_e


@pytest.mark.parametrize("key", list(CASES))
def test_returned_energies_are_the_energy_kernels_bits(runs, key):
    r = runs(key)
    sw = r["sw"]
    assert torch.equal(r["e_a"], sw.energy_a.energy(r["x"])[:, 0]) and torch.equal(r["e_b"], sw.energy_b.energy(r["x"])[:, 0])


def pair_case(golden, dev, end_a, end_b, n, d):
    P = golden("particles")
    a, b = make_end(P, (end_a, n, d)).to(dev), make_end(P, (end_b, n, d)).to(dev)
    if (n, d) == (53, 3):               # n d = 159: the widest row bgk_philox_fields writes, and a tile of fewer than 64 rows (49)
        x0 = torch.tensor(P["x_55_3"], device=dev)[:, :53].reshape(B, -1).contiguous()
    else:
        x0 = torch.tensor(P[f"x_{n}_{d}"], device=dev).reshape(B, -1)
    return a, b, x0


LAMBDAS = [0.0, 0.05, 0.2, 0.45, 0.7, 0.9, 1.0]


@pytest.mark.parametrize("end_a,end_b,n,d,std", [("lj", "mdw", 4, 2, 0.15), ("mfn", "lj", 53, 3, 0.015)])
def test_in_kernel_philox_equals_the_same_numbers_handed_in(hip_lib, dev, golden, end_a, end_b, n, d, std):
    torch.manual_seed(1234)
    a, b, x0 = pair_case(golden, dev, end_a, end_b, n, d)
    drawn = always(bg.AnnealedSwitching(a, b, LAMBDAS, n_steps=2, noise_std=std), x0).set_philox_stream(40, calls=7)
    seed, offset = stream_seed(drawn)
    assert offset == 7
    xa, wa = drawn(x0)
    assert drawn._philox_ids()[1] == 7 + 12                                         # the counter is the index of the next step
    noise, unif = philox_numbers(seed, offset, 12, B, n * d, dev)
    fed = always(bg.AnnealedSwitching(a, b, LAMBDAS, n_steps=2, noise_std=std), x0).feed_noise(noise, unif)
    xb, wb = fed(x0)
    assert torch.equal(xa, xb) and torch.equal(wa, wb) and torch.equal(drawn.n_accepted, fed.n_accepted)
    assert torch.equal(drawn.e_a, fed.e_a) and torch.equal(drawn.e_b, fed.e_b)
    rate = float(drawn.n_accepted.float().mean()) / 12
    assert 0.1 < rate < 0.95, rate                                                  # (a run that moves: the comparison is not of frozen chains)


@pytest.mark.parametrize("key", ["mdw_mfn_13_3", "lj_mdw_64_3", "rep_harm_36"])
def test_independence_of_sharding_and_the_step_cap(hip_lib, dev, golden, monkeypatch, key):
    torch.manual_seed(99)
    sw, x0 = switching(golden, key, device=dev)
    sw.feed_noise(None, None)
    always(sw, x0).set_philox_stream(50)
    xw, ww = sw(x0)
    whole = dict(e_a=sw.e_a, e_b=sw.e_b, acc=sw.n_accepted)
    assert 0 < int(whole["acc"].sum()) < 12 * B
    # chains 64..149 alone, told where they sit in the whole
    sw.set_philox_stream(50)
    sw.chain_offset = 64
    xp, wp = sw(x0[64:].contiguous())
    assert torch.equal(xp, xw[64:]) and torch.equal(wp, ww[64:]) and torch.equal(sw.n_accepted, whole["acc"][64:])
    assert torch.equal(sw.e_a, whole["e_a"][64:]) and torch.equal(sw.e_b, whole["e_b"][64:])
    sw.chain_offset = 0
    # a cap of 5 steps -- launches [0, 5), [5, 10), [10, 12), the first two split inside a stage of 2 steps -- is the run in one launch
    monkeypatch.setattr(annealing, "ANNEAL_MAX_STEPS_PER_LAUNCH", 5)
    sw.set_philox_stream(50)
    xc, wc = sw(x0)
    assert torch.equal(xc, xw) and torch.equal(wc, ww) and torch.equal(sw.n_accepted, whole["acc"])
    assert torch.equal(sw.e_a, whole["e_a"]) and torch.equal(sw.e_b, whole["e_b"])
    # ... also with the ends' start energies handed in (the flow layer's entry)
    sw.set_philox_stream(50)
    xs, ws = sw._run(x0, start=True)
    assert torch.equal(xs, xw) and torch.equal(ws, ww) and torch.equal(sw.e_a_start, sw.energy_a.energy(x0)[:, 0])


@pytest.mark.parametrize("lam,n,d", [(0.0, 13, 3), (1.0, 13, 3), (0.0, 64, 3)])
def test_a_constant_schedule_is_the_metropolis_chain_kernel(hip_lib, dev, golden, lam, n, d):
    """lambdas = [0, 0, 0]: 2 K steps on A alone, the bits of bgk_pair_mcmc and no work; [1, 1, 1] likewise on B"""
    torch.manual_seed(17)
    lj, mdw, x0 = pair_case(golden, dev, "lj", "mdw", n, d)
    std, K = 0.03 if n == 13 else 0.015, 3
    sw = always(bg.AnnealedSwitching(lj, mdw, [lam] * 3, n_steps=K, noise_std=std), x0)
    plain = bg.MCMCStep(lj if lam == 0.0 else mdw, proposal=bg.GaussianProposal(noise_std=std), n_steps=2 * K)
    if lam == 0.0:                      # fed numbers
        noise, unif = (torch.tensor(t, device=dev) for t in random_numbers(31, n * d, 2 * K, B))
        sw.feed_noise(noise, unif)
        plain.feed_noise(noise, unif)
    else:                               # the same Philox stream
        sw.set_philox_stream(77)
        plain.set_philox_stream(78)
        plain.__dict__["_philox_state"][0] = 77
    x, work = sw(x0)
    state = bg.SamplerState(samples=x0)
    assert plain._fused_setup(state) is not None
    want = plain(state).as_dict()
    assert torch.equal(work, torch.zeros(B, dtype=torch.float64, device=dev))
    assert torch.equal(x, want["samples"][0]) and torch.equal(sw.n_accepted, plain.n_accepted)
    assert torch.equal(sw.e_a if lam == 0.0 else sw.e_b, want["energies"])
    assert 0 < int(sw.n_accepted.sum()) < 2 * K * B


def test_a_protocol_under_the_cap_is_one_launch(hip_lib, dev, golden):
    from test_gpu_round6 import _device_kernel_names
    sw, x0 = switching(golden, "mfn_lj_13_3", device=dev)
    sw.feed_noise(None, None)
    always(sw, x0).set_philox_stream(60)
    assert sw.n_stages * sw.n_steps <= annealing.ANNEAL_MAX_STEPS_PER_LAUNCH
    names = _device_kernel_names(lambda: sw(x0))
    print(names)
    # the tracer also lists memory copies: the one device-to-device copy is the working copy of the caller's tensor, not a launch
    copies = [k for k in names if k.startswith("Memcpy") or k.startswith("Memset")]
    kernels = [k for k in names if k not in copies]
    assert len(kernels) == 1 and "pair_anneal_kernel" in kernels[0], names
    assert len(copies) <= 1 and all("DtoD" in k for k in copies), names


def test_philox_layout_at_the_widest_row(hip_lib, dev):
    """n d = 192: one step from x = 0 with noise_std = 1 at temperatures that accept everything leaves x = eps, the in-kernel normals --
    the numpy restatement of the generator (oracle/philox.py) to 4e-6, the project's bound for Box-Muller in f32 against f64"""
    from oracle import philox
    n, d, rows, row0, offset = 64, 3, 100, 70, 5
    a = bg.MeanFreeNormalDistribution(n * d, n, std=1.0, two_event_dims=False).to(dev)
    b = bg.MeanFreeNormalDistribution(n * d, n, std=2.0, two_event_dims=False).to(dev)
    x0 = torch.zeros(rows, n * d, device=dev)
    sw = always(bg.AnnealedSwitching(a, b, [0.0, 0.5, 1.0], n_steps=1, noise_std=1.0, temperature_a=1e30, temperature_b=1e30), x0)
    sw.set_philox_stream(3, calls=offset)
    sw.chain_offset = row0
    seed, _ = stream_seed(sw)
    x, work = sw(x0)
    assert int(sw.n_accepted.sum()) == 2 * rows
    want = sum(philox.sample_field(seed, offset + s, 0, rows, n * d, 1, row0=row0).astype(np.float64) for s in (0, 1))
    # two steps: twice the bound of one normal, and the f32 rounding of their sum (|x| < 12: 2^-24 * 12 = 7e-7)
    np.testing.assert_allclose(x.cpu().numpy(), want, rtol=0, atol=2 * 4e-6 + 7e-7)


def test_non_finite_rows_behave_as_on_the_general_path(hip_lib, dev, golden):
    """the host test's rows on the device: e_B = +inf in row 0 where its coefficient is 0 -- work = +inf, the chain moves on, no NaN
    reaches x -- and NaN noise, which rejects every proposal; the general path on the device (the same energy kernels) decides alike"""
    P = golden("particles")
    x0 = torch.tensor(start_state(golden, ("rep", 2)), device=dev)[:8].clone()
    x0[0, 6:8] = x0[0, 4:6]
    harm, rep = make_end(P, ("harm", 2)).to(dev), make_end(P, ("rep", 2)).to(dev)
    assert torch.isinf(rep.energy(x0)[0, 0]) and torch.isfinite(harm.energy(x0)).all()
    noise, unif = (torch.tensor(t, device=dev) for t in random_numbers(37, 8, 4, 8))
    nan_noise = torch.full((1, 8, 8), float("nan"), device=dev)
    for lambdas, K, feed in (([0.0, 0.5, 1.0], 2, (noise, unif)), ([0.0, 0.0], 2, (noise, unif)), ([0.0, 1.0], 1, (nan_noise, unif[:1].contiguous()))):
        sw = always(bg.AnnealedSwitching(harm, rep, lambdas, n_steps=K, noise_std=0.05), x0).feed_noise(*feed)
        x, work = sw(x0)
        ref = bg.AnnealedSwitching(harm, rep, lambdas, n_steps=K, noise_std=0.05).feed_noise(*feed)
        ref.fused = False
        xr, wr = ref(x0)
        assert torch.equal(x, xr) and torch.equal(work, wr) and torch.equal(sw.n_accepted, ref.n_accepted)
        assert torch.equal(sw.e_a, ref.e_a) and torch.equal(sw.e_b, ref.e_b)
        assert torch.isfinite(x).all()
        if lambdas == [0.0, 0.5, 1.0]:
            assert work[0] == float("inf") and torch.isfinite(work[1:]).all() and int(sw.n_accepted[0]) >= 1
            assert torch.isfinite(sw.e_b).all()
        elif lambdas == [0.0, 0.0]:
            assert torch.equal(work, torch.zeros(8, dtype=torch.float64, device=dev))
        else:
            assert torch.equal(x, x0) and int(sw.n_accepted.sum()) == 0 and work[0] == float("inf")


def test_fallbacks_take_the_general_path_and_agree_with_it(hip_lib, dev, golden):
    P = golden("particles")
    n, d = 4, 2
    lj, mdw = make_end(P, ("lj", n, d)).to(dev), make_end(P, ("mdw", n, d)).to(dev)
    x0 = torch.tensor(start_state(golden, ("lj", n, d)), device=dev)
    noise, unif = (torch.tensor(t, device=dev) for t in random_numbers(43, n * d, 12, B))

    def general(a, b, x, std=0.15):
        ref = bg.AnnealedSwitching(a, b, LAMBDAS, n_steps=2, noise_std=std).feed_noise(noise, unif)
        ref.fused = False
        return ref(x)

    def falls_back(a, b, x, std=0.15):
        sw = bg.AnnealedSwitching(a, b, LAMBDAS, n_steps=2, noise_std=std).feed_noise(noise, unif)
        sw.fused = "always"
        assert sw._fused_setup(x) is None
        got, want = sw(x), general(a, b, x, std)
        assert torch.equal(got[0].detach(), want[0].detach()) and torch.equal(got[1].detach(), want[1].detach())
        assert got[0].dtype == x.dtype and got[1].dtype == torch.float64 and sw.n_proposed == 12
        return sw, got

    # the fused path itself takes the general path's decisions (the same energy bits): the same states on the chains whose margin is wide
    fused = always(bg.AnnealedSwitching(lj, mdw, LAMBDAS, n_steps=2, noise_std=0.15), x0).feed_noise(noise, unif)
    xf, wf = fused(x0)
    xg, wg = general(lj, mdw, x0)
    same = (xf == xg).all(dim=1)
    assert float(same.float().mean()) >= 0.95 and torch.equal(wf[same], wg[same])
    # ends of mismatched (n, d) over the same 8 columns
    line = bg.MeanFreeNormalDistribution(8, 8, std=0.8, two_event_dims=False).to(dev)
    falls_back(line, lj, x0)
    # an f64 input
    _, (x64, w64) = falls_back(lj, mdw, x0.double())
    assert float(((x64.float() - xg).abs().amax(dim=1) < 1e-4).float().mean()) >= 0.9
    # a tensor-valued noise_std
    falls_back(lj, mdw, x0, std=torch.tensor(0.15, device=dev))
    # an input that requires grad
    xr = x0.clone().requires_grad_(True)
    _, (y, w) = falls_back(lj, mdw, xr)
    (g,) = torch.autograd.grad(w.sum(), xr)
    assert torch.isfinite(g).all()
    with torch.no_grad():
        assert fused._fused_setup(xr) is not None
    # fused = False; fused = True takes the kernel here (64 rows per tile) and not at n d = 192 (41 rows: measured slower)
    plain = bg.AnnealedSwitching(lj, mdw, LAMBDAS, n_steps=2, noise_std=0.15)
    assert plain.fused is True and plain._fused_setup(x0) is not None
    plain.fused = False
    assert plain._fused_setup(x0) is None
    wide, xw = switching(golden, "mfn_lj_64_3", device=dev)
    assert wide.fused is True and wide._fused_setup(xw) is None
    wide.fused = "always"
    assert wide._fused_setup(xw) is not None


def test_annealed_mc_flow_on_the_kernel(hip_lib, dev, golden):
    P = golden("particles")
    n, d = 13, 3
    prior, target = make_end(P, ("mfn", n, d)).to(dev), make_end(P, ("lj", n, d)).to(dev)
    z = torch.tensor(start_state(golden, ("lj", n, d)), device=dev)
    flow = bg.AnnealedMCFlow(prior, target, LAMBDAS, nsteps=2, stepsize=0.04)
    always(flow.switching, z).set_philox_stream(90)
    gen = bg.BoltzmannGenerator(prior, flow, target)
    x, dW = flow(z)
    sw = always(bg.AnnealedSwitching(prior, target, LAMBDAS, n_steps=2, noise_std=0.04), z).set_philox_stream(91)
    sw.__dict__["_philox_state"][0] = 90
    x2, work = sw(z)
    assert torch.equal(x, x2) and dW.shape == (B, 1) and dW.dtype == torch.float32
    logw = gen.log_weights_given_latent(x, z, dW, normalize=False).double()
    e_a, e_b = prior.energy(z)[:, 0].double().abs(), target.energy(x)[:, 0].double().abs()
    slack = 4 * 2.0 ** -23 * (e_a + e_b + dW[:, 0].double().abs() + work.abs())      # a few f32 roundings of the operands
    assert bool(((logw + work).abs() <= slack).all())


def test_bar_of_forward_and_reverse_work_with_in_kernel_philox(hip_lib, dev):
    """the host suite's statistical check on the kernel: -6 ln 0.8 = 1.3389 within five reported standard errors, themselves <= 0.02"""
    torch.manual_seed(2026)
    prior = bg.MeanFreeNormalDistribution(8, 4, std=1.0, two_event_dims=False).to(dev)
    target = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False).to(dev)
    x_f, x_r = prior.sample(4096), target.sample(4096)
    df, ddf, exact, sw, rv = bar_check(prior, target, x_f, x_r, fused="always", stream=70)
    assert sw._fused_setup(x_f) is not None and rv._fused_setup(x_r) is not None
    rate = float(sw.n_accepted.float().mean()) / sw.n_proposed
    print(f"BAR {df:.4f} +- {ddf:.4f}, exact {exact:.4f}; forward acceptance {rate:.2f}")
    assert sw.n_proposed == 64 and 0.3 < rate < 0.95
    assert abs(df - exact) <= 5 * ddf
    assert ddf <= 0.02
