"""GPU (-m gpu): every consumer of the kernels' Philox draws at a word from either end of the 32-bit range.  ``u01`` (csrc/bgk_philox.h)
maps the 256 largest words ("top") to 1 - 2^-24 -- without its clamp, to exactly 1.0: a uniform draw on ``high``, a refused replica
exchange at equal temperatures -- and the 256 smallest ("bottom") to 2^-25, the largest Box-Muller radius sqrt(50 ln 2) = 5.887.  Either
kind turns up once per 2^24 draws, so tests/golden/philox_edges.npz records global rows at which the kernels' counter layouts meet one
(philox_edges_common.py re-derives them), and every test here passes ``row0`` so that such a row sits in a batch of one tile or less.

All shapes: B <= 64, d <= 8, chains of 4 particles in 2 dimensions, <= 3 steps.  No assertion leaves an element out."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import annealing, modulo, sampling, stochastic
from bgflow_amd.distributions import _kernel_plan, philox_sample
from oracle import philox

import philox_edges_common as C
from mcmc_common import make

pytestmark = pytest.mark.gpu

D = 7              # columns of the prior fields: two counter blocks, the second one partial


def T(a, dev):
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the device probe: u01 and the Box-Muller pair on chosen words ------------------------------------------------------------------
def _probe(hip_lib, dev, words, which):
    from bgflow_amd import _lib
    xd = torch.from_numpy(words.view(np.int32).copy()).to(dev)                     # the word IS the input's bit pattern
    out = torch.empty(xd.numel(), dtype=torch.float32, device=dev)
    assert hip_lib.bgk_detmath_probe(_lib.ptr(xd), xd.numel(), which, _lib.ptr(out), _lib.stream_ptr(dev)) == 0
    return out.cpu().numpy()


def test_probe_u01_and_box_muller(hip_lib, oracle, dev):
    """bgk_detmath_probe codes 7 (u01), 8 / 9 (the cos / sin member of philox_normal4 on the words of elements (i, i + 1)) on the words
    k << 8 | j, k in [0, 4096), [2^23 - 2048, 2^23 + 2048), [2^24 - 4096, 2^24) and every 257th k, j in {0, 255}: u01 has the bits of
    oracle/philox.py::u01; the normals are finite and within 4e-6 of f64 Box-Muller of the same two u's.  The bound: the suite's 4e-6
    for |n| <= 1; above, 4 x the worst error of the plain numpy-f32 evaluation of the formula on these words, never less than 4e-6 --
    measured on the host (test_host_philox_edges.py): 6.1e-7 at |n| > 1 (radii up to 5.887), so 4e-6 holds there too.  The normals
    also have the bits of the C oracle's mirror of the probe (the deterministic log / sincos, a correctly rounded square root)."""
    ref = C.probe_reference()
    w = ref["w"]
    u = _probe(hip_lib, dev, w, 7)
    assert np.array_equal(u.view(np.uint32), ref["u"].view(np.uint32))
    assert u.min() == C.U_MIN and u.max() == C.U_MAX
    for code, name, want in ((8, "normal_cos", ref["cos64"]), (9, "normal_sin", ref["sin64"])):
        got = _probe(hip_lib, dev, w, code)
        assert np.isfinite(got).all()
        host = oracle.detmath_probe(w.view(np.float32), name)
        assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), f"{name}: {np.sum(got != host)} of {got.size} differ from the C oracle"
        err = np.abs(got.astype(np.float64) - want)
        bound = C.normal_bound(want, ref["err32_large"])
        big = np.abs(want) > 1.0
        print(f"code {code}: max error {err[~big].max():.3g} at |n| <= 1, {err[big].max():.3g} at |n| > 1 (up to {np.abs(want).max():.4f}); "
              f"numpy f32 {ref['err32_small']:.3g} / {ref['err32_large']:.3g}; bound {bound.min():.3g} / {bound.max():.3g}")
        assert (err <= bound).all()


# ---- bgk_philox_fields ----------------------------------------------------------------------------------------------------------------
def _restated_uniform(e, row0, B, field, low, high):
    """low + u (high - low) in numpy f32 on the restated u: the kernel's two operations"""
    u = philox.sample_field(e.seed, e.offset, field, B, D, 0, row0=row0)
    return np.float32(low) + u * (np.float32(high) - np.float32(low))


@pytest.mark.parametrize("low,high", [(0.0, 1.0), (0.0, 2.0), (-4.0, 4.0), (0.0, 3.0)])
@pytest.mark.parametrize("layout,field", [("field0", 0), ("field1", 1)])
def test_uniform_fields_at_a_top_word_stay_below_high(hip_lib, dev, layout, field, low, high):
    """two uniform fields of 7 columns with the targeted row on lanes 0, 1, 37, 63 of a 64-row tile and as a batch of one: the whole tile
    has the bits of low + u (high - low) of the restatement, the targeted row the same bits in every launch, and every element lies in
    [low, high) -- for the widths 1, 2 and 8, powers of two, where u (high - low) is exact.  For (0, 3) the f32 product u * 3 may round up
    to 3 for u < 1 exactly as the reference's own `low + rand * (high - low)` does: there equality with the restatement is the
    assertion, and `<= high`."""
    lo_t, hi_t = torch.full((D,), low, device=dev), torch.full((D,), high, device=dev)
    spec = [(0, D, lo_t, hi_t, 1.0, 0.0)] * 2
    for e in C.select(layout, True) + C.select(layout, False):
        seen = []
        for row0, B, lane in C.launches(e):
            outs, _ = philox_sample(spec, B, dev, e.seed, e.offset, row0=row0)
            for f, out in enumerate(outs):
                got = out.cpu().numpy()
                assert np.array_equal(got.view(np.uint32), _restated_uniform(e, row0, B, f, low, high).view(np.uint32)), (e, row0, f)
                assert (got >= low).all()
                assert (got < high).all() if high - low in (1.0, 2.0, 8.0) else (got <= high).all(), (e, row0, f, got.max())
            hit = outs[field][lane, e.word].item()
            want = np.float32(low) + (C.U_MAX if e.top else C.U_MIN) * np.float32(high - low)
            assert hit == want, (e, hit)
            seen.append(torch.stack([o[lane] for o in outs]))
        assert all(torch.equal(bits(s), bits(seen[0])) for s in seen)


@pytest.mark.parametrize("layout,field", [("field0", 0), ("field1", 1)])
def test_normal_fields_and_their_energy_at_the_edges(hip_lib, dev, layout, field):
    """two standard-normal fields with the launch's prior energy: a top word as u1 (radius 3.5e-4) and as u2 (angle 2 pi (1 - 2^-24)) and
    a bottom word as u1 (radius 5.887) and as u2: every sample finite and within the bound of test_probe_u01_and_box_muller of the f64
    restatement; the energy finite and within rtol 3e-6, atol 1e-4 (test_fused_philox_prior_sampling's bound) of bgk_energy_fields on the
    returned tensors"""
    err32 = C.probe_reference()["err32_large"]
    e_const = float(D / 2 * np.log(2 * np.pi))
    spec = [(1, D, None, None, 1.0, e_const)] * 2
    prior = bg.ProductDistribution([bg.NormalDistribution(D).to(dev), bg.NormalDistribution(D).to(dev)])
    for e in [s for top in (True, False) for parity in (0, 1) for s in C.select(layout, top, parity)]:
        seen = []
        for row0, B, lane in C.launches(e, lanes=(0, 37, 63)):
            outs, energy = philox_sample(spec, B, dev, e.seed, e.offset, row0=row0, want_energy=True)
            for f, out in enumerate(outs):
                got = out.cpu().numpy()
                want = philox.sample_field(e.seed, e.offset, f, B, D, 1, row0=row0)
                assert np.isfinite(got).all()
                assert (np.abs(got - want) <= C.normal_bound(want, err32)).all(), (e, row0, f, np.abs(got - want).max())
            pair = outs[field][lane, e.word & ~1:(e.word & ~1) + 2].cpu().numpy().astype(np.float64)
            if e.word % 2 == 0:
                assert abs(np.hypot(*pair) - (np.sqrt(-2 * np.log1p(-2.0 ** -24)) if e.top else C.R_MAX)) <= 8e-6
            assert torch.isfinite(energy).all() and energy.shape == (B, 1)
            np.testing.assert_allclose(energy.cpu().numpy(), prior.energy(*outs).cpu().numpy(), rtol=3e-6, atol=1e-4)
            seen.append(torch.cat([o[lane] for o in outs] + [energy[lane]]))
        assert all(torch.equal(bits(s), bits(seen[0])) for s in seen)


@pytest.mark.parametrize("low,high", [(0.0, 1.0), (0.0, 2.0), (-4.0, 4.0)])
def test_uniform_priors_at_a_top_word_stay_in_their_support(hip_lib, dev, low, high):
    """the fields ``UniformDistribution(sample_fused=True)`` alone and two of them in a ``ProductDistribution`` hand to the kernel, driven
    through ``philox_sample(..., row0=R)``: ``SloppyUniform.log_prob`` with tol = 0 is finite on every element (its support is closed at
    ``high``), and so is the log_prob of torch's own ``Uniform``, -inf at ``high``: [low, high) is the support of the reference's sampler
    (distributions.py:100-117)"""
    lo_t, hi_t = torch.full((D,), low, device=dev), torch.full((D,), high, device=dev)
    single = bg.UniformDistribution(lo_t, hi_t, tol=0.0, sample_fused=True)
    product = bg.ProductDistribution([bg.UniformDistribution(lo_t, hi_t, tol=0.0), bg.UniformDistribution(lo_t, hi_t, tol=0.0)], sample_fused=True)
    strict = torch.distributions.Uniform(lo_t, hi_t, validate_args=False)
    cases = [([single._philox_field()], "field0"), ([c._philox_field() for c in product._components], "field0"),
             ([c._philox_field() for c in product._components], "field1")]
    for spec, layout in cases:
        assert all(f is not None and f[0] == 0 for f in spec)
        for e in C.select(layout, True):
            for row0, B, lane in C.launches(e, lanes=(0, 63)):
                outs, energy = philox_sample(spec, B, dev, e.seed, e.offset, row0=row0, want_energy=True)
                assert torch.isfinite(energy).all()
                for out in outs:
                    assert torch.isfinite(single.uniform.log_prob(out)).all()
                    assert torch.isfinite(strict.log_prob(out)).all()          # -inf outside [low, high), at `high` too
                assert outs[len(spec) - 1 if layout == "field1" else 0][lane, e.word].item() == np.float32(low) + C.U_MAX * np.float32(high - low)


# ---- bgk_colmap: the sheaf draw of IncreaseMultiplicityFlow ---------------------------------------------------------------------------
def test_colmap_sheaf_draw_at_the_edges(hip_lib, dev):
    """CM_MULT_FWD over 4 columns with the multiplicities 1, 2, 3, 7 in every rotation (so each meets the targeted word), inputs on the
    grid j / 64 in [0, 1) (where (x + sheaf) / m < 1 survives f32 rounding): the output lies in [0, 1), the sheaf y m - x is an integer
    <= m - 1 -- m - 1 at a top word, 0 at a bottom word -- and the launch equals the one that takes the restated uniforms handed in"""
    gen = torch.Generator().manual_seed(5)
    for e in C.select("field0", True) + C.select("field0", False):
        for shift in range(4):
            m = np.roll(np.array([1.0, 2.0, 3.0, 7.0], np.float32), shift)
            table = modulo.ColumnTable(4, [(modulo.MULT_FWD, j, float(v), 0.0) for j, v in enumerate(m)])
            seen = []
            for row0, B, lane in C.launches(e):
                x = (torch.randint(0, 64, (B, 4), generator=gen).float() / 64).to(dev)
                bad = torch.zeros(1, dtype=torch.int32, device=dev)
                y = modulo.colmap_launch(x, table, seed=e.seed, offset=e.offset, row0=row0, bad=bad)
                u = T(philox.sample_field(e.seed, e.offset, 0, B, 4, 0, row0=row0), dev)
                y_fed = modulo.colmap_launch(x, table, u=u)
                assert torch.equal(bits(y), bits(y_fed)) and int(bad.item()) == 0
                assert bool((y >= 0).all()) and bool((y < 1).all())
                sheaf = (y.cpu().numpy().astype(np.float64) * m - x.cpu().numpy())
                assert (np.abs(sheaf - np.round(sheaf)) < 1e-5).all() and (np.round(sheaf) <= m - 1).all() and (np.round(sheaf) >= 0).all()
                assert np.array_equal(np.round(sheaf), np.minimum(np.floor(u.cpu().numpy() * m), m - 1))      # (the f32 product, as in the kernel)
                assert round(sheaf[lane, e.word]) == (m[e.word] - 1 if e.top else 0)
                seen.append(y[lane] * T(m, dev) - x[lane])
            assert all(torch.allclose(s, seen[0], atol=1e-5) for s in seen)


# ---- the chain kernels ------------------------------------------------------------------------------------------------------------------
N, DIM, STEPS = 4, 2, 3
ND = N * DIM


def _chain_case(golden, dev, B, kind="mdw"):
    P = golden("particles")
    energy = make(P, kind, N, DIM).to(dev)
    x0 = torch.tensor(P[f"x_{N}_{DIM}"], device=dev).reshape(-1, ND)[:B].contiguous()
    return energy, _kernel_plan(energy, 1.0), x0


def _numbers(e, row0, B, n_steps, dev, fields=((1, ND), (0, 1))):
    """per step what bgk_philox_fields writes for (seed, offset + s) at rows row0 ..: the normals as the device draws them (f32), the
    uniform fields from the numpy restatement, checked equal to the device's bits"""
    spec = [(kind, d, None, None, 1.0, 0.0) for kind, d in fields]
    per_field = [[] for _ in fields]
    for s in range(n_steps):
        outs, _ = philox_sample(spec, B, dev, e.seed, e.offset + s, row0=row0)
        for f, (kind, d) in enumerate(fields):
            if kind == 0:
                restated = T(philox.sample_field(e.seed, e.offset + s, f, B, d, 0, row0=row0), dev)
                assert torch.equal(bits(restated), bits(outs[f]))
                per_field[f].append(restated[:, 0])
            else:
                per_field[f].append(outs[f])
    return [torch.stack(v) for v in per_field]


def _run_mcmc(plan, x0, e0, temps, std, **kw):
    B = x0.shape[0]
    x, e = x0.clone(), (e0.clone() if e0 is not None else torch.empty(B, device=x0.device))
    traj, traj_e = torch.empty(STEPS, B, ND, device=x0.device), torch.empty(STEPS, B, device=x0.device)
    acc = torch.empty(B, dtype=torch.int32, device=x0.device)
    sampling.pair_mcmc(plan, x, e, e0 is not None, temps, std, STEPS, traj=traj, traj_e=traj_e, traj_every=1, n_accepted=acc, **kw)
    return x, e, traj, traj_e, acc


def _same(a, b):
    return all(torch.equal(bits(s), bits(t)) if s.is_floating_point() else torch.equal(s, t) for s, t in zip(a, b))


def test_replica_exchange_at_equal_temperatures_with_a_top_word(hip_lib, dev, golden):
    """ladders of two replicas at equal temperatures, one step with noise_std = 0 from handed energies (the set-up of
    test_kernel_hand_cases_equal_temperatures_and_nan), in-kernel Philox, the exchange word of the targeted ladder's lower slot a top
    word: c = 0 < -log r for every r < 1, so EVERY ladder exchanges -- the targeted one too, where r = 1.0 refused -- the counter of each
    lower slot says 1, and states, energies, counters and walkers equal the launch with the restated numbers handed in"""
    for e in C.select("exchange", True) + C.select("exchange", False):
        for row0, B, lane in [(e.row - 2 * k, 64, 2 * k) for k in (0, 1, 18, 31)] + [(e.row, 2, 0)]:
            energy, plan, x0 = _chain_case(golden, dev, B)
            e0 = energy.energy(x0)[:, 0].contiguous()
            temps = torch.ones(B, device=dev)
            got = []
            for fed in (False, True):
                x, en = x0.clone(), e0.clone()
                nex, acc = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
                walkers = torch.arange(2, dtype=torch.int32, device=dev).repeat(B // 2)
                kw = dict(seed=e.seed, offset=e.offset, row0=row0)
                if fed:
                    noise, unif, exch = _numbers(e, row0, B, 1, dev, fields=((1, ND), (0, 1), (0, 1)))
                    kw = dict(noise=noise, uniforms=unif, exchange_uniforms=exch)
                    assert exch[0, lane].item() == (C.U_MAX if e.top else C.U_MIN) and bool((exch < 1).all())
                sampling.pair_mcmc(plan, x, en, True, temps, 0.0, 1, n_accepted=acc, n_replicas=2, exchange_every=1, n_exchanged=nex,
                                   walkers=walkers, **kw)
                got.append((x, en, acc, nex, walkers))
                if not fed:                 # the in-kernel draw, judged on its own before the handed-in numbers are formed
                    perm = torch.arange(B, device=dev) ^ 1
                    assert nex[lane].item() == 1 and walkers[lane:lane + 2].tolist() == [1, 0], (e, row0, nex.tolist())
                    assert nex.tolist() == [1, 0] * (B // 2) and walkers.tolist() == [1, 0] * (B // 2)
                    assert torch.equal(bits(x), bits(x0[perm])) and torch.equal(bits(en), bits(e0[perm]))
            assert _same(got[0], got[1])


def test_metropolis_acceptance_at_a_top_word(hip_lib, dev, golden):
    """bgk_pair_mcmc, 3 steps, the first acceptance draw of the targeted chain a top (then a bottom) word: frames, energies, final state
    and accept counts of the in-kernel run have the bits of the run with the same numbers handed in.  At r = 1 - 2^-24, log r = -2^-24:
    a proposal is accepted iff -(e' - e) / T >= -2^-24"""
    for e in C.select("accept", True) + C.select("accept", False):
        for row0, B, lane in C.launches(e, lanes=(0, 37, 63)):
            _, plan, x0 = _chain_case(golden, dev, B)
            temps = torch.tensor([1.0, 2.0], device=dev).repeat((B + 1) // 2)[:B].contiguous()
            noise, unif = _numbers(e, row0, B, STEPS, dev)
            assert unif[0, lane].item() == (C.U_MAX if e.top else C.U_MIN) and bool((unif < 1).all()) and bool((unif > 0).all())
            drawn = _run_mcmc(plan, x0, None, temps, 0.3, seed=e.seed, offset=e.offset, row0=row0)
            fed = _run_mcmc(plan, x0, None, temps, 0.3, noise=noise, uniforms=unif)
            assert _same(drawn, fed)
            assert all(bool(torch.isfinite(t).all()) for t in drawn[:4])
            if B > 1:
                assert 0 < int(drawn[4].sum()) < STEPS * B                        # (chains that move and reject)


def test_hmc_acceptance_at_a_top_word(hip_lib, dev, golden):
    """bgk_pair_hmc (5 leapfrog steps of 0.15), as test_metropolis_acceptance_at_a_top_word"""
    for e in C.select("accept", True) + C.select("accept", False):
        for row0, B, lane in C.launches(e, lanes=(0, 37, 63)):
            _, plan, x0 = _chain_case(golden, dev, B)
            temps = torch.tensor([1.0, 2.0], device=dev).repeat((B + 1) // 2)[:B].contiguous()
            noise, unif = _numbers(e, row0, B, STEPS, dev)
            assert unif[0, lane].item() == (C.U_MAX if e.top else C.U_MIN)
            got = []
            for kw in (dict(seed=e.seed, offset=e.offset, row0=row0), dict(noise=noise, uniforms=unif)):
                x, en = x0.clone(), torch.empty(B, device=dev)
                traj, traj_e = torch.empty(STEPS, B, ND, device=dev), torch.empty(STEPS, B, device=dev)
                acc = torch.empty(B, dtype=torch.int32, device=dev)
                sampling.pair_hmc(plan, x, en, False, temps, 0.15, 5, 1.0, STEPS, traj=traj, traj_e=traj_e, traj_every=1, n_accepted=acc, **kw)
                got.append((x, en, traj, traj_e, acc))
            assert _same(*got)
            assert all(bool(torch.isfinite(t).all()) for t in got[0][:4])
            if B > 1:
                assert 0 < int(got[0][4].sum())


def test_anneal_acceptance_at_a_top_word(hip_lib, dev, golden):
    """bgk_pair_anneal from Lennard-Jones to the multi-double-well over 3 stages of one step, as
    test_metropolis_acceptance_at_a_top_word: final state, both ends' energies, the work (f64) and the accept counts bit for bit"""
    schedule = annealing.anneal_coefficients([0.0, 0.3, 0.7, 1.0]).to(dev).contiguous()
    for e in C.select("accept", True) + C.select("accept", False):
        for row0, B, lane in C.launches(e, lanes=(0, 37, 63)):
            _, plan_b, x0 = _chain_case(golden, dev, B)
            _, plan_a, _ = _chain_case(golden, dev, B, kind="lj")
            noise, unif = _numbers(e, row0, B, STEPS, dev)
            assert unif[0, lane].item() == (C.U_MAX if e.top else C.U_MIN)
            got = []
            for kw in (dict(seed=e.seed, offset=e.offset, row0=row0), dict(noise=noise, uniforms=unif)):
                x, e_a, e_b = x0.clone(), torch.empty(B, device=dev), torch.empty(B, device=dev)
                work, acc = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
                annealing.pair_anneal(plan_a, plan_b, x, schedule, 1, 0, STEPS, 0.15, e_a, e_b, False, work, n_accepted=acc, **kw)
                got.append((x, e_a, e_b, acc, work))
            assert all(torch.equal(s, t) for s, t in zip(got[0], got[1]))
            assert all(bool(torch.isfinite(t).all()) for t in got[0])
            if B > 1:
                assert 0 < int(got[0][3].sum())


def test_chain_proposals_at_the_largest_radius(hip_lib, dev, golden):
    """bgk_pair_mcmc / _hmc / _anneal with a bottom word as the u1 of a proposal's (momentum's) Box-Muller pair at the first step -- the
    radius 5.887 -- and a top word there and as u2: finite, and the bits of the run with the same numbers handed in (the bound of the
    *_in_kernel_philox_equals_the_same_numbers_handed_in tests).  The handed-in normals are what bgk_philox_fields writes, themselves
    within the probe's bound of the f64 restatement (test_normal_fields_and_their_energy_at_the_edges)."""
    schedule = annealing.anneal_coefficients([0.0, 0.3, 0.7, 1.0]).to(dev).contiguous()
    for e in C.select("field0", False, 0) + C.select("field0", True):
        for row0, B, lane in C.launches(e, lanes=(0, 63)):
            _, plan, x0 = _chain_case(golden, dev, B)
            _, plan_lj, _ = _chain_case(golden, dev, B, kind="lj")
            noise, unif = _numbers(e, row0, B, STEPS, dev)
            if not e.top:
                assert abs(float(torch.linalg.vector_norm(noise[0, lane, e.word:e.word + 2].double())) - C.R_MAX) <= 8e-6
            assert bool(torch.isfinite(noise).all())
            stream, fed = dict(seed=e.seed, offset=e.offset, row0=row0), dict(noise=noise, uniforms=unif)
            runs = [_run_mcmc(plan, x0, None, 1.5, 0.3, **kw) for kw in (stream, fed)]
            assert _same(*runs) and all(bool(torch.isfinite(t).all()) for t in runs[0][:4])
            got = []
            for kw in (stream, fed):
                x, en = x0.clone(), torch.empty(B, device=dev)
                acc = torch.empty(B, dtype=torch.int32, device=dev)
                sampling.pair_hmc(plan, x, en, False, 1.5, 0.15, 5, 1.0, STEPS, n_accepted=acc, **kw)
                got.append((x, en, acc))
            assert _same(*got) and all(bool(torch.isfinite(t).all()) for t in got[0][:2])
            got = []
            for kw in (stream, fed):
                x, e_a, e_b = x0.clone(), torch.empty(B, device=dev), torch.empty(B, device=dev)
                work, acc = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
                annealing.pair_anneal(plan_lj, plan, x, schedule, 1, 0, STEPS, 0.15, e_a, e_b, False, work, n_accepted=acc, **kw)
                got.append((x, e_a, e_b, acc, work))
            assert all(torch.equal(s, t) for s, t in zip(*got)) and all(bool(torch.isfinite(t).all()) for t in got[0])


@pytest.mark.parametrize("layer", ["brownian", "langevin"])
def test_langevin_noise_at_the_largest_radius(hip_lib, dev, golden, layer):
    """bgk_pair_langevin, 2 steps, with a bottom word as the u1 of a Box-Muller pair of w / w1 (field 0) or, for Langevin, of w2 (field 1)
    at the first step, and the top words of those fields: q, v and dW finite, and the bits of the run with the same normals handed in
    (test_gpu_stochastic.py's in-kernel test asks the same bits)"""
    from stochastic_common import case_key
    h = float(golden("stochastic")[case_key(layer, "mdw", N, DIM, 12) + "stepsize"])
    mass, gamma, kT = (1.3, 0.7, 1.2) if layer == "langevin" else (1.0, 0.0, 1.0)        # (Brownian: what BrownianFlow passes)
    n_steps = 2
    layouts = ("field0", "field1") if layer == "langevin" else ("field0",)
    for e in [s for l in layouts for s in C.select(l, False, 0) + C.select(l, True)]:
        for row0, B, lane in C.launches(e, lanes=(0, 63)):
            _, plan, x0 = _chain_case(golden, dev, B)
            v0 = torch.zeros_like(x0) if layer == "langevin" else None
            w1, w2 = _numbers(e, row0, B, n_steps, dev, fields=((1, ND), (1, ND)))
            hit = (w1 if e.layout == "field0" else w2)[0, lane, e.word & ~1:(e.word & ~1) + 2].double()
            if e.word % 2 == 0:
                radius = float(torch.linalg.vector_norm(hit))
                assert abs(radius - (np.sqrt(-2 * np.log1p(-2.0 ** -24)) if e.top else C.R_MAX)) <= 8e-6
            got = []
            for kw in (dict(seed=e.seed, offset=e.offset, row0=row0), dict(w1=w1, w2=w2 if layer == "langevin" else None)):
                q, v, dW = x0.clone(), (None if v0 is None else v0.clone()), torch.empty(B, device=dev)
                stochastic.pair_langevin(plan, q, v, h, mass, gamma, kT, n_steps, dW, **kw)
                got.append((q, dW) if v is None else (q, v, dW))
            assert _same(*got) and all(bool(torch.isfinite(t).all()) for t in got[0])
            assert float((got[0][0] - x0).abs().max()) > 1e-3
