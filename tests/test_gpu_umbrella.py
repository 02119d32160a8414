"""On the GPU: the kernel path of bgflow_amd.umbrella (csrc/bgk_mbar.hip) against the BFGS values of tests/golden/umbrella.npz and against
the torch path on the same device -- the window counts at which the kernel takes another route (one window, fewer windows than waves, more
windows than waves, the envelope's edge and one beyond it), the loads (unaligned slice, head and tail), the block partition, determinism,
the stream, the log-weight entry, the argument checks -- and ``UmbrellaSampling.for_box`` on the fused chain kernel.  Bounds:
umbrella_common.py."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib, umbrella
from bgflow_amd.distributions import BoxPlan, _kernel_plan

import umbrella_common as uc
from box_common import err_u, make

pytestmark = pytest.mark.gpu

KERNEL_CASES = ["k1", "k2", "k5", "k64", "k256"]


def table_of(case, dev, counts=None):
    counts_, centres, k = uc.B_CASES[case]
    return umbrella._window_table(counts_ if counts is None else counts, centres, np.full(len(counts_), k), 1.0, dev)


def pooled(G, case, dtype, dev):
    return torch.cat(uc.b_tensors(G, case, dtype, dev))


def kernel(rc, table, **kw):
    return umbrella._mbar_kernel(rc, table, 10000, uc.B_TOLERANCE, **kw)


def synthetic(dev, dtype=torch.float32):
    """70001 samples in 5 unequal windows (the geometry of the fixture's k5), from a seeded CPU generator: 69 blocks of one tile by
    default, 10-tile slices with a ragged last tile at 7 blocks, 69 tiles in one block"""
    counts, centres, k = (20001, 9000, 17000, 4000, 20000), uc.B_CASES["k5"][1], 1.0
    g = torch.Generator().manual_seed(5)
    sd = (0.5 / (0.5 + k)) ** 0.5
    rc = torch.cat([k * float(c) / (0.5 + k) + sd * torch.randn(n, generator=g, dtype=torch.float64) for c, n in zip(centres, counts)])
    return rc.to(dtype).to(dev), umbrella._window_table(counts, centres, np.full(5, k), 1.0, dev)


@pytest.fixture(scope="module")
def large(dev):
    rc, table = synthetic(dev)
    return rc, table, umbrella._mbar_torch(rc, table, 10000, uc.B_TOLERANCE), kernel(rc, table)


# ---- the solver ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_kernel_path_meets_bfgs_and_the_torch_path(golden, dev, case, dtype):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES[case]
    trajs = uc.b_tensors(G, case, dtype, dev)
    r = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE, path="kernel")
    assert r.f.device == trajs[0].device and r.log_weights.device == trajs[0].device and r.f.dtype == torch.float64
    uc.check_case(G, case, r, f"kernel {dtype} ")
    t = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE, path="torch")
    df, dw = float((r.f - t.f).abs().max()), float((r.log_weights - t.log_weights).abs().max())
    print(f"  against the torch path: |df| {df:.2e} (bound {uc.path_bound(G, case):.2e}), |d log w| {dw:.2e}, iterations {r.iterations} / {t.iterations}")
    assert t.status == r.status == umbrella.CONVERGED and abs(r.iterations - t.iterations) <= 1
    assert df <= uc.path_bound(G, case)
    assert dw <= uc.path_bound(G, case) + uc.log_weight_bound(len(counts), t.log_weights.cpu().numpy())      # |d(-D)/df| <= 1
    auto = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE)              # path=None takes the kernel
    assert auto.f.equal(r.f) and auto.log_weights.equal(r.log_weights) and auto[2:] == r[2:]
    if case == "k1":
        rc = trajs[0].double()
        assert r.iterations == 1 and float(r.f[0]) == 0.0
        assert float((r.log_weights + (np.log(37.0) - k * (rc - float(centres[0])) ** 2)).abs().max()) <= 1e-14


def test_one_window_beyond_the_envelope_takes_the_torch_path(golden, dev, hip_lib):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES["k257"]
    trajs = uc.b_tensors(G, "k257", torch.float32, dev)
    assert not umbrella._kernel_eligible(trajs) and umbrella._kernel_eligible(trajs[:256]) and umbrella.MAX_WINDOWS == 256
    r = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE)
    uc.check_case(G, "k257", r, "torch on the device ")
    assert r.f.device == trajs[0].device
    with pytest.raises(ValueError, match="kernel path"):
        bg.mbar_solve(trajs, centres, k, path="kernel")
    rc, table = torch.cat(trajs), table_of("k257", dev)
    scratch = torch.zeros(257 + 8 + 257, dtype=torch.float64, device=dev)
    st = hip_lib.bgk_mbar_solve_steps(_lib.ptr(rc), rc.numel(), 0, _lib.ptr(table), 257, 1, _lib.ptr(scratch[265:]), _lib.ptr(scratch[:257]),
                                      _lib.ptr(scratch[257:265]), 100, 1e-10, 1, None)
    assert st == -2 and b"envelope" in hip_lib.bgk_last_error()
    torch.cuda.synchronize()
    assert float(scratch.abs().max()) == 0.0                          # nothing was launched


def test_argument_checks_of_the_entries(hip_lib, dev):
    uc.check_entry_arguments(hip_lib)


def test_unaligned_slice(golden, dev):
    """an f32 slice rc[1:] starts 4 bytes past a 16-byte boundary: scalar head, then 16-byte loads, then a tail"""
    G = golden("umbrella")
    rc, table = pooled(G, "k5", torch.float32, dev), table_of("k5", dev)
    pad = torch.cat([rc[:1], rc])
    s = pad[1:]
    assert s.data_ptr() % 16 == 4 and rc.data_ptr() % 16 == 0 and s.is_contiguous()
    a, b = kernel(rc, table), kernel(s, table)
    assert float((a.f - b.f).abs().max()) <= uc.path_bound(G, "k5") and abs(a.iterations - b.iterations) <= 1
    uc.check_case(G, "k5", b, "rc[1:] ")
    assert float((a.log_weights - b.log_weights).abs().max()) <= uc.path_bound(G, "k5") + uc.log_weight_bound(5, a.log_weights.cpu().numpy())
    # every element is counted once: one sample fewer at either end is another problem with another answer
    for cut, counts in ((s[:-1], (257, 300, 129, 64, 249)), (s[1:], (256, 300, 129, 64, 250))):
        tb = table_of("k5", dev, counts)
        k_, t_ = kernel(cut, tb), umbrella._mbar_torch(cut, tb, 10000, uc.B_TOLERANCE)
        assert float((k_.f - t_.f).abs().max()) <= uc.path_bound(G, "k5") and abs(k_.iterations - t_.iterations) <= 1
        assert float((k_.f - a.f).abs().max()) > 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_block_counts(golden, dev, dtype):
    """n_blocks = 1 against 7 against 512: only the order of the f64 sums differs.  1000 samples in 512 blocks: slices of 4, most
    blocks empty"""
    G = golden("umbrella")
    rc, table = pooled(G, "k5", dtype, dev), table_of("k5", dev)
    assert umbrella._blocks(1000) == 1 and umbrella._blocks(1025) == 2 and umbrella._blocks(2 ** 20) == umbrella.MAX_BLOCKS == 512
    runs = [kernel(rc, table, n_blocks=nb) for nb in (1, 7, 512)]
    for r in runs[1:]:
        assert float((r.f - runs[0].f).abs().max()) <= 1e-12 and abs(r.iterations - runs[0].iterations) <= 1 and r.status == umbrella.CONVERGED
        assert float((r.log_weights - runs[0].log_weights).abs().max()) <= 1e-12
    uc.check_case(G, "k5", runs[2], f"512 blocks {dtype} ")


def test_many_tiles_and_many_blocks(large):
    rc, table, t, k = large
    assert umbrella._blocks(rc.numel()) == 69
    print(f"70001 samples: kernel {k.f.tolist()} in {k.iterations} iterations, torch {t.iterations}; |df| {float((k.f - t.f).abs().max()):.2e}")
    assert k.status == t.status == umbrella.CONVERGED and abs(k.iterations - t.iterations) <= 1
    bound = 2 * uc.B_TOLERANCE / (1 - uc.B_TOLERANCE ** (1.0 / max(2, t.iterations))) + 1e-13        # umbrella_common.path_bound
    assert float((k.f - t.f).abs().max()) <= bound
    assert float((k.log_weights - t.log_weights).abs().max()) <= bound + uc.log_weight_bound(5, t.log_weights.cpu().numpy())
    for nb in (1, 7, 512):
        other = kernel(rc, table, n_blocks=nb)
        assert float((other.f - k.f).abs().max()) <= 1e-12 and abs(other.iterations - k.iterations) <= 1
    d = kernel(rc.double(), table)                                     # the exact widening: the same numbers through the f64 loads
    assert float((d.f - k.f).abs().max()) <= 1e-12 and abs(d.iterations - k.iterations) <= 1


def test_deterministic_and_independent_of_the_chunk(large):
    rc, table, _, k = large
    again = kernel(rc, table)
    assert again.f.equal(k.f) and again.log_weights.equal(k.log_weights) and again[2:] == k[2:]           # bit-identical f64
    for chunk in (1, 5):
        other = kernel(rc, table, chunk=chunk)
        assert other.f.equal(k.f) and other[2:] == k[2:]
    assert umbrella.MBAR_CHUNK == 32


def test_start_vector_budget_and_nan(golden, dev):
    G = golden("umbrella")
    rc, table = pooled(G, "k5", torch.float32, dev), table_of("k5", dev)
    full = kernel(rc, table)
    warm = kernel(rc, table, f0=full.f)                                # a start vector: at the fixed point one iteration suffices
    assert warm.status == umbrella.CONVERGED and warm.iterations <= 2 and float((warm.f - full.f).abs().max()) <= uc.path_bound(G, "k5")
    counts, centres, k = uc.B_CASES["k5"]
    trajs = uc.b_tensors(G, "k5", torch.float32, dev)
    short = bg.mbar_solve(trajs, centres, k, maximum_iterations=3, tolerance=uc.B_TOLERANCE)
    ref = bg.mbar_solve(trajs, centres, k, maximum_iterations=3, tolerance=uc.B_TOLERANCE, path="torch")
    assert short.status == ref.status == umbrella.BUDGET and short.iterations == ref.iterations == 3
    assert float((short.f - ref.f).abs().max()) <= 1e-13 and abs(short.err - ref.err) <= 1e-13 and short.err > uc.B_TOLERANCE
    for value in (float("nan"), float("inf")):
        planted = [t.clone() for t in trajs]
        planted[3][-1] = value
        bad = bg.mbar_solve(planted, centres, k)
        assert bad.status == umbrella.NOT_A_NUMBER and bad.iterations == 1 and bad.err != bad.err and bool(torch.isnan(bad.f).any())
        assert bg.mbar_solve(planted, centres, k, path="torch").status == umbrella.NOT_A_NUMBER


def test_log_weight_entry(golden, dev, hip_lib):
    """bgk_mbar_log_weights against -D_n of the torch ops at the SAME f, f32 and f64 input, an unaligned start"""
    G = golden("umbrella")
    for case in ("k5", "k256"):
        K = len(uc.B_CASES[case][0])
        table = table_of(case, dev)
        f = torch.from_numpy(G[f"{case}_f"]).to(dev)
        want = torch.from_numpy(uc.b_log_weights(G, case, G[f"{case}_f"])).to(dev)
        for dtype in (torch.float32, torch.float64):
            rc = pooled(G, case, dtype, dev)
            for src in (rc, torch.cat([rc[:1], rc])[1:]):
                out = torch.full((rc.numel() + 2,), 7.0, dtype=torch.float64, device=dev)
                st = hip_lib.bgk_mbar_log_weights(_lib.ptr(src), src.numel(), umbrella._DTYPE_CODES[dtype], _lib.ptr(table), K, _lib.ptr(f),
                                                  _lib.ptr(out[1:]), _lib.stream_ptr(dev))
                _lib.check(st, "bgk_mbar_log_weights")
                assert float(out[0]) == 7.0 and float(out[-1]) == 7.0                  # nothing written outside [n]
                assert float((out[1:-1] - want).abs().max()) <= uc.log_weight_bound(K, want.cpu().numpy())
        t = -umbrella._log_denominators(rc, table[:, 2] + f, table[:, 1], table[:, 0])
        assert float((t - want).abs().max()) <= uc.log_weight_bound(K, want.cpu().numpy())


def test_stream(golden, dev):
    G = golden("umbrella")
    counts, centres, k = uc.B_CASES["k64"]
    trajs = uc.b_tensors(G, "k64", torch.float32, dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE)   # enqueued on the current stream: `side`
        after = r.f + 1.0                                               # the stream stays usable
    assert torch.cuda.default_stream(dev).query()                       # nothing went to another stream
    side.synchronize()
    torch.cuda.synchronize()
    uc.check_case(G, "k64", r, "side stream ")
    assert after.equal(r.f + 1.0)
    main = bg.mbar_solve(trajs, centres, k, tolerance=uc.B_TOLERANCE)
    torch.cuda.synchronize()
    assert main.f.equal(r.f) and main.log_weights.equal(r.log_weights)


# ---- the box -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rep", "harm"])
def test_biased_energy_on_the_kernel_path(golden, dev, kind):
    """``biased_system(...)`` is a box the pair kernel takes: its f32 energies against the torch formulas in f64 plus the umbrella, at the
    bound the box parity test (test_gpu_box.py) allows for the unbiased energy: four times the reference's own f32 error + 1e-6"""
    G = golden("box")
    system = make(G, kind, 2)
    k, m = 50.0, 1.2
    biased = bg.biased_system(system, k, m).to(dev)
    assert isinstance(_kernel_plan(biased, 1.0), BoxPlan)
    x = torch.tensor(G["x_2"], device=dev)
    u = biased.energy(x).cpu().numpy().reshape(-1)
    x64 = torch.tensor(G["x_2"], dtype=torch.float64)
    d = system.dimer_distance(x64)
    want = (system._energy(x64).reshape(-1) + k * (d - m) ** 2 - k * (system.params["dimer_dmid"] - m) ** 2).numpy()
    e, ref = err_u(u, want), float(G[f"{kind}_2_err_u32"])
    print(f"{kind}: biased energy error {e:.3g} (bound {4 * ref + 1e-6:.3g})")
    assert e <= 4 * ref + 1e-6


def test_for_box(golden, dev):
    """64 walkers, 3 umbrellas at m = 1.0, 1.5, 2.0 with k = 50, 200 recorded steps each, on the fused chain kernel.  The same classes on
    CPU tensors (torch ops; seeds 0, 1, 2 of torch.manual_seed) gave window means 0.982 .. 0.987, 1.309 .. 1.340, 2.020 .. 2.023: gaps
    of 0.32 .. 0.36 and 0.68 .. 0.71, i.e. more than 10 standard errors of the least certain mean (0.028 .. 0.031 for the middle
    window, whose umbrella leaves the dimer bistable -- within-window standard deviation 0.33 against 0.12 .. 0.15 for the others; the
    standard error is the spread of the 64 walker means / 8)."""
    G = golden("box")
    system = make(G, "rep", 2).to(dev)
    x0 = torch.tensor(G["x_2"][:64], device=dev)
    us = bg.UmbrellaSampling.for_box(system, x0, 3, 50.0, 1.0, 2.0, forward_backward=False)
    assert [u.m_umbrella for u in us.umbrellas] == [1.0, 1.5, 2.0]
    assert bg.GaussianMCMCSampler(bg.biased_system(system, 50.0, 1.5), x0.clone(), noise_std=0.1)._fused_setup() is not None      # the chain kernel
    torch.manual_seed(0)
    us.run(200, verbose=False)
    trajs = us.rc_trajs
    assert all(t.shape == (64 * 200,) and t.device == x0.device and t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in trajs)
    means = [float(t.mean()) for t in trajs]
    print(f"for_box: window means {means}")
    assert means[0] < means[1] < means[2]
    assert umbrella._kernel_eligible(trajs)
    xg, F = us.mbar(rc_bins=20)
    w = us.mbar_weights()
    solved = us._solve()
    assert solved.status == umbrella.CONVERGED and solved.f.is_cuda
    states = torch.bucketize(torch.cat(trajs).double(), torch.from_numpy(np.linspace(float(torch.cat(trajs).min()), float(torch.cat(trajs).max()), 20)).to(dev),
                             right=True).cpu().numpy()
    occupied = np.bincount(states, minlength=21) > 0
    assert xg.shape == (21,) and F.shape == (21,) and np.isfinite(F[occupied]).all() and np.isposinf(F[~occupied]).all() and occupied.sum() >= 10
    assert len(w) == 3 and all(v.dtype == torch.float32 and v.device == x0.device and v.shape == t.shape for v, t in zip(w, trajs))
    assert abs(float(torch.cat(w).double().sum()) - 1.0) <= 1e-4 and bool((torch.cat(w) >= 0).all())
    centres, Es = bg.free_energy_bootstrap(torch.cat(trajs), 0.8, 2.2, 8, sample=4, weights=torch.cat(w), seed=3)
    assert Es.shape == (4, 7) and Es.is_cuda and bool(torch.isfinite(Es).all())
