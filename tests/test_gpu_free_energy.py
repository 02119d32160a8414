"""On the GPU: the kernel path of bgflow_amd.free_energy (csrc/bgk_bar.hip) against tests/golden/free_energy.npz and against the torch
path on the same device -- the loads (unaligned slice, ragged sizes), the block partition (many blocks against one, 2^20 values), NaN and
infinity, determinism, the stream, the public function.  Bounds: free_energy_common.py."""
import math

import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import free_energy as fe

from free_energy_common import check_record, delta_bound, uncertainty_bound, works

pytestmark = pytest.mark.gpu

CASES = ["pos", "neg", "far", "scales", "ragged", "tiny", "single", "expand_a", "expand_b", "nooverlap"]


def synthetic(nf, nr, seed, dev, dtype=torch.float32):
    """work values as the fixture's, from a seeded CPU generator: shift 0.5, offset 1.5"""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(nf, generator=g, dtype=torch.float64)
    x2 = 0.5 + torch.randn(nr, generator=g, dtype=torch.float64)
    wf = (1.5 + 0.5 * (x1 - 0.5) ** 2) - 0.5 * x1 ** 2
    wr = 0.5 * x2 ** 2 - (1.5 + 0.5 * (x2 - 0.5) ** 2)
    return wf.to(dtype).to(dev), wr.to(dtype).to(dev)


@pytest.fixture(scope="module")
def large(dev):
    """2^20 + 3 / 2^19 + 1 f32 work values, the torch path's record on them (f64 ops on the device) and the kernel's"""
    wf, wr = synthetic(2 ** 20 + 3, 2 ** 19 + 1, 7, dev)
    return wf, wr, bg.bar_solve(wf, wr, path="torch"), bg.bar_solve(wf, wr, path="kernel")


def agree(k, t, nf, nr, label):
    """kernel record against the torch path's on the same data"""
    dk, dt, uk, ut = float(k.delta_f), float(t.delta_f), float(k.uncertainty), float(t.uncertainty)
    print(f"{label}: kernel {dk:.16g} torch {dt:.16g} (diff {abs(dk - dt):.2e})  unc {uk:.12g} / {ut:.12g}  residual {float(k.residual):.2e}  "
          f"evaluations {k.n_evaluations} / {t.n_evaluations}  read-backs {k.n_readbacks} / {t.n_readbacks}")
    assert k.status == t.status == fe.CONVERGED
    assert abs(dk - dt) <= delta_bound(dt)
    assert abs(uk - ut) <= uncertainty_bound(ut, nf, nr)
    assert abs(float(k.residual)) <= 1e-9
    assert abs(k.n_evaluations - t.n_evaluations) <= 2 and k.n_evaluations <= 100


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", CASES)
def test_kernel_path_meets_the_fixture(golden, dev, case, dtype):
    G = golden("free_energy")
    wf, wr = works(G, case, dtype, dev)
    r = bg.bar_solve(wf, wr, path="kernel")
    check_record(G, case, r, label=f"kernel {dtype} ")
    assert r.delta_f.device == wf.device and r.uncertainty.device == wf.device and r.residual.device == wf.device
    t = bg.bar_solve(wf, wr, path="torch")
    assert abs(r.n_evaluations - t.n_evaluations) <= 2 and r.status == t.status
    auto = bg.bar_solve(wf, wr)                                       # path=None takes the kernel: one read-back per chunk
    assert auto.n_readbacks == r.n_readbacks < t.n_readbacks
    assert auto.delta_f.equal(r.delta_f) or case == "nooverlap"


def test_unaligned_slice(golden, dev):
    """an f32 slice w[1:] starts 4 bytes past a 16-byte boundary: scalar head, then 16-byte loads"""
    G = golden("free_energy")
    wf, wr = works(G, "pos", torch.float32, dev)
    pad_f, pad_r = torch.cat([wf[:1], wf]), torch.cat([wr[:3], wr])
    sf, sr = pad_f[1:], pad_r[3:]
    assert sf.data_ptr() % 16 == 4 and sr.data_ptr() % 16 == 12 and sf.is_contiguous()
    r = bg.bar_solve(sf, sr, path="kernel")
    check_record(G, "pos", r, label="w[1:] ")
    # every element counted once: one value fewer on each side is another problem with another answer
    short = bg.bar_solve(sf[:-1], sr[1:], path="kernel")
    t = bg.bar_solve(sf[:-1], sr[1:], path="torch")
    agree(short, t, sf.numel() - 1, sr.numel() - 1, "w[1:-1]")
    assert not short.delta_f.equal(r.delta_f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_many_blocks_against_one(dev, dtype):
    wf, wr = synthetic(70001, 33, 11, dev, dtype)
    assert fe._blocks(70001) == 18 and fe._blocks(33) == 1
    agree(bg.bar_solve(wf, wr, path="kernel"), bg.bar_solve(wf, wr, path="torch"), 70001, 33, f"70001 / 33 {dtype}")
    agree(bg.bar_solve(wr, wf, path="kernel"), bg.bar_solve(wr, wf, path="torch"), 33, 70001, f"33 / 70001 {dtype}")


def test_large_arrays_fill_the_block_cap(large):
    wf, wr, t, k = large
    assert fe._blocks(wf.numel()) == 257 and fe._blocks(2 ** 22) == fe.MAX_BLOCKS == 512
    agree(k, t, wf.numel(), wr.numel(), "2^20 + 3 / 2^19 + 1")


def test_deterministic_and_independent_of_the_chunk(large):
    wf, wr, _, k = large
    again = bg.bar_solve(wf, wr, path="kernel")
    for a, b in zip(k[:3], again[:3]):
        assert a.equal(b)                                             # bit-identical f64
    assert k[3:] == again[3:]
    flat_f, flat_r = wf.reshape(-1), wr.reshape(-1)
    for chunk in (1, 5):
        other = fe._bar_kernel(flat_f, flat_r, 500, 1e-12, chunk=chunk)
        assert all(a.equal(b) for a, b in zip(k[:3], other[:3])) and k[3:7] == other[3:7]
        assert other.n_readbacks >= k.n_readbacks
    assert fe.BAR_CHUNK == 16 and k.n_readbacks == -(-(k.n_evaluations + 1) // 16)


def test_nan_and_infinity(golden, dev):
    G = golden("free_energy")
    wf, wr = works(G, "pos", torch.float32, dev)
    planted = wf.clone()
    planted[-1] = float("nan")
    for a, b, label in ((planted, wr, "NaN in the last forward value"), (wf, torch.full_like(wr, float("inf")), "all reverse +inf"),
                        (torch.full_like(wf, float("-inf")), wr, "all forward -inf")):
        r = bg.bar_solve(a, b, path="kernel")
        t = bg.bar_solve(a, b, path="torch")
        print(label, r, t)
        assert math.isnan(float(r.delta_f)) and math.isnan(float(r.uncertainty)) and r.status in (fe.NO_ROOT, fe.NOT_A_NUMBER)
        assert r.status == t.status and r.n_evaluations == t.n_evaluations <= 100
        d, u = bg.bennett_acceptance_ratio(a, b)
        assert math.isnan(float(d)) and math.isnan(float(u))
    # one infinite value among finite ones is a sample of weight zero (+inf) in the sums, not a NaN
    one = wf.clone()
    one[5] = float("inf")
    agree(bg.bar_solve(one, wr, path="kernel"), bg.bar_solve(one, wr, path="torch"), wf.numel(), wr.numel(), "one +inf forward value")


def test_stream(golden, dev):
    G = golden("free_energy")
    wf, wr = works(G, "ragged", torch.float32, dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = bg.bar_solve(wf, wr, path="kernel")                      # enqueued on the current stream: `side`
        after = r.delta_f + 1.0                                      # the stream stays usable
    assert torch.cuda.default_stream(dev).query()                    # nothing went to another stream
    side.synchronize()
    torch.cuda.synchronize()
    check_record(G, "ragged", r, label="side stream ")
    assert float(after) == float(r.delta_f) + 1.0
    main = bg.bar_solve(wf, wr, path="kernel")
    torch.cuda.synchronize()
    assert main.delta_f.equal(r.delta_f)


def test_public_function_on_hip_tensors(golden, dev):
    G = golden("free_energy")
    for case in ("pos", "neg", "scales"):
        wf, wr = works(G, case, torch.float32, dev)
        d, u = bg.bennett_acceptance_ratio(wf[:, None], wr[:, None])
        d64, u64 = float(G[f"{case}_delta64"]), float(G[f"{case}_unc64"])
        assert d.dtype == torch.float32 and u.dtype == torch.float32 and d.dim() == 0 and u.dim() == 0 and d.device == wf.device == u.device
        assert abs(float(d) - d64) <= 2.0 ** -23 * abs(d64) + 1e-10
        assert abs(float(u) - u64) <= 2.0 ** -23 * u64 + uncertainty_bound(u64, wf.numel(), wr.numel())
    d, u = bg.bennett_acceptance_ratio(wf, wr, compute_uncertainty=False)
    assert u is None
    grad = wf.clone().requires_grad_(True)
    assert bg.bar_solve(grad, wr).n_readbacks > 3 and bg.bar_solve(grad, wr).delta_f.grad_fn is not None      # the torch path
    with pytest.raises(ValueError):
        bg.bar_solve(grad, wr, path="kernel")
    with pytest.raises(ValueError):
        bg.bar_solve(wf, wr.double(), path="kernel")
    with pytest.raises(ValueError):
        bg.bar_solve(wf, wr.cpu())
    with torch.no_grad():
        assert bg.bar_solve(grad, wr).n_readbacks == bg.bar_solve(wf, wr).n_readbacks       # grad disabled: the kernel
