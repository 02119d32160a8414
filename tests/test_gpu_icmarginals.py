"""GPU (-m gpu): the column-moments kernel (bgk_column_moments_update / _finalize, csrc/bgk_moments.hip) against a two-pass f64
computation, and InternalCoordinateMarginals.inform_with_data on it against the reference's golden vectors
(tests/golden/g_icmarginals.npz, written by tests/golden/make_icmarginal_goldens.py from the unmodified reference).

Bounds.  Kernel: min / max equal in bits; mean 1e-12 relative; std 1e-9 relative -- the error of the shifted f64 sums is bounded by
N 2^-53 (1 + (mu - K)^2 / sigma^2), and with K a sample of the column the bracket is below 30 for the columns used here.
End to end and built flow: 4 x the reference's own f32-vs-f64 deviation recorded in the fixture (dev_*), for the statistics with a
floor of 4 f32 ulp of the value: the GPU IC kernel and the reference's f32 chain are two independent f32 roundings of the same
quantity, and the f64 statistics add nothing."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import BONDS, ANGLES, TORSIONS, InternalCoordinateMarginals, configs

pytestmark = pytest.mark.gpu

FIELDS = (("bonds", BONDS), ("angles", ANGLES), ("torsions", TORSIONS))
KINDS = ("uniform", "0.1 + 0.003 z", "1000 + 0.001 z", "constant", "one NaN")
PAD, OFFSET = 7, 3


def _columns(B, P):
    """[B, P] f32 test matrix, the kind of each column, and its two-pass f64 statistics"""
    g = np.random.default_rng(1000 * P + B)
    kinds = [(j + (2 if P == 1 else 0)) % 5 for j in range(P)]
    x = np.empty((B, P), np.float32)
    for j, k in enumerate(kinds):
        z = g.standard_normal(B)
        x[:, j] = (g.random(B), 0.1 + 0.003 * z, 1000 + 0.001 * z, np.full(B, 0.3 + j), g.random(B))[k]
        if k == 4:
            x[B // 2, j] = np.nan
    x64 = x.astype(np.float64)
    mean = x64.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((x64 - mean) ** 2).sum(0) / (B - 1)) if B > 1 else np.full(P, np.nan)
    return x, np.array(kinds), mean, std, x64.min(0), x64.max(0)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check(r, B, kinds, mean, std, lo, hi, what):
    got = [v.cpu().numpy() for v in r]
    ok = kinds != 4
    assert np.array_equal(got[0], np.full(len(kinds), float(B))), what
    assert np.array_equal(got[3][ok], lo[ok]) and np.array_equal(got[4][ok], hi[ok]), f"{what}: min / max"
    e_mean = np.abs(got[1][ok] - mean[ok]) / np.abs(mean[ok])
    assert e_mean.max(initial=0) <= 1e-12, f"{what}: mean, relative error {e_mean.max():.2e}"
    if B == 1:
        assert np.isnan(got[2]).all(), f"{what}: std of one row is NaN"
    else:
        const = (kinds == 3) | (std == 0)           # (two rows of 1000 + 0.001 z can round to the same f32)
        assert (got[2][const] == 0.0).all(), f"{what}: a constant column has std exactly 0"
        v = ok & ~const
        e_std = np.abs(got[2][v] - std[v]) / std[v]
        assert e_std.max(initial=0) <= 1e-9, f"{what}: std, relative error {e_std.max():.2e}"
    # a NaN stays in its own column (and reaches all four of its statistics)
    for k in (1, 2, 3, 4):
        assert np.array_equal(np.isnan(got[k]), (~ok) | (k == 2 and B == 1)), f"{what}: NaN columns of {r._fields[k]}"


@pytest.mark.parametrize("P", [1, 9, 17, 65, 425])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 1000, 4099])
def test_kernel_matches_two_pass_f64(hip_lib, dev, B, P):
    x, kinds, *ref = _columns(B, P)
    xd = torch.from_numpy(x).to(dev)
    m = bg.ColumnMoments(P, dev).update(xd)
    r = m.result()
    assert all(v.dtype == torch.float64 and v.shape == (P,) and v.is_cuda for v in r)
    _check(r, B, kinds, *ref, f"contiguous [{B}, {P}]")
    # a column slice of a wider buffer whose other columns would wreck every statistic
    wide = torch.full((B, P + PAD), 1e30, device=dev)
    wide[:, OFFSET:OFFSET + P] = xd
    view = wide[:, OFFSET:OFFSET + P]
    assert view.stride(0) == P + PAD
    ms = bg.ColumnMoments(P, dev).update(view)
    _check(ms.result(), B, kinds, *ref, f"slice of [{B}, {P + PAD}]")
    assert torch.equal(_bits(ms.state), _bits(m.state))                   # the stride changes nothing
    # two calls on the same input: the same bits
    m2 = bg.ColumnMoments(P, dev).update(xd)
    assert torch.equal(_bits(m2.state), _bits(m.state))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m2.result(), r))


@pytest.mark.parametrize("B,first", [(1000, 300), (4099, 64)])
def test_streaming_matches_one_shot(hip_lib, dev, B, first):
    from bgflow_amd import _lib
    P = 17
    x, kinds, *ref = _columns(B, P)
    xd = torch.from_numpy(x).to(dev)
    one = bg.ColumnMoments(P, dev).update(xd).result()
    m = bg.ColumnMoments(P, dev).update(xd[:first])
    k_first = m.state[:, 1].clone()
    m.update(xd[first:])
    assert torch.equal(_bits(m.state[:, 1]), _bits(k_first))              # the merge keeps the state's K
    before = m.state.clone()
    m.update(xd[:0])                                                      # B = 0: a no-op, in the wrapper and in the entry point
    assert _lib.lib().bgk_column_moments_update(None, P, 0, P, None, 1, None, None) == 0
    assert torch.equal(_bits(m.state), _bits(before)) and m.n_rows == B
    many = m.result()
    _check(many, B, kinds, *ref, f"{first} + {B - first} rows")
    ok = torch.from_numpy(kinds != 4).to(dev)
    const = torch.from_numpy(kinds == 3).to(dev)
    assert torch.equal(many.count, one.count) and torch.equal(many.min[ok], one.min[ok]) and torch.equal(many.max[ok], one.max[ok])
    assert float(((many.mean - one.mean).abs() / one.mean.abs())[ok].max()) <= 1e-12
    assert float(((many.std - one.std).abs() / one.std)[ok & ~const].max()) <= 1e-9
    # the extremes of an earlier chunk survive a later one
    lo_first = bg.ColumnMoments(P, dev).update(xd[:first]).result().min
    assert bool((many.min[ok] <= lo_first[ok]).all())
    # no rows: a status error with text, not a launch
    with pytest.raises(RuntimeError, match="no rows"):
        bg.ColumnMoments(P, dev).result()


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ala2(dev):
    zmat, rigid, xyz = configs.ala2_system()
    data = configs.ala2_whitening_data()
    ic = bg.MixedCoordinateTransformation(data, zmat, rigid, keepdims=9, raise_warnings=False).to(dev)
    return ic, data.to(dev), xyz


def _informed(ic, frames, dev, dtype=torch.float32, n_constraints=0, **kwargs):
    shapes = bg.ShapeDictionary.from_coordinate_transform(ic, n_constraints=n_constraints)
    m = InternalCoordinateMarginals(shapes, {"device": dev, "dtype": dtype})
    m.inform_with_data(frames, ic, **kwargs)
    return m


def test_inform_with_data_end_to_end(hip_lib, dev, golden, ala2):
    G = golden("g_icmarginals")
    ic, data, _ = ala2
    frames = data[:256]
    c_idx = [int(i) for i in G["c_idx"]]
    m = _informed(ic, frames, dev, n_constraints=2, torsions=TORSIONS, constrained_bond_indices=c_idx)
    with torch.no_grad():
        values = [v.cpu().numpy() for v in ic.forward(frames)[:3]]
    failures = []
    for (name, field), v in zip(FIELDS, values):
        d = m[field]
        assert type(d) is bg.TruncatedNormalDistribution and d._mu.is_cuda and d._mu.dtype == torch.float32
        assert d._mu.shape == (15 if name == "bonds" else 17,)
        for stat, got in (("mu", d._mu), ("sigma", d._sigma)):
            ref = G[f"{stat}_{name}_c1_b0_t1_64"]
            got = got.cpu().numpy().astype(np.float64)
            bound = np.maximum(4 * float(G[f"dev_{stat}_{name}"]), 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
            err = np.abs(got - ref)
            print(f"{name} {stat}: max |kernel - reference f64| {err.max():.3e}, bound {bound.min():.3e} (reference's own f32 deviation "
                  f"{float(G[f'dev_{stat}_{name}']):.3e})")
            for col in np.where(err > bound)[0]:
                # a different wrap decision at the 0/1 edge is the one legitimate cause in a torsion column: name the frames
                diff = np.abs(v[:, col] - G[f"ic_{name}"][:, col]) if name != "bonds" else np.zeros(1)
                rows = np.where(diff > 0.5)[0]
                failures.append(f"{name} {stat} column {col}: error {err[col]:.3e} > {bound[col]:.3e}; frames that wrap differently: "
                                f"{[(int(r), float(v[r, col]), float(G[f'ic_{name}'][r, col])) for r in rows]}")
    assert not failures, "\n".join(failures)
    # the same in chunks of 100 frames, statistics streamed (f64 context: the f64 statistics themselves are compared)
    one = _informed(ic, frames, dev, torch.float64, 2, torsions=TORSIONS, constrained_bond_indices=c_idx)
    many = _informed(ic, frames, dev, torch.float64, 2, torsions=TORSIONS, constrained_bond_indices=c_idx, batch_size=100)
    for _, field in FIELDS:
        assert one[field]._mu.dtype == torch.float64
        assert float(((many[field]._mu - one[field]._mu).abs() / one[field]._mu.abs()).max()) <= 1e-9
        assert float(((many[field]._sigma - one[field]._sigma).abs() / one[field]._sigma).max()) <= 1e-9
    # torsions stay uniform unless asked for
    assert type(_informed(ic, frames, dev)[TORSIONS]).__name__ == "SloppyUniform"


def test_built_flow_matches_the_reference(hip_lib, dev, golden, ala2):
    G = golden("g_icmarginals")
    ic, data, _ = ala2
    builder = bg.BoltzmannGeneratorBuilder(bg.ShapeDictionary.from_coordinate_transform(ic), device=dev, dtype=torch.float32)
    m = InternalCoordinateMarginals(builder.current_dims, builder.ctx)
    m.inform_with_data(data[:256], ic, torsions=TORSIONS)
    builder.add_map_to_ic_domains(m)
    builder.add_map_to_cartesian(ic)
    flow = builder.build_flow()
    us = [torch.from_numpy(G[f"flow_u{k}"]).to(dev) for k in range(4)]
    assert flow.segments()[-1][0] == "icdf+ic2xyz"
    with torch.no_grad():
        x_f, d_f = flow(*us)                                   # the fused sampling tail (per-channel: bgk_icdf_ic2xyz_reg)
        bg.SequentialFlow.FUSE_GENERATION_TAIL = False
        try:
            x, d = flow(*us)                                   # block by block
        finally:
            bg.SequentialFlow.FUSE_GENERATION_TAIL = True
        *back, d_back = flow(x, inverse=True)
    bx, bd, bu = 4 * float(G["dev_flow_x"]), 4 * float(G["dev_flow_dlogp"]), 4 * float(G["dev_flow_roundtrip"])
    ex = np.abs(x.cpu().numpy() - G["flow_x64"]).max(1)
    ed = np.abs(d.cpu().numpy().astype(np.float64) - G["flow_dlogp64"])[:, 0]
    print(f"x: max error {ex.max():.3e} (row {ex.argmax()}), bound {bx:.3e}; dlogp: {ed.max():.3e} (row {ed.argmax()}), bound {bd:.3e}")
    assert x.shape == (256, 66) and d.shape == (256, 1)
    assert ex.max() <= bx and ed.max() <= bd                  # every row
    eu = max(float((b - u).abs().max()) for b, u in zip(back, us))
    ec = float((d + d_back).abs().max())
    print(f"round trip: inputs {eu:.3e} (bound {bu:.3e}), log-dets cancel to {ec:.3e} (bound {bd:.3e})")
    assert len(back) == 4 and eu <= bu and ec <= bd
    # the fused tail against the blocks, at the tolerance test_fused_generation_tail_equals_blocks uses for its golden rows
    assert float((x_f - x).abs().max()) <= 5 * float(G["dev_flow_x"]) + 1e-5
    assert float(((d_f - d).abs() / d.abs()).max()) <= 1e-5


def test_training_smoke_with_informed_marginals(hip_lib, dev, golden, ala2):
    G = golden("g_icmarginals")
    ic, data, xyz = ala2
    c_idx = [int(i) for i in G["c_idx"]]
    torch.manual_seed(0)
    shapes = bg.ShapeDictionary.from_coordinate_transform(ic, n_constraints=2)
    target = bg.NormalDistribution(66, torch.tensor(xyz[0], dtype=torch.float32, device=dev))
    builder = bg.BoltzmannGeneratorBuilder(shapes, target=target, device=dev, dtype=torch.float32)
    builder.add_condition(TORSIONS, on=bg.FIXED, hidden=(32, 32))
    builder.add_condition(BONDS, on=ANGLES, hidden=(32, 32))
    m = InternalCoordinateMarginals(builder.current_dims, builder.ctx)
    m.inform_with_data(data, ic, constrained_bond_indices=c_idx)
    assert m[BONDS]._mu.shape == (15,)
    builder.add_map_to_ic_domains(m)
    builder.add_merge_constraints(c_idx, G["mu_bonds_c0_b0_t1_32"][c_idx])
    builder.add_map_to_cartesian(ic)
    gen = builder.build_generator()
    tr = bg.KLTrainer(gen, train_likelihood=True)
    assert type(tr.optim).__name__ == "FlatAdam"
    tr.train(2, data=data, batchsize=256)
    _, _, ys = tr.losses()
    assert len(ys) == 2 and all(len(y) == 2 and np.isfinite(y).all() for y in ys), ys
    assert bool(torch.isfinite(tr.optim.grad).all()) and float(tr.optim.grad.abs().max()) > 0
    assert tr.optim.skipped_steps() == 0
