"""CPU: host-side logic of the bgflow-compatible layer (tuple plumbing, error behaviour, shape
bookkeeping), the C-ABI library's exported symbols, and that the product refuses to run without
a HIP device.  Mirrors the reference's tests/nn/flow/test_coupling.py, test_sequential.py,
test_inverted.py, tests/nn/flow/transformer/test_affine.py (:36-42), test_ic.py (:499-516)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib
from bgflow_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_library_exports_every_declared_symbol(hip_lib):
    header = open(os.path.join(ROOT, "include", "bgflow_amd.h")).read()
    declared = set(re.findall(r"\b(bgk_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} is declared in include/bgflow_amd.h but not exported"
    assert declared == set(_lib.ABI_SYMBOLS), "ctypes signature table and header disagree"
    assert hip_lib.bgk_abi_version() == 1


def test_pack_rqs_columns_host_function(hip_lib):
    d, K = 7, 8
    slots = np.array([0, -1, 1, 2, -1, 3, 4], dtype=np.int32)
    ncp = hip_lib.bgk_pack_rqs_columns(d, K, None, None)
    assert ncp == 256
    src = np.empty(ncp, dtype=np.int32)
    hip_lib.bgk_pack_rqs_columns(d, K, slots.ctypes.data, src.ctypes.data)
    P = 3 * K * d + 5
    used = src[src >= 0]
    assert len(set(used)) == len(used) == P and used.max() == P - 1      # a permutation of the reference columns
    assert src[0] == 0 and src[8] == d * K and src[16] == 2 * d * K and src[24] == 3 * d * K
    assert src[25 + 24] == -1                                               # circular dim: no extra slope
    assert src[128] == 5 * K                                                # chunk 1 starts with dim 5


@pytest.mark.parametrize("K,dims_per_chunk", [(4, 9), (8, 5), (12, 3), (16, 2), (32, 1)])
def test_pack_rqs_columns_other_bin_counts(hip_lib, K, dims_per_chunk):
    """the 128-column parameter chunks of the fused spline kernels hold floor(128 / (3 K + 1)) dims; every reference column
    appears exactly once, padding is -1 (transformer/spline.py:113-126 column order [w | h | s | s_nc])"""
    d = 11
    slots = np.arange(d, dtype=np.int32)                       # all dims non-circular: one extra slope column each
    ncp = hip_lib.bgk_pack_rqs_columns(d, K, None, None)
    n_chunks = -(-d // dims_per_chunk)
    assert ncp == 128 * n_chunks
    src = np.empty(ncp, dtype=np.int32)
    hip_lib.bgk_pack_rqs_columns(d, K, slots.ctypes.data, src.ctypes.data)
    P = 3 * K * d + d
    used = src[src >= 0]
    assert len(used) == P and sorted(used) == list(range(P))
    ppd = 3 * K + 1
    for c in range(n_chunks):
        live = min(dims_per_chunk, d - c * dims_per_chunk) * ppd
        assert (src[128 * c:128 * c + live] >= 0).all() and (src[128 * c + live:128 * (c + 1)] == -1).all()
    dim = dims_per_chunk if n_chunks > 1 else 0                # first dim of chunk 1: its widths start at column K * dim
    assert src[128 if n_chunks > 1 else 0] == K * dim


@pytest.mark.parametrize("K,fusable", [(4, True), (8, True), (12, True), (16, True), (32, True), (6, False), (10, False), (64, False)])
def test_fused_plan_bin_counts(hip_lib, K, fusable):
    """which bin counts the one-launch spline coupling kernels take (the others run conditioner + generic spline kernel)"""
    from bgflow_amd import dense
    d, d_c = 3, 5
    tr = bg.ConditionalSplineTransformer(bg.DenseNet([d_c, 128, 128, 3 * K * d + d], torch.nn.SiLU()), is_circular=False)
    nc_host = np.arange(d, dtype=np.int32)
    plan = dense._fused_plan(tr, d, nc_host)
    assert (plan is not None) == fusable
    if fusable:
        assert plan["n_bins"] == K and plan["d_c"] == d_c and plan["mode"] == "f16x2"


def test_kernels_refuse_cpu_tensors(hip_lib):
    tr = bg.ConditionalSplineTransformer(torch.nn.Linear(3, 3 * 8 * 2 + 2))
    with pytest.raises(RuntimeError, match="HIP"):
        tr(torch.zeros(4, 3), torch.rand(4, 2))
    aff = bg.AffineTransformer(torch.nn.Linear(3, 2), torch.nn.Linear(3, 2))
    with pytest.raises(RuntimeError, match="HIP"):
        aff(torch.zeros(4, 3), torch.rand(4, 2))
    ic = bg.RelativeInternalCoordinateTransformation(np.array([[0, 1, 2, 3]]), np.array([1, 2, 3]))
    with pytest.raises(RuntimeError, match="HIP"):
        ic(torch.rand(4, 12))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


# ---- split / merge / swap / coupling / wrap plumbing (reference tests/nn/flow/test_coupling.py) ----
def test_split_flow_sizes_and_indices():
    t = torch.arange(24.0).reshape(2, 12)
    split = bg.SplitFlow(3, 4)
    a, b, c, dlogp = split(t)
    assert a.shape == (2, 3) and b.shape == (2, 4) and c.shape == (2, 5) and dlogp.shape == (2, 1)
    y, dl = split(a, b, c, inverse=True)
    assert torch.equal(y, t)
    with pytest.raises(ValueError):
        bg.SplitFlow(8, 8)(t)
    split = bg.SplitFlow([0, 2], [1, 3, 5], [4, 6, 7, 8, 9, 10, 11])
    a, b, c, _ = split(t)
    assert torch.equal(a, t[:, [0, 2]]) and torch.equal(b, t[:, [1, 3, 5]])
    y, _ = split(a, b, c, inverse=True)
    assert torch.equal(y, t)
    with pytest.raises(ValueError, match="overlapping"):
        bg.SplitFlow([0, 1], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])(t)
    with pytest.raises(ValueError, match="missed"):
        bg.SplitFlow([0, 1], [3, 4, 5, 6, 7, 8, 9, 10, 11])(t)


def test_merge_and_swap_and_inverse():
    t = torch.arange(8.0).reshape(2, 4)
    flow = bg.SequentialFlow([bg.SplitFlow(2), bg.SwapFlow(), bg.MergeFlow(2)])
    y, dlogp = flow(t)
    assert torch.equal(y, t[:, [2, 3, 0, 1]]) and torch.equal(dlogp, torch.zeros(2, 1))
    z, dl = flow(y, inverse=True)
    assert torch.equal(z, t)
    inv = bg.InverseFlow(flow)
    z2, _ = inv(y)
    assert torch.equal(z2, t)
    assert len(flow) == 3 and isinstance(flow[0], bg.SplitFlow) and len(flow[1:]) == 2
    assert [type(b).__name__ for b in flow] == ["SplitFlow", "SwapFlow", "MergeFlow"]


class DummyTransformer(bg.Transformer):
    """y +- 2x, like the reference's DummyTransformer (tests/nn/flow/test_coupling.py:58-70)"""

    def _forward(self, x, y, **kwargs):
        return y + 2 * x.sum(-1, keepdim=True), torch.zeros(*y.shape[:-1], 1)

    def _inverse(self, x, y, **kwargs):
        return y - 2 * x.sum(-1, keepdim=True), torch.zeros(*y.shape[:-1], 1)


@pytest.mark.parametrize("ti,ci", [((1,), (0,)), ((0, 2), (1,)), ((2,), (0, 1))])
def test_coupling_flow_routing(ti, ci):
    xs = [torch.rand(5, 2), torch.rand(5, 3), torch.rand(5, 1)]
    flow = bg.CouplingFlow(DummyTransformer(), transformed_indices=ti, cond_indices=ci)
    *ys, dlogp = flow(*xs, temperature=2.0)          # unknown kwargs are passed through / ignored
    cond_sum = sum(xs[i].sum(-1, keepdim=True) for i in ci)
    for i in range(3):
        expect = xs[i] + 2 * cond_sum if i in ti else xs[i]
        assert torch.allclose(ys[i], expect)
    *zs, _ = flow(*ys, inverse=True)
    for a, b in zip(zs, xs):
        assert torch.allclose(a, b, atol=1e-6)
    with pytest.raises(ValueError):
        bg.CouplingFlow(DummyTransformer(), transformed_indices=(0, 1), cond_indices=(1,))


def test_wrap_flow_and_set_constant():
    xs = [torch.rand(4, 2), torch.rand(4, 3), torch.rand(4, 1)]
    wrap = bg.WrapFlow(bg.SwapFlow(), indices=(0, 2))
    a, b, c, dl = wrap(*xs)
    assert torch.equal(a, xs[2]) and torch.equal(b, xs[1]) and torch.equal(c, xs[0])
    a2, b2, c2, _ = wrap(a, b, c, inverse=True)
    assert torch.equal(a2, xs[0]) and torch.equal(c2, xs[2])
    merge = bg.WrapFlow(bg.MergeFlow(2), indices=(0, 1), out_indices=(0,))
    m, rest, _ = merge(*xs)
    assert m.shape == (4, 5) and torch.equal(rest, xs[2])
    const = bg.SetConstantFlow(indices=[1], values=[torch.tensor([1.0, 2.0])])
    a, k, b, c, dl = const(*xs)
    assert k.shape == (4, 2) and torch.equal(k[3], torch.tensor([1.0, 2.0])) and dl.shape == (4, 1)
    back = const(a, k, b, c, inverse=True)
    assert len(back) == 4 and torch.equal(back[1], xs[1])


def test_sequential_trigger_and_empty():
    class Pen(bg.Flow):
        def _forward(self, x, **kw):
            return x, torch.zeros(x.shape[0], 1)

        def penalty(self):
            return torch.tensor(2.0)
    flow = bg.SequentialFlow([Pen(), bg.SwapFlow(), Pen()])
    assert torch.equal(flow.trigger("penalty"), torch.tensor([2.0, 2.0]))
    assert flow.trigger("nope").numel() == 0


def test_affine_scale_and_circular_is_rejected():
    with pytest.raises(ValueError):
        bg.AffineTransformer(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), is_circular=True)


def test_state_dict_keys_match_reference_layout():
    gen = bg.configs.make_ala2_spline_generator() if hasattr(bg, "configs") else None
    from bgflow_amd import configs
    gen = configs.make_ala2_spline_generator()
    keys = set(gen.flow.state_dict().keys())
    assert "_blocks.0.transformer._params_net._layers.0.weight" in keys
    assert "_blocks.1.transformer._params_net.net._layers.4.bias" in keys
    assert "_blocks.20._flow._delegate._whiten.Twhiten" in keys
    assert "_blocks.16._flow._delegate.distribution._cdf_lower_bound" in keys
    assert sum(p.numel() for p in gen.flow.parameters()) == 1070892
    aff = bg.AffineTransformer(bg.DenseNet([2, 4, 2]), bg.DenseNet([2, 4, 2]))
    assert set(aff.state_dict()) >= {"_log_alpha", "_shift_transformation._layers.0.weight", "_scale_transformation._layers.1.bias"}


def test_decompose_z_matrix_matches_reference(golden):
    G = golden("g_ic")
    blocks, i2a, a2i, i2o = bg.decompose_z_matrix(G["z_matrix"].astype(np.int64), G["rigid_block"].astype(np.int64))
    assert [len(b) for b in blocks] == list(G["dec_block_sizes"])
    assert np.array_equal(np.concatenate(blocks), G["dec_blocks"])
    assert np.array_equal(i2a, G["dec_index2atom"]) and np.array_equal(a2i, G["dec_atom2index"])
    assert np.array_equal(i2o, G["dec_index2order"])
    # invariants of the reference's test_ic.py:499-516
    assert sorted(i2a.tolist()) == list(range(22)) and np.array_equal(i2a[a2i], np.arange(22))
    with pytest.raises(ValueError, match="not reachable"):
        bg.decompose_z_matrix(np.array([[0, 1, 2, 3], [4, 5, 0, 1]]), np.array([1, 2, 3]))


def test_whiten_flow_roundtrip_and_buffers():
    torch.manual_seed(0)
    X = torch.randn(500, 6) @ torch.randn(6, 6)
    wf = bg.WhitenFlow(X, keepdims=4, whiten_inverse=False)
    z, dl = wf(X)
    assert z.shape == (500, 4) and torch.allclose(z.std(0), torch.ones(4), atol=0.05)
    xb, dli = wf(z, inverse=True)
    assert torch.allclose(dl + dli, torch.zeros(500, 1))
    assert set(wf.state_dict()) == {"X0mean", "Twhiten", "Tblacken", "std"}
    with pytest.raises(ValueError):
        bg.WhitenFlow(torch.ones(10, 3), keepdims=3)


def test_boltzmann_generator_api_with_stub_flow():
    class Shift(bg.Flow):
        def _forward(self, x, **kw):
            return x + 1.0, torch.full((x.shape[0], 1), 0.5)

        def _inverse(self, x, **kw):
            return x - 1.0, torch.full((x.shape[0], 1), -0.5)
    prior = bg.NormalDistribution(3)
    target = bg.NormalDistribution(3, mean=torch.ones(3))
    gen = bg.BoltzmannGenerator(prior, bg.SequentialFlow([Shift()]), target)
    torch.manual_seed(1)
    x, z, dlogp, e, lw, w = gen.sample(64, with_latent=True, with_dlogp=True, with_energy=True, with_log_weights=True, with_weights=True)
    assert torch.allclose(x, z + 1) and torch.allclose(w.sum(), torch.tensor(1.0), atol=1e-5)
    kl = gen.kldiv(32)
    assert kl.shape == (32, 1)
    nll = gen.energy(x)
    assert torch.allclose(nll, prior.energy(z) + 0.5)
    ess = bg.effective_sample_size(lw.view(-1))
    assert 0 < float(ess) <= 64.0 + 1e-3


def _emulate_h2_gemm(blocks, NT, S, bvals):
    """numpy restatement of the split-f16 MFMA dataflow: blocks [(S*NT*2 [+NT]), 64, 8] f16 as packed by dense._pack_h2,
    bvals[s][kb][e] = the B operand value lane-half kb supplies for k-slot e of step s.  Returns out[32*NT]."""
    out = np.zeros(32 * NT, np.float64)
    blk = blocks.astype(np.float64)
    for s in range(S):
        for m in range(NT):
            a = blk[(s * NT + m) * 2 + 0] + blk[(s * NT + m) * 2 + 1]          # [64 lanes, 8]: hi + lo
            for lane in range(64):
                i, kb = lane & 31, lane >> 5
                out[32 * m + i] += float(np.dot(a[lane], bvals[s][kb]))
    if blocks.shape[0] > S * NT * 2:
        for m in range(NT):
            b = blk[S * NT * 2 + m]
            out[32 * m:32 * m + 32] += b[:32, 0] + b[:32, 1]
    return out


def test_split_f16_packing_layout():
    """the host-side operand packing of the split-f16 kernels reproduces W x + b when the B operand is fed in the MFMA
    accumulator layout (hidden layers) / natural order (layer 0) -- no GPU needed"""
    from bgflow_amd import packing as dense          # the layout helpers live in packing.py
    rng = np.random.default_rng(0)
    # hidden layer, HT = 4 input tiles (K = 128), NT = 2 output tiles
    W = torch.tensor(rng.normal(size=(64, 128)) * 0.3, dtype=torch.float32)
    b = torch.tensor(rng.normal(size=64), dtype=torch.float32)
    x = rng.normal(size=128)
    e = dense._h2_scale_exp(W, b)
    blocks = dense._pack_h2(W * 2.0 ** e, b * 2.0 ** e, dense._h2_k_hidden(4), NT=2).numpy()
    assert blocks.shape == (8 * 2 * 2 + 2, 64, 8) and blocks.dtype == np.float16
    assert np.abs(blocks.astype(np.float64)).max() < 65504
    # accumulator layout: lane-half kb, register r of tile t holds hidden unit 32 t + (r & 3) + 8 (r >> 2) + 4 kb;
    # k16-step s consumes registers 8 (s & 1) .. + 7 of tile s >> 1
    bv = [[np.array([x[32 * (s >> 1) + ((8 * (s & 1) + ee) & 3) + 8 * ((8 * (s & 1) + ee) >> 2) + 4 * kb] for ee in range(8)])
           for kb in range(2)] for s in range(8)]
    got = _emulate_h2_gemm(blocks, 2, 8, bv) * 2.0 ** -e
    ref = W.double().numpy() @ x + b.double().numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * np.abs(W.numpy()).sum(1).max() * np.abs(x).max())
    # layer 0: natural order, bias as the column of the constant-1 feature, zero padding up to 16 S0
    n_in = 21
    W0 = torch.tensor(rng.normal(size=(128, n_in)), dtype=torch.float32)
    b0 = torch.tensor(rng.normal(size=128), dtype=torch.float32)
    S0 = (n_in + 1 + 15) // 16
    W0e = torch.zeros(128, 16 * S0)
    W0e[:, :n_in] = W0
    W0e[:, n_in] = b0
    blocks0 = dense._pack_h2(W0e, None, dense._h2_k_natural(S0), NT=4).numpy()
    x0 = np.zeros(16 * S0)
    x0[:n_in] = rng.normal(size=n_in)
    x0[n_in] = 1.0
    bv0 = [[x0[16 * s + 8 * kb:16 * s + 8 * kb + 8] for kb in range(2)] for s in range(S0)]
    got0 = _emulate_h2_gemm(blocks0, 4, S0, bv0)
    np.testing.assert_allclose(got0, W0.double().numpy() @ x0[:n_in] + b0.double().numpy(), rtol=0, atol=1e-5)


def test_width_256_packing_reproduces_the_conditioner():
    """operands of the width-256 kernel (dense.pack_dense_for_fused_w256): layer 0 and layer 1 as two 128-row halves, 16 k16-steps in
    the accumulator layout of 8 tiles, parameter chunks regrouped per transformed dim -- a numpy restatement of the kernel's dataflow
    reproduces DenseNet([n_in, 256, 256, P]) column for column"""
    import bgflow_amd as bg
    from bgflow_amd import dense
    from bgflow_amd.utils import hash_init_
    d, n_in, K = 7, 21, 8
    P = 3 * K * d + d
    net = hash_init_(bg.DenseNet([n_in, 256, 256, P], activation=torch.nn.SiLU())).double()
    l0, l1, l2 = net._layers[0], net._layers[2], net._layers[4]
    nc_host = np.arange(d, dtype=np.int32)
    A0, A1, A2, (c0, c1, c2) = dense.pack_dense_for_fused_w256((l0, l1, l2), nc_host, d, K)
    S0 = (n_in + 1 + 15) // 16
    src = dense._src_col_table(d, K, nc_host, "cpu").numpy()
    n_chunks = src.size // 128
    assert A0.shape == (2 * S0 * 8, 64, 8) and A1.shape == (2 * 132, 64, 8) and A2.shape == (n_chunks * 132, 64, 8)
    A0, A1, A2 = A0.numpy(), A1.numpy(), A2.numpy()
    rng = np.random.default_rng(3)
    x = rng.normal(size=n_in)
    x0 = np.zeros(16 * S0)
    x0[:n_in] = x
    x0[n_in] = 1.0
    bv0 = [[x0[16 * s + 8 * kb:16 * s + 8 * kb + 8] for kb in range(2)] for s in range(S0)]
    silu = lambda v: v / (1.0 + np.exp(-v))                                                          # noqa: E731

    def acc_layout(a):      # B operands of the 16 k16-steps taken from 8 accumulator tiles
        return [[np.array([a[32 * (s >> 1) + ((8 * (s & 1) + ee) & 3) + 8 * ((8 * (s & 1) + ee) >> 2) + 4 * kb] for ee in range(8)])
                 for kb in range(2)] for s in range(16)]

    h0 = np.concatenate([_emulate_h2_gemm(A0[g * S0 * 8:(g + 1) * S0 * 8], 4, S0, bv0) for g in range(2)]) * c0
    b1 = acc_layout(silu(h0))
    h1 = np.concatenate([_emulate_h2_gemm(A1[g * 132:(g + 1) * 132], 4, 16, b1) for g in range(2)]) * c1
    b2 = acc_layout(silu(h1))
    got = np.full(P, np.nan)
    for c in range(n_chunks):
        pc = _emulate_h2_gemm(A2[c * 132:(c + 1) * 132], 4, 16, b2) * c2
        live = src[c * 128:(c + 1) * 128] >= 0
        got[src[c * 128:(c + 1) * 128][live]] = pc[live]
        assert np.all(pc[~live] == 0.0)
    ref = net(torch.tensor(x)[None]).detach().numpy()[0]
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * max(1.0, np.abs(ref).max()))


def test_width_256_plan_envelope():
    """hidden layers of 129 .. 256 units plan the width-256 kernel (zero-padded), in split-f16 mode only; wider ones are rejected with
    one warning -- host logic, no launch"""
    import warnings
    import bgflow_amd as bg
    from bgflow_amd import dense
    nc = np.full(5, -1, dtype=np.int32)
    mk = lambda h: bg.ConditionalSplineTransformer(bg.DenseNet([9, *h, 3 * 8 * 5], torch.nn.SiLU()), is_circular=True)     # noqa: E731
    for h, padded in (((256, 256), False), ((200, 130), True), ((64, 256), True)):
        plan = dense._fused_plan(mk(h), 5, nc)
        assert plan["hidden"] == 256 and plan["padded"] == padded and plan["n_bins"] == 8 and plan["cs"] is None
        assert plan["packed"][1].shape == (2 * 132, 64, 8)
    tr = mk((256, 256))
    tr.gemm_mode = "f32"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert dense._fused_plan(tr, 5, nc) is None and dense._fused_plan(mk((384, 384)), 5, nc) is None
    assert len(w) == 2 and "f16x2" in str(w[0].message) and "up to 256" in str(w[1].message)
    assert dense._fused_plan(mk((100, 100)), 5, nc)["hidden"] == 128


def test_linear_layer_packing_reproduces_the_layer():
    """operands of bgk_dense_layer (dense.pack_linear_layer): passes over blocks of <= 256 input columns, each zero-padded to the
    kernel instance's k-steps and to whole 128-row groups -- the numpy restatement of the MFMA dataflow gives W x"""
    from bgflow_amd import dense, _lib
    assert [_lib.lib().bgk_dense_layer_steps(n) for n in (1, 16, 17, 33, 64, 65, 128, 129, 192, 193, 256, 257, 0)] == \
        [1, 1, 2, 4, 4, 8, 8, 12, 12, 16, 16, -1, -1]
    rng = np.random.default_rng(7)
    for n_out, n_in in ((4, 1), (130, 21), (5, 300)):
        W = torch.tensor(rng.normal(size=(n_out, n_in)) * 3.0, dtype=torch.float32)
        x = rng.normal(size=n_in)
        got = np.zeros(n_out)
        passes = dense.pack_linear_layer(W)
        assert len(passes) == (n_in + 255) // 256
        G = (n_out + 127) // 128
        for A, S, c, k0, k1 in passes:
            assert A.shape == (G * S * 8, 64, 8) and 16 * S >= k1 - k0
            xp = np.zeros(16 * S)
            xp[:k1 - k0] = x[k0:k1]
            bv = [[xp[16 * s + 8 * kb:16 * s + 8 * kb + 8] for kb in range(2)] for s in range(S)]
            out = np.concatenate([_emulate_h2_gemm(A.numpy()[g * S * 8:(g + 1) * S * 8], 4, S, bv) for g in range(G)]) * c
            assert np.all(out[n_out:] == 0.0)
            got += out[:n_out]
        ref = W.double().numpy() @ x
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * np.abs(W.numpy()).sum(1).max() * np.abs(x).max())


def test_deep_conditioner_plan_and_packing():
    """spline conditioners with 1, 3, 4 hidden layers (<= 128 units) plan bgk_coupling_rqs_dense_deep: hidden -> hidden layers packed back
    to back with one unscale factor each; the numpy restatement of the MFMA dataflow reproduces the network; nine hidden layers, a
    mixed activation list and the exact-f32 mode are outside the envelope"""
    import warnings
    import bgflow_amd as bg
    from bgflow_amd import dense
    from bgflow_amd.utils import hash_init_
    d, n_in, K = 5, 9, 8
    P = 3 * K * d + d
    nc = np.arange(d, dtype=np.int32)
    silu = lambda v: v / (1.0 + np.exp(-v))                                                          # noqa: E731

    def acc_layout(a):
        return [[np.array([a[32 * (s >> 1) + ((8 * (s & 1) + ee) & 3) + 8 * ((8 * (s & 1) + ee) >> 2) + 4 * kb] for ee in range(8)])
                 for kb in range(2)] for s in range(8)]

    for hidden in ((128,), (128, 128, 128), (64, 128, 32, 100)):
        net = hash_init_(bg.DenseNet([n_in, *hidden, P], activation=torch.nn.SiLU())).double()
        tr = bg.ConditionalSplineTransformer(net, is_circular=False)
        plan = dense._fused_plan(tr, d, nc)
        assert plan["deep"] == len(hidden) and plan["hidden"] == 128 and plan["padded"] == any(h != 128 for h in hidden)
        A0, A1, A2, c0, c1s, c2 = plan["packed"]
        assert len(c1s) == len(hidden) - 1 and (A1 is None) == (len(hidden) == 1)
        assert A1 is None or A1.shape == ((len(hidden) - 1) * 68, 64, 8)
        S0 = (n_in + 1 + 15) // 16
        rng = np.random.default_rng(len(hidden))
        x = rng.normal(size=n_in)
        x0 = np.zeros(16 * S0)
        x0[:n_in] = x
        x0[n_in] = 1.0
        bv0 = [[x0[16 * s + 8 * kb:16 * s + 8 * kb + 8] for kb in range(2)] for s in range(S0)]
        h = silu(_emulate_h2_gemm(A0.numpy(), 4, S0, bv0) * c0)
        for li, c1 in enumerate(c1s):
            h = silu(_emulate_h2_gemm(A1.numpy()[li * 68:(li + 1) * 68], 4, 8, acc_layout(h)) * c1)
        src = dense._src_col_table(d, K, nc, "cpu").numpy()
        got = np.full(P, np.nan)
        for c in range(src.size // 128):
            pc = _emulate_h2_gemm(A2.numpy()[c * 68:(c + 1) * 68], 4, 8, acc_layout(h)) * c2
            live = src[c * 128:(c + 1) * 128] >= 0
            got[src[c * 128:(c + 1) * 128][live]] = pc[live]
        ref = net(torch.tensor(x)[None]).detach().numpy()[0]
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * max(1.0, np.abs(ref).max()))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        nine = bg.ConditionalSplineTransformer(bg.DenseNet([n_in] + [32] * 9 + [P], activation=torch.nn.SiLU()), is_circular=False)
        mixed = bg.ConditionalSplineTransformer(bg.DenseNet([n_in, 32, 32, 32, P], activation=[torch.nn.SiLU(), torch.nn.ReLU(), torch.nn.SiLU()]),
                                                is_circular=False)
        exact = bg.ConditionalSplineTransformer(bg.DenseNet([n_in, 32, 32, 32, P], activation=torch.nn.SiLU()), is_circular=False)
        exact.gemm_mode = "f32"
        assert all(dense._fused_plan(t, d, nc) is None for t in (nine, mixed, exact))
    assert len(w) == 3 and all("1 .. 8 hidden layers" in str(x.message) for x in w)


def test_deep_affine_plan_and_packing():
    """affine conditioners with 1 or 4 hidden layers plan bgk_coupling_affine_dense_deep (widths zero-padded to 64 / 128); the numpy
    restatement of the MFMA dataflow reproduces the README flow's [1, 4, 1] shift network from its packed operands"""
    import bgflow_amd as bg
    from bgflow_amd import dense
    from bgflow_amd.utils import hash_init_
    tr = hash_init_(bg.AffineTransformer(bg.DenseNet([1, 4, 1], torch.nn.ReLU()), bg.DenseNet([1, 4, 1], torch.nn.Tanh())))
    plan = dense._affine_plan(tr, 1)
    assert plan["anydepth"] and plan["depth"] == 2 and plan["hidden"] == 64 and plan["d_c"] == 1
    (A0, A1, A2, c0, c1s, c2), act = plan["packed"][0]
    assert A1 is None and c1s == [] and act == 2 and A0.shape == (1 * 2 * 2, 64, 8) and A2.shape == (4 * 1 * 2 + 1, 64, 8)
    x = 0.37
    x0 = np.zeros(16)
    x0[0], x0[1] = x, 1.0
    h = np.maximum(_emulate_h2_gemm(A0.numpy(), 2, 1, [[x0[8 * kb:8 * kb + 8] for kb in range(2)]]) * c0, 0.0)
    bv = [[np.array([h[32 * (s >> 1) + ((8 * (s & 1) + ee) & 3) + 8 * ((8 * (s & 1) + ee) >> 2) + 4 * kb] for ee in range(8)])
           for kb in range(2)] for s in range(4)]
    out = _emulate_h2_gemm(A2.numpy(), 1, 4, bv) * c2
    ref = tr._shift_transformation.double()(torch.tensor([[x]], dtype=torch.float64)).item()
    assert abs(out[0] - ref) < 2e-6 and np.all(out[1:] == 0.0)
    four = bg.AffineTransformer(bg.DenseNet([12, 128, 64, 32, 100, 20], torch.nn.SiLU()), None)
    plan4 = dense._affine_plan(four, 20)
    assert plan4["anydepth"] and plan4["depth"] == 5 and plan4["hidden"] == 128 and plan4["packed"][1] is None
    assert plan4["packed"][0][0][1].shape == (3 * 68, 64, 8) and len(plan4["packed"][0][0][4]) == 3
    two = dense._affine_plan(bg.AffineTransformer(bg.DenseNet([12, 64, 64, 20], torch.nn.SiLU()), None), 20)
    assert not two["anydepth"] and two["depth"] == 3


def test_gemm_mode_switch_and_errors():
    import bgflow_amd as bg
    from bgflow_amd import dense
    tr = bg.ConditionalSplineTransformer(bg.DenseNet([9, 128, 128, 408], torch.nn.SiLU()), is_circular=True)
    assert dense._gemm_mode(tr) == dense.GEMM_MODE
    tr.gemm_mode = "f32"
    assert dense._gemm_mode(tr) == "f32"
    tr.gemm_mode = "fp8"
    with pytest.raises(ValueError):
        dense._gemm_mode(tr)


def _builder_cfg3():
    """the cfg-3 recipe written against the builder API exactly as a bgflow user would (generator_builder.py docstring)"""
    from bgflow_amd import configs
    zmat, rigid, xyz = configs.ala2_system()
    ic = bg.MixedCoordinateTransformation(configs.ala2_whitening_data(), zmat, rigid, keepdims=9, raise_warnings=False)
    shapes = bg.ShapeDictionary.from_coordinate_transform(ic)
    builder = bg.BoltzmannGeneratorBuilder(shapes, target=bg.NormalDistribution(66, torch.tensor(xyz[0], dtype=torch.float32)),
                                           dtype=torch.float32)
    for _ in range(4):
        builder.add_condition(bg.TORSIONS, on=bg.FIXED)
        builder.add_condition(bg.FIXED, on=bg.TORSIONS)
    for _ in range(4):
        builder.add_condition(bg.BONDS, on=bg.ANGLES)
        builder.add_condition(bg.ANGLES, on=bg.BONDS)
    builder.add_map_to_ic_domains()
    builder.add_map_to_cartesian(ic)
    return builder, shapes


def test_builder_reproduces_the_cfg3_flow():
    from bgflow_amd import configs
    builder, shapes = _builder_cfg3()
    assert list(shapes.items()) == [(bg.BONDS, (17,)), (bg.ANGLES, (17,)), (bg.TORSIONS, (17,)), (bg.FIXED, (9,))]
    assert list(builder.current_dims) == [bg.TARGET] and builder.current_dims[bg.TARGET] == (60,)
    gen = builder.build_generator()
    assert builder.layers == [] and list(builder.current_dims) == list(shapes)      # cleared after building
    ref = configs.make_ala2_spline_generator()
    a, b = gen.flow.state_dict(), ref.flow.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert [type(x).__name__ for x in gen.flow] == [type(x).__name__ for x in ref.flow]
    for x, y in zip(gen.flow, ref.flow):
        if isinstance(x, bg.CouplingFlow):
            assert (x.transformed_indices, x.cond_indices) == (y.transformed_indices, y.cond_indices)
    assert [tuple(s) for s in gen.prior.event_shapes] == [(17,), (17,), (17,), (9,)]
    z = gen.prior.sample(5)
    assert [tuple(t.shape) for t in z] == [(5, 17), (5, 17), (5, 17), (5, 9)] and all((t >= 0).all() and (t <= 1).all() for t in z)


def test_shape_dictionary_and_builder_bookkeeping():
    s = bg.ShapeDictionary()
    s[bg.BONDS], s[bg.ANGLES], s[bg.TORSIONS] = (21,), (20,), (19,)
    a1, a2 = bg.TensorInfo("A1"), bg.TensorInfo("A2")
    s.split(bg.ANGLES, (a1, a2), (8, 12))
    assert list(s) == [bg.BONDS, a1, a2, bg.TORSIONS] and s[a2] == (12,)
    with pytest.raises(ValueError):
        s.split(a1, (bg.TensorInfo("x"), bg.TensorInfo("y")), (3, 3))
    assert s.dim_all() == 60 and s.dim_circular() == 19 and s.dim_noncircular((bg.BONDS, a1)) == 29
    assert s.circular_indices((a2, bg.TORSIONS)).tolist() == list(range(12, 31))
    assert s.is_circular((bg.TORSIONS,)).all() and s.index(a2) == 2 and s.names((a1,)) == ["A1"]
    s.merge((a1, a2), to=bg.ANGLES)
    assert list(s) == [bg.BONDS, bg.ANGLES, bg.TORSIONS] and s[bg.ANGLES] == (20,)
    r = s.replace(bg.BONDS, "B2")
    assert r.name == "B2" and list(s)[0] == r and s.copy() == s and s.copy() is not s
    # builder: split / merge layers, errors of add_condition, param groups
    shapes = bg.ShapeDictionary()
    shapes[bg.BONDS], shapes[bg.ANGLES] = (4,), (6,)
    b = bg.BoltzmannGeneratorBuilder(shapes)
    s1, s2 = b.add_split(bg.ANGLES, ("S1", "S2"), (2, 4))
    assert list(b.current_dims) == [bg.BONDS, s1, s2] and not s1.is_circular
    b.add_condition(s1, on=s2, param_groups=("g",), hidden=(16,))
    b.add_condition(bg.BONDS, on=(s1, s2), transformer_type=bg.AffineTransformer)
    assert len(b.param_groups["g"]) == 4
    with pytest.raises(ValueError):
        b.add_condition(s1, on=())
    with pytest.raises(ValueError):
        b.add_merge((s1, bg.TensorInfo("c", True)), to="M")
    b.add_merge((s1, s2), to=bg.ANGLES)
    assert list(b.current_dims) == [bg.BONDS, bg.ANGLES]
    flow = b.build_flow()
    names = [type(x).__name__ for x in flow]
    assert names == ["WrapFlow", "CouplingFlow", "CouplingFlow", "WrapFlow"]
    net = flow[1].transformer._params_net
    assert [m.out_features for m in net._layers if hasattr(m, "out_features")] == [16, 3 * 8 * 2 + 2]
    assert isinstance(flow[2].transformer, bg.AffineTransformer) and flow[2].cond_indices == [1, 2]
    with pytest.raises(NotImplementedError):
        b.add_merge_constraints()
    prior = bg.BoltzmannGeneratorBuilder(shapes).build_prior()
    assert [tuple(e) for e in prior.event_shapes] == [(4,), (6,)]


def test_builder_reproduces_the_augmented_cfg5_flow():
    """cfg 5 through the builder: AUGMENTED field, per-field transformer type, multi-field conditioning"""
    from bgflow_amd import configs
    zmat, rigid, xyz = configs.ala2_system()
    ic = bg.MixedCoordinateTransformation(configs.ala2_whitening_data(), zmat, rigid, keepdims=9, raise_warnings=False)
    shapes = bg.ShapeDictionary.from_coordinate_transform(ic, dim_augmented=66)
    builder = bg.BoltzmannGeneratorBuilder(shapes, target=bg.NormalDistribution(66, torch.tensor(xyz[0], dtype=torch.float32)),
                                           dtype=torch.float32)
    assert bg.AUGMENTED in builder.targets
    builder.transformer_type[bg.AUGMENTED] = bg.AffineTransformer
    for _ in range(4):
        builder.add_condition(bg.TORSIONS, on=bg.AUGMENTED)
        builder.add_condition(bg.AUGMENTED, on=bg.TORSIONS)
    for _ in range(2):
        builder.add_condition(bg.BONDS, on=bg.ANGLES)
        builder.add_condition(bg.ANGLES, on=bg.BONDS)
    for _ in range(2):
        builder.add_condition(bg.FIXED, on=bg.AUGMENTED)
        builder.add_condition(bg.AUGMENTED, on=(bg.FIXED, bg.BONDS, bg.ANGLES))
    builder.add_map_to_ic_domains()
    builder.add_map_to_cartesian(ic)
    assert list(builder.current_dims) == [bg.TARGET, bg.AUGMENTED]
    gen = builder.build_generator()
    ref = configs.make_ala2_augmented_generator()
    a, b = gen.flow.state_dict(), ref.flow.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert sum(p.numel() for p in gen.flow.parameters()) == 1072356      # probe of the reference builder


def test_reference_style_import_paths_resolve():
    """sub-package import paths used by bgflow code resolve to the accelerated classes (bgflow_amd/_compat.py)"""
    import importlib
    from bgflow_amd.nn.flow.crd_transform.ic import GlobalInternalCoordinateTransformation, MixedCoordinateTransformation
    from bgflow_amd.nn.flow.transformer.spline import ConditionalSplineTransformer
    from bgflow_amd.nn.flow.coupling import CouplingFlow, SplitFlow
    from bgflow_amd.nn.periodic import WrapPeriodic
    from bgflow_amd.distribution.normal import NormalDistribution
    from bgflow_amd.factory.tensor_info import BONDS, TORSIONS, ShapeDictionary
    from bgflow_amd.factory.generator_builder import BoltzmannGeneratorBuilder
    assert MixedCoordinateTransformation is bg.MixedCoordinateTransformation and CouplingFlow is bg.CouplingFlow
    assert ConditionalSplineTransformer is bg.ConditionalSplineTransformer and WrapPeriodic is bg.WrapPeriodic
    assert BoltzmannGeneratorBuilder is bg.BoltzmannGeneratorBuilder and TORSIONS.is_circular and not BONDS.is_circular
    assert importlib.import_module("bgflow_amd.nn.flow.cdf").CDFTransform is bg.CDFTransform
    assert GlobalInternalCoordinateTransformation is bg.GlobalInternalCoordinateTransformation and ShapeDictionary and SplitFlow and NormalDistribution
    with pytest.raises(ImportError):
        importlib.import_module("bgflow_amd.nn.flow.dynamics")      # outside the hot path: not provided


def test_c_abi_argument_validation_needs_no_gpu(hip_lib):
    """status codes and bgk_last_error of the entry points: validation happens before any launch, so this runs on a CPU box
    (fake non-null pointers are never dereferenced on these paths)"""
    L = hip_lib
    P1 = ctypes.c_void_p(0x1000)         # a non-null placeholder
    err = lambda: L.bgk_last_error().decode(errors="replace")      # noqa: E731
    # empty batches are a no-op
    assert L.bgk_rqs_transform(P1, 17, P1, 425, 425, P1, 0, 17, 8, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None) == 0
    assert L.bgk_affine_transform(P1, 4, P1, 4, P1, 4, P1, 0, 0, 0, 0, 4, P1, 4, P1, 0, None) == 0
    # ... even with the NULL pointers empty tensors have (torch: data_ptr() == 0 for numel() == 0)
    assert L.bgk_rqs_transform(None, 17, None, 425, 425, P1, 0, 17, 8, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, None, 17, None, 0, None, None, None) == 0
    assert L.bgk_affine_transform(None, 4, None, 4, None, 4, P1, 0, 0, 0, 0, 4, None, 4, None, 0, None) == 0
    # bad sizes / null pointers -> BGK_EINVAL with a message
    assert L.bgk_rqs_transform(P1, 17, P1, 425, 425, P1, -1, 17, 8, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None) == -1
    assert "bad sizes" in err()
    assert L.bgk_rqs_transform(None, 17, P1, 425, 425, P1, 4, 17, 8, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None) == -1
    assert "null pointer" in err()
    assert L.bgk_rqs_transform(P1, 17, P1, 425, 425, P1, 4, 17, 8, 0, 0.0, 1.0, 0.0, 1.0, 0.2, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None) == -1
    assert "Minimal bin width/height too large" in err()                      # the reference's ValueError text (nflows)
    assert L.bgk_affine_transform(P1, 4, P1, 4, P1, 4, P1, 0, 1, 0, 8, 4, P1, 4, P1, 0, None) == -1
    assert "Scaling is not compatible with periodicity." in err()             # transformer/affine.py:26-27
    # valid requests outside a fused kernel's envelope -> BGK_EUNSUPPORTED (callers fall back to the generic kernels)
    # (bgk_rqs_backward takes any bin count since round 5: its argument checks only)
    assert L.bgk_rqs_backward(P1, 17, P1, 263, 300, P1, 8, 17, 5, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, P1, 17, P1, 263, None, 0, None) == -1
    assert "bad params width" in err()
    assert L.bgk_rqs_backward(P1, 17, P1, 263, 263, P1, 8, 17, 5, 0, 0.0, 1.0, 0.0, 1.0, 0.3, 1e-3, 1e-3, 1, P1, 17, P1, P1, 17, P1, 263, None, 0, None) == -1
    assert "too large for the number of bins" in err()
    tail = (P1, 17, 8, 17, 8, 0, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None)
    assert L.bgk_coupling_rqs_dense_h2(P1, 17, 17, 0, P1, P1, P1, 1.0, 1.0, 1.0, None, 0, 64, 64, 1, *tail) == -2
    assert "hidden=(128,128)" in err()
    assert L.bgk_coupling_rqs_dense_h2(P1, 17, 17, 0, P1, P1, P1, 1.0, 1.0, 1.0, None, 7, 128, 128, 1, *tail) == -1
    assert "operand_dtype" in err()
    assert L.bgk_coupling_affine_dense_h2(P1, 32, 32, 0, P1, P1, P1, 1.0, 1.0, 1.0, 2, P1, P1, P1, 1.0, 1.0, 1.0, 3,
                                          256, P1, 0, 0, 0, P1, 32, 8, 32, P1, 32, P1, 0, None) == -2
    assert L.bgk_dense_backward_dx(P1, 425, 425, P1, P1, P1, 120, 120, 0, P1, P1, P1, P1, 1, 8, P1, P1, P1, P1, None, 0, None, 0, None, None, None) == -2
    assert L.bgk_column_sum(P1, 4, 8, 0, P1, 4, P1, None) == -1
    # round 4 entry points: empty batches, envelope and argument checks before any launch
    n1 = (ctypes.c_void_p * 1)(0x1000)
    i1 = (ctypes.c_int32 * 1)(0)
    assert L.bgk_pack_dense_h2_many(0, n1, n1, i1, n1, n1, n1, n1, i1, n1, i1, n1, n1, n1, n1, None) == 0      # no conditioner: no launch
    assert L.bgk_pack_dense_h2_many(1, n1, n1, i1, n1, n1, n1, n1, i1, n1, i1, n1, n1, n1, n1, None) == -1 and "bad conditioner 0" in err()
    assert L.bgk_pack_dense_h2_t_many(0, n1, i1, n1, n1, i1, n1, n1, n1, n1, None) == 0
    assert L.bgk_pack_dense_h2_t_many(1, n1, i1, n1, n1, i1, n1, n1, n1, n1, None) == -1 and "bad conditioner 0" in err()
    b1 = (ctypes.c_int64 * 1)(0)
    assert L.bgk_dense_weight_grad_reduce_many(0, b1, i1, i1, n1, n1, n1, n1, n1, n1, n1, 1, None) == 0
    assert L.bgk_dense_weight_grad_reduce_many(1, b1, i1, i1, n1, n1, n1, n1, n1, n1, n1, 1, None) == -1 and "bad layer 0" in err()
    assert L.bgk_dense_weight_grad_reduce_many(1, b1, i1, i1, n1, n1, n1, n1, n1, n1, n1, 2, None) == -1
    assert L.bgk_icdf_ic2xyz_uni_train(P1, P1, P1, P1, P1, 1, 1e-7, P1, 17, P1, 5, 1e-7, 1, P1, P1, 9, 0.0, 0,
                                       P1, 66, P1, 0, None, P1, P1, P1, P1, None) == 0                      # empty batch
    assert L.bgk_icdf_ic2xyz_uni_train(P1, P1, P1, P1, P1, 1, 1e-7, P1, 17, P1, 5, 1e-7, 1, P1, P1, 9, 0.0, 64,
                                       P1, 66, P1, 0, None, None, P1, P1, P1, None) == -1 and "null pointer" in err()


def test_c_abi_argument_validation_of_the_wide_envelope_entry_points(hip_lib):
    """round-5 entry points (hidden width 256, any-depth spline / affine conditioners, bgk_dense_layer and its packer): empty batches are
    a no-op, bad arguments BGK_EINVAL, shapes outside the envelope BGK_EUNSUPPORTED -- all before any launch (no GPU needed)"""
    L = hip_lib
    P1 = ctypes.c_void_p(0x1000)
    err = lambda: L.bgk_last_error().decode(errors="replace")      # noqa: E731
    tail = (P1, 17, 8, 17, 8, 0, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None)
    # hidden width 256: split-f16 inference only (operand_dtype 1 = bf16 is outside the envelope), other widths unsupported
    assert L.bgk_coupling_rqs_dense_h2(P1, 17, 17, 0, P1, P1, P1, 1.0, 1.0, 1.0, None, 1, 256, 256, 1, *tail) == -2 and "width 256" in err()
    assert L.bgk_coupling_rqs_dense_h2(P1, 17, 17, 0, P1, P1, P1, 1.0, 1.0, 1.0, None, 0, 192, 192, 1, *tail) == -2
    # any-depth spline entry: 1 .. 8 hidden layers, the fused bin counts, host array of unscale factors
    c1 = (ctypes.c_float * 8)(*([1.0] * 8))
    dtail = (1, P1, 17, 8, 17, 8, 0, 0, 0.0, 1.0, 0.0, 1.0, 1e-3, 1e-3, 1e-3, 1, P1, 17, P1, 0, None, None, None)
    zero_b = dtail[:3] + (0,) + dtail[4:]
    assert L.bgk_coupling_rqs_dense_deep(None, 17, 17, 0, None, None, None, 1.0, c1, 1.0, 3, *zero_b) == 0
    assert L.bgk_coupling_rqs_dense_deep(P1, 17, 17, 0, P1, P1, P1, 1.0, c1, 1.0, 9, *dtail) == -2 and "hidden layers" in err()
    assert L.bgk_coupling_rqs_dense_deep(P1, 17, 17, 0, P1, P1, P1, 1.0, c1, 1.0, 0, *dtail) == -2
    assert L.bgk_coupling_rqs_dense_deep(P1, 17, 17, 0, P1, None, P1, 1.0, c1, 1.0, 3, *dtail) == -1 and "hidden-layer operands" in err()
    k7 = dtail[:5] + (7,) + dtail[6:]
    assert L.bgk_coupling_rqs_dense_deep(P1, 17, 17, 0, P1, P1, P1, 1.0, c1, 1.0, 3, *k7) == -2
    assert L.bgk_coupling_rqs_dense_deep(P1, 17, 120, 0, P1, P1, P1, 1.0, c1, 1.0, 3, *dtail) == -2 and "layer-0 tile" in err()
    # any-depth affine entry
    atail = (P1, 0, 0, 0, P1, 32, 8, 32, P1, 32, P1, 0, None)
    nets = (P1, P1, P1, 1.0, c1, 1.0, 2, P1, P1, P1, 1.0, c1, 1.0, 3)
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, *nets, 4, 64, *(atail[:6] + (0,) + atail[7:])) == 0
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, *nets, 9, 64, *atail) == -2 and "hidden layers" in err()
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, *nets, 4, 96, *atail) == -2
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, P1, None, P1, 1.0, c1, 1.0, 2, None, None, None, 1.0, None, 1.0, 0, 4, 64, *atail) == -1 \
        and "incomplete shift network" in err()
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, None, None, None, 1.0, None, 1.0, 0, None, None, None, 1.0, None, 1.0, 0, 1, 64, *atail) == -1 \
        and "no conditioner network" in err()
    assert L.bgk_coupling_affine_dense_deep(P1, 32, 32, 0, *nets, 4, 64, P1, 0, 1, 0, *atail[4:]) == -1 and "not compatible with periodicity" in err()
    # one Linear layer on its own
    assert L.bgk_dense_layer(None, 40, 0, 40, None, 4, 1.0, None, None, 70, 1, None, 70, 0, None) == 0
    assert L.bgk_dense_layer(P1, 40, 8, 40, P1, 4, 1.0, None, None, 70, 4, P1, 70, 0, None) == -1 and "act 4" in err()
    assert L.bgk_dense_layer(P1, 40, 8, 40, P1, 2, 1.0, None, None, 70, 1, P1, 70, 0, None) == -1 and "k-steps" in err()
    assert L.bgk_dense_layer(P1, 300, 8, 300, P1, 16, 1.0, None, None, 70, 1, P1, 70, 0, None) == -1 and "at most 256" in err()
    assert L.bgk_dense_layer(P1, 30, 8, 40, P1, 4, 1.0, None, None, 70, 1, P1, 70, 0, None) == -1
    assert L.bgk_dense_layer(P1, 40, 8, 40, ctypes.c_void_p(0x1004), 4, 1.0, None, None, 70, 1, P1, 70, 0, None) == -1 and "16-byte aligned" in err()
    assert L.bgk_pack_linear_layer(P1, 40, 70, 300, P1, P1, None) == -1 and "at most 256" in err()
    assert L.bgk_pack_linear_layer(P1, 30, 70, 40, P1, P1, None) == -1
    assert L.bgk_pack_linear_layer(P1, 40, 70, 40, None, P1, None) == -1


def test_dense_layer_dispatch_host_semantics():
    """host side of the layer kernel's dispatch, no GPU: CPU tensors and non-f32 inputs keep torch's own Linear (DenseNet on the host is
    the reference's arithmetic), a wrong input width raises like torch.nn.Linear does instead of reading past the row"""
    import bgflow_amd as bg
    from bgflow_amd import dense
    net = bg.DenseNet([5, 8, 3], activation=torch.nn.Tanh())
    x = torch.randn(7, 5)
    lin0, act, lin1 = net._layers
    assert not dense._on_layer_kernel(lin0, x) and not dense._on_layer_kernel(lin0, x.double())
    with torch.no_grad():
        assert torch.equal(net(x), lin1(act(lin0(x))))
    with pytest.raises(RuntimeError, match="5 input features"):
        dense.dense_layer(torch.randn(7, 6), lin0)
    with pytest.raises(RuntimeError):
        dense.dense_layer(x, lin0)                       # right shape, but not a HIP tensor: no CPU path
    assert dense._LAYER_ACTS[torch.nn.SiLU] == 1 and dense._LAYER_ACTS[torch.nn.ReLU] == 2 and dense._LAYER_ACTS[torch.nn.Tanh] == 3


def test_training_glue_host_semantics():
    """host side of the round-4 training glue, no GPU: row pitches, operand buffer sizes (T2 in whole groups of four k-steps, as the
    header documents), the deferred weight-gradient reductions are dropped when a backward pass raises, and nothing is re-packed
    when no fused layer has run"""
    from bgflow_amd import dense
    from bgflow_amd.utils import param_pitch, row_pitch
    assert row_pitch(425) == 448 and row_pitch(448) == 448 and row_pitch(1) == 32
    assert param_pitch(425) == 428 and param_pitch(408) == 408
    bufs = {}
    T0, T1, T2 = dense._t_operand_bufs(bufs, 425, 34, torch.device("cpu"))
    assert T0.shape == (8 * 2 * 2 + 2, 64, 8) and T1.shape == (68, 64, 8) and T2.shape == (28 * 8 + 4, 64, 8)      # ceil(425 / 16) = 27 -> 28
    assert dense._t_operand_bufs(bufs, 425, 34, torch.device("cpu"))[2] is T2                                      # cached per (P, n_in, device)
    assert dense._t_operand_bufs(bufs, 408, 34, torch.device("cpu"))[2].shape == (28 * 8 + 4, 64, 8)               # 25.5 -> 26 -> 28
    assert dense.repack_training_plans(set()) == 0
    dense._PENDING_REDUCE.clear()
    with pytest.raises(RuntimeError):
        with dense.direct_grad_accumulation():
            dense._PENDING_REDUCE[1] = (torch.device("cpu"), 8, 425, 17, None, (None,) * 6)
            with dense.direct_grad_accumulation():      # a nested context leaves the flush to the outermost one
                pass
            assert 1 in dense._PENDING_REDUCE
            raise RuntimeError("backward failed")
    assert not dense._PENDING_REDUCE and not dense._DIRECT_GRADS[0]
    dense.flush_weight_grad_reductions()                # nothing pending: no library call



def _check_augmentation(G, device):
    """StochasticAugmentation vs the reference (nn/flow/stochastic/augment.py:27-55; golden g_augment): pre-sampled momenta pass
    through with zero log-det, the inverse strips them and charges their energy, return_momenta keeps them, caches work"""
    t = lambda a: torch.as_tensor(a).to(device)  # noqa: E731
    q, p = t(G["q"]), t(G["p"])
    for T, sfx in ((1.0, "T1"), (2.5, "T2p5")):
        layer = bg.StochasticAugmentation(bg.NormalDistribution(6).to(device))
        x, dl = layer(q, momenta=p, temperature=T, cache_momenta=True)
        assert torch.equal(x.cpu(), torch.as_tensor(G[f"x_{sfx}"])) and torch.equal(dl.cpu(), torch.as_tensor(G[f"dlogp_{sfx}"]))
        assert layer._cached_momenta_forward is p
        qb, dli = layer(x, inverse=True, temperature=T, cache_momenta=True)
        assert torch.equal(qb.cpu(), torch.as_tensor(G[f"q_back_{sfx}"]))
        np.testing.assert_allclose(dli.cpu().numpy(), G[f"dlogp_inv_{sfx}"], rtol=1e-6, atol=1e-6)
        assert torch.equal(layer._cached_momenta_backward.cpu(), p.cpu())
        xm, dlm = layer(x, inverse=True, temperature=T, return_momenta=True)
        assert torch.equal(xm.cpu(), torch.as_tensor(G[f"x_mom_{sfx}"])) and float(dlm.abs().max()) == 0.0
        # without momenta: fresh samples of the right shape, log-det = their energy at this temperature
        torch.manual_seed(3)
        x2, dl2 = layer(q, temperature=T)
        assert x2.shape == (q.shape[0], 12) and torch.equal(x2[:, :6], q)
        np.testing.assert_allclose(dl2.cpu().numpy(), layer.distribution.energy(x2[:, 6:], temperature=T).cpu().numpy(), rtol=1e-6)
        assert abs(float(x2[:, 6:].var()) - T) < 0.6 * T


def test_stochastic_augmentation_vs_reference_golden(golden):
    _check_augmentation(golden("g_augment"), torch.device("cpu"))


def test_log_weights_from_samples_host():
    """bg.py:31-52: weights of freshly sampled batches, normalised over all of them"""
    from bgflow_amd.bg import log_weights_from_samples, log_weights_given_latent

    class Shift(bg.Flow):
        def _forward(self, x, **kw):
            return x + 1.0, torch.full((x.shape[0], 1), 0.25)

        def _inverse(self, x, **kw):
            return x - 1.0, torch.full((x.shape[0], 1), -0.25)
    prior, target = bg.NormalDistribution(3), bg.NormalDistribution(3, mean=torch.ones(3))
    torch.manual_seed(0)
    lw = log_weights_from_samples(prior, Shift(), target, num_samples=64, batch_size=16)
    assert lw.shape == (64,) and abs(float(torch.logsumexp(lw, 0))) < 1e-5
    # N(0,1) pushed by +1 onto N(1,1): all weights equal
    np.testing.assert_allclose(lw.numpy(), np.full(64, -np.log(64.0)), atol=1e-5)
    lw_raw = log_weights_from_samples(prior, Shift(), target, num_samples=32, batch_size=16, normalize=False)
    np.testing.assert_allclose(lw_raw.numpy(), 0.25, atol=1e-5)


def test_kltrainer_host_semantics(capsys):
    """KLTrainer / LossReporter / DataSetSampler with the reference's signatures (nn/training/trainers.py:13-205) on a tiny
    pure-torch flow (CPU, torch.optim.Adam path): loss bookkeeping, weighting of the two losses, the NaN-gradient skip"""
    from bgflow_amd.training import KLTrainer, LossReporter, DataSetSampler

    class Scale(bg.Flow):
        def __init__(self):
            super().__init__()
            self.log_s = torch.nn.Parameter(torch.zeros(1, 2))

        def _forward(self, x, **kw):
            return x * torch.exp(self.log_s), self.log_s.sum().expand(x.shape[0], 1)

        def _inverse(self, x, **kw):
            return x * torch.exp(-self.log_s), (-self.log_s.sum()).expand(x.shape[0], 1)
    torch.manual_seed(0)
    gen = bg.BoltzmannGenerator(bg.NormalDistribution(2), Scale(), bg.NormalDistribution(2, mean=torch.zeros(2)))
    data = torch.randn(256, 2) * 2.0
    tr = KLTrainer(gen, optim=torch.optim.Adam(gen.parameters(), lr=5e-2), train_likelihood=True, train_energy=True, test_likelihood=True)
    assert tr.reporter._labels == ("KLL", "NLL", "NLL(Test)") and tr.w_energy == 1.0 and tr.w_likelihood == 1.0
    tr.train(30, data=data, testdata=data[:64], batchsize=64, n_print=0)
    labels, x, ys = tr.losses(n_smooth=5)
    assert labels == ("KLL", "NLL", "NLL(Test)") and len(x) == 26 and all(len(y) == 26 for y in ys)
    assert ys[1][-1] < ys[1][0], "the NLL must go down"
    assert tr.reporter.recent(3).shape == (3, 3)
    # NaN gradient -> the step is skipped, the parameters stay
    before = gen.flow.log_s.detach().clone()
    tr2 = KLTrainer(gen, optim=torch.optim.Adam(gen.parameters(), lr=5e-2), train_likelihood=False, train_energy=True,
                    custom_loss=lambda: gen.flow.log_s.sum() * float("nan"))
    tr2.train(1, batchsize=16, w_custom=1.0)
    assert "found nan in grad; skipping optimization step" in capsys.readouterr().out
    assert torch.equal(gen.flow.log_s.detach(), before)
    # sampler: every element once per epoch
    s = DataSetSampler(torch.arange(10.0)[:, None])
    seen = torch.cat([s.sample(5), s.sample(5)]).reshape(-1).sort().values
    assert torch.equal(seen, torch.arange(10.0))
    rep = LossReporter("a")
    rep.report(torch.tensor(1.0)); rep.report(2.0)
    assert rep.losses()[2][0].tolist() == [1.0, 2.0]


def test_uniform_energy_is_finite_and_product_temperature_like_reference():
    """UniformDistribution.energy never returns inf (reference: falls back to an in-support sample's energy,
    distributions.py:108-114); ProductDistribution sums its components at T = 1 and divides the sum by T (product.py:36-44)"""
    u = bg.UniformDistribution(torch.zeros(3), torch.tensor([1.0, 2.0, 4.0]))
    x = torch.tensor([[0.5, 1.0, 2.0], [7.0, -3.0, 9.0]])
    e = u.energy(x)
    assert e.shape == (2, 1) and torch.isfinite(e).all()
    np.testing.assert_allclose(e.numpy(), np.log(8.0), rtol=1e-6)
    n = bg.NormalDistribution(2)
    prod = bg.ProductDistribution([n, bg.NormalDistribution(3)])
    a, b = torch.randn(5, 2), torch.randn(5, 3)
    T = 2.5
    np.testing.assert_allclose(prod.energy(a, b, temperature=T).numpy(),
                               ((n.energy(a) + bg.NormalDistribution(3).energy(b)) / T).numpy(), rtol=1e-6)
    tr = bg.ConditionalSplineTransformer(torch.nn.Linear(3, 3 * 8 * 2 + 2))
    tr._fused_cache["x"] = 1
    tr.invalidate_fused_cache()
    assert tr._fused_cache == {}


def test_coupling_stack_detection_is_conservative():
    """SequentialFlow.segments(): only Split(sizes) -> (affine Coupling(1 | 0) | Swap)* -> Merge(same sizes) runs become a stack"""
    from bgflow_amd.flow import _coupling_stack_end

    def aff(d_c, d):
        return bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([d_c, 64, 64, d])))

    ok = [bg.SplitFlow(4), aff(4, 4), bg.SwapFlow(), aff(4, 4), bg.SwapFlow(), bg.MergeFlow(4)]
    assert _coupling_stack_end(ok, 0, False) == 5
    assert _coupling_stack_end(list(reversed(ok)), 0, True) == 5          # inverse direction: the merge acts as the split
    assert _coupling_stack_end(list(reversed(ok)), 0, False) is None
    assert [lbl for lbl, _ in bg.SequentialFlow(ok).segments()] == ["coupling stack"]
    one = [bg.SplitFlow(4), aff(4, 4), bg.MergeFlow(4)]
    assert _coupling_stack_end(one, 0, False) is None                     # a single layer gains nothing
    by_index = [bg.SplitFlow([0, 1, 2, 3], [4, 5, 6, 7]), aff(4, 4), aff(4, 4), bg.MergeFlow(4)]
    assert _coupling_stack_end(by_index, 0, False) is None
    other_cond = [bg.SplitFlow(4), aff(4, 4), bg.CouplingFlow(bg.AffineTransformer(shift_transformation=bg.DenseNet([4, 64, 64, 4])),
                                                            transformed_indices=(0,), cond_indices=(1,)), bg.MergeFlow(4)]
    assert _coupling_stack_end(other_cond, 0, False) is None
    mismatch = [bg.SplitFlow(4), aff(4, 4), aff(4, 4), bg.MergeFlow(3)]
    assert _coupling_stack_end(mismatch, 0, False) is None
    three = [bg.SplitFlow(2, 2, 4), aff(2, 2), aff(2, 2), bg.MergeFlow(2, 2, 4)]
    assert _coupling_stack_end(three, 0, False) is None
    flow = bg.SequentialFlow([bg.SwapFlow()] + ok + [bg.SwapFlow()])
    assert [lbl for lbl, _ in flow.segments()] == ["SwapFlow", "coupling stack", "SwapFlow"]
    assert [lbl for lbl, _ in flow.segments(inverse=True)] == ["SwapFlow", "coupling stack", "SwapFlow"]


def test_distribution_transfer_and_constrain_gaussian_flows():
    """DistributionTransferFlow / ConstrainGaussianFlow (bgflow/nn/flow/cdf.py:49-121) on the distributions' own torch ops
    (CPU tensors never reach a kernel): the behaviour the reference's tests/nn/flow/test_cdf.py checks"""
    from torch.distributions import Normal
    swap = bg.DistributionTransferFlow(Normal(torch.zeros(2), torch.ones(2)), Normal(torch.ones(2), torch.ones(2)))
    out, dlogp = swap.forward(torch.zeros(2, 2))
    assert torch.allclose(out, torch.ones(2, 2)) and torch.allclose(dlogp, torch.zeros(2, 1))
    back, dlogp = swap.forward(out, inverse=True)
    assert torch.allclose(back, torch.zeros(2, 2), atol=1e-6) and torch.allclose(dlogp, torch.zeros(2, 1), atol=1e-6)
    torch.manual_seed(1)
    positive = bg.ConstrainGaussianFlow(mu=torch.ones(10), lower_bound=1e-10)
    y, dlogp = positive.forward((1.0 + torch.randn(10, 10)) * 1000.0)
    assert y.shape == (10, 10) and dlogp.shape == (10, 1) and bool((y >= 0.0).all()) and float(dlogp.sum()) < 0.0
    generous = bg.ConstrainGaussianFlow(mu=torch.ones(10), sigma=torch.ones(10), lower_bound=-1000.0, upper_bound=1000.0)
    x = 1.0 + torch.randn(10, 10)
    y, dlogp = generous.forward(x)
    assert torch.allclose(x, y, atol=1e-4, rtol=0.0) and torch.allclose(dlogp, torch.zeros_like(dlogp), atol=1e-4, rtol=0.0)
    x2, dlogp = generous.forward(y, inverse=True)
    assert torch.allclose(x2, y, atol=1e-4, rtol=0.0) and torch.allclose(dlogp, torch.zeros_like(dlogp), atol=1e-4, rtol=0.0)


def test_transfer_flows_match_reference_golden(golden):
    """DistributionTransferFlow / ConstrainGaussianFlow against vectors generated by importing the reference
    (tests/golden/make_goldens.py::g_cdf_flows, nn/flow/cdf.py:49-121), f64 on the CPU path"""
    G = golden("g_cdf_flows")
    x = torch.tensor(synth(501, 64, 6, scale=1.5).astype(np.float64) + 0.8)
    mu = torch.tensor(synth(502, 6).astype(np.float64) * 0.3 + 1.0)
    sigma = torch.tensor(np.abs(synth(503, 6).astype(np.float64)) * 0.4 + 0.6)
    flow = bg.ConstrainGaussianFlow(mu=mu, sigma=sigma, lower_bound=0.1, upper_bound=3.0)
    y, dl = flow.forward(x)
    xb, dlb = flow.forward(y, inverse=True)
    for got, key in ((y, "cg_y"), (dl, "cg_dlogp"), (xb, "cg_back"), (dlb, "cg_back_dlogp")):
        np.testing.assert_allclose(got.numpy(), G[key], rtol=1e-10, atol=1e-10)
    flow = bg.ConstrainGaussianFlow(mu=mu, sigma=sigma, lower_bound=0.0, mu_out=mu + 0.25, sigma_out=0.5 * sigma)
    y, dl = flow.forward(x)
    np.testing.assert_allclose(y.numpy(), G["cg2_y"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(dl.numpy(), G["cg2_dlogp"], rtol=1e-10, atol=1e-10)
    src = torch.distributions.Normal(mu, sigma)
    dst = torch.distributions.Normal(torch.zeros(6, dtype=torch.float64), 2.0 * torch.ones(6, dtype=torch.float64))
    flow = bg.DistributionTransferFlow(src, dst)
    y, dl = flow.forward(x)
    xb, dlb = flow.forward(y, inverse=True)
    for got, key in ((y, "dt_y"), (dl, "dt_dlogp"), (xb, "dt_back"), (dlb, "dt_back_dlogp")):
        np.testing.assert_allclose(got.numpy(), G[key], rtol=1e-10, atol=1e-10)


def test_ic_helper_functions_and_wrap_distances():
    """public helpers of the reference's ic module (ic.py:94-125) and the WrapDistances conditioner front end (periodic.py:40-58)"""
    z = np.array([[0, -1, -1, -1], [1, 0, -1, -1], [2, 1, 0, -1], [3, 2, 1, 0], [4, 3, 2, 1]])
    first, rest = bg.slice_initial_atoms(z)
    assert list(first) == [0, 1, 2] and rest.tolist() == [[3, 2, 1, 0], [4, 3, 2, 1]]
    t0 = torch.tensor([[-3.0, 0.0, 3.0]])
    tn, dl = bg.normalize_torsions(t0)
    tb, dlb = bg.unnormalize_torsions(tn)
    assert torch.allclose(tb, t0, atol=1e-6) and abs(dl + dlb) < 1e-12 and abs(dl + 3 * np.log(2 * np.pi)) < 1e-12
    assert float(tn.min()) >= 0.0 and float(tn.max()) < 1.0
    a0 = torch.tensor([[0.1, 1.5, 3.1]])
    an, dl = bg.normalize_angles(a0)
    ab, dlb = bg.unnormalize_angles(an)
    assert torch.allclose(ab, a0, atol=1e-6) and abs(dl + dlb) < 1e-12 and abs(dl + 3 * np.log(np.pi)) < 1e-12
    # WrapDistances: 2 extra inputs + the 3 pairwise distances of 3 points
    seen = {}

    class Probe(torch.nn.Module):
        def forward(self, f):
            seen["f"] = f
            return f
    x = torch.tensor([[7.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 4.0, 0.0, 9.0]])
    wd = bg.WrapDistances(Probe(), indices=np.arange(1, 10))
    wd(x)
    assert torch.allclose(seen["f"], torch.tensor([[7.0, 9.0, 3.0, 4.0, 5.0]]))


def test_logdet_accumulator_and_catview_host_semantics():
    """flow._LogDetAcc / flow.CatView: the plumbing behind the running log-det and the unconcatenated conditioner inputs (CPU tensors:
    no kernel involved)"""
    from bgflow_amd.flow import _LogDetAcc, CatView, as_tensor
    acc = _LogDetAcc(5, torch.device("cpu"))
    buf, accumulate = acc.peek()
    assert accumulate is False and not acc.started            # peek does not mark the buffer written
    acc.add(None)
    acc.add(acc)                                              # a block that wrote in its own kernel returns the accumulator itself
    assert not acc.started
    acc.add(torch.arange(5.0).reshape(5, 1))                  # a third-party block's [B, 1] term: first writer copies
    acc.add(2.0)                                              # scalar terms (SetConstantFlow-style) are added
    buf2, accumulate = acc.target()
    assert accumulate is True and buf2 is buf
    assert torch.equal(acc.result(), (torch.arange(5.0) + 2.0)[:, None])
    fresh = _LogDetAcc(3, torch.device("cpu"))
    assert torch.equal(fresh.result(), torch.zeros(3, 1))     # a pass without any log-det term is zero, not garbage
    a, b = torch.randn(4, 3), torch.randn(4, 2)
    cv = CatView([a, b])
    assert cv.shape[-1] == 5 and torch.equal(cv.cat(), torch.cat([a, b], -1)) and torch.equal(as_tensor(cv), cv.cat())
    assert as_tensor(a) is a


def test_zero_padded_hidden_layers_compute_the_same_function():
    """dense._pad_hidden: the stand-in layers the packers read for hidden widths below the kernels' 64 / 128 rows"""
    import bgflow_amd as bg
    from bgflow_amd.dense import _pad_hidden
    for act in (torch.nn.SiLU(), torch.nn.ReLU(), torch.nn.Tanh()):
        net = bg.DenseNet([9, 32, 96, 40], activation=act)
        lins = [m for m in net._layers if isinstance(m, torch.nn.Linear)]
        padded = _pad_hidden(lins, 128)
        assert [tuple(p.weight.shape) for p in padded] == [(128, 9), (128, 128), (40, 128)]
        x = torch.randn(6, 9)
        h = x
        for i, p in enumerate(padded):
            h = h @ p.weight.T + p.bias
            if i < 2:
                h = act(h)
                assert torch.count_nonzero(h[:, lins[i].out_features:]) == 0      # padded units hold act(0) = 0
        assert torch.allclose(h, net(x), atol=1e-6)


def test_exported_symbols_are_the_headers_prototypes():
    """libbgflow_amd.so is built with hidden visibility and an export list generated from include/bgflow_amd.h: its dynamic symbol table
    is exactly the header's prototypes -- no launcher shared between translation units, no option variable, no hipcc marker leaks."""
    import re
    import subprocess
    from bgflow_amd import _lib, build
    want = set(build.abi_symbols())
    assert len(want) >= 42 and "bgk_coupling_rqs_dense_h2" in want
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ [A-Za-z] ", ln)}
    assert have == want, f"only in the library: {sorted(have - want)}; only in the header: {sorted(want - have)}"
    sigs = build.abi_signatures()
    assert set(sigs) == want == set(_lib.ABI_SYMBOLS)
    handle = _lib.lib()
    for name, (res, args) in sigs.items():          # every function of the loaded handle carries the header's types
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_ctypes_signatures_are_derived_from_the_header():
    """the ctypes table is parsed from include/bgflow_amd.h; four rows written out by hand (no arguments and a string return; the
    eight spline scalars; unsigned 64- and 32-bit parameters; a 64-bit return)"""
    from ctypes import c_char_p, c_double as f64, c_int, c_int32 as i32, c_int64 as i64, c_uint32, c_uint64, c_void_p as vp
    from bgflow_amd import _lib
    sigs = _lib._SIGNATURES
    assert sigs["bgk_last_error"] == (c_char_p, [])
    assert sigs["bgk_rqs_transform"] == (c_int, [vp, i64, vp, i64, i32, vp, i64, i32, i32, i32,
                                                 f64, f64, f64, f64, f64, f64, f64, i32,
                                                 vp, i64, vp, i32, vp, vp, vp])
    assert sigs["bgk_philox_fields"] == (c_int, [c_uint64, c_uint32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, f64, i64, vp, vp])
    assert sigs["bgk_dense_weight_grad_workspace"] == (i64, [i64, i32, i32])


def test_header_parser_refuses_what_it_does_not_know():
    from bgflow_amd._abi import abi_signatures
    ok = abi_signatures(text="/* a comment ( */\nint bgk_a(const float* x, int64_t n);\nconst char* bgk_b(void);\n")
    assert ok == {"bgk_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]), "bgk_b": (ctypes.c_char_p, [])}
    with pytest.raises(ValueError, match="bgk_bad.*size_t n"):
        abi_signatures(text="int bgk_fine(int32_t a);\nint bgk_bad(const float* x, size_t n);\n")
    with pytest.raises(ValueError, match=r"bgk_arr.*float x\[3\]"):
        abi_signatures(text="int bgk_arr(float x[3]);\n")
    with pytest.raises(ValueError, match="bgk_ret"):
        abi_signatures(text="long bgk_ret(int32_t a);\n")
    with pytest.raises(ValueError, match="bgk_open.*cannot split"):
        abi_signatures(text="int bgk_open(int32_t a, int (*cb)(int));\n")


def test_kl_trainer_runs_a_generators_own_kldiv():
    """KLTrainer takes the fused ``kldiv_mean`` path only for the package's own ``BoltzmannGenerator.kldiv``; a subclass that overrides
    ``kldiv`` (regulariser, other target) is evaluated through its code (advisor finding of round 3); likewise a subclass of a kernel-
    describable energy that overrides ``_energy`` is not routed to the energy kernel."""
    import bgflow_amd as bg
    from bgflow_amd.distributions import _kernel_plan
    from bgflow_amd.training import KLTrainer

    class Reg(bg.BoltzmannGenerator):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.w = torch.nn.Parameter(torch.tensor([2.0]))
            self.calls = 0

        def kldiv(self, n_samples, temperature=1.0):
            self.calls += 1
            return (self.w ** 2).expand(n_samples, 1)

        def kldiv_mean(self, *a, **k):
            raise AssertionError("the override was bypassed")

    g = Reg()
    tr = KLTrainer(g, optim=torch.optim.SGD(g.parameters(), lr=0.1), train_likelihood=False)
    tr.train(3, batchsize=8)
    assert g.calls == 3 and float(g.w) < 2.0
    assert abs(tr.losses()[2][0][0] - 4.0) < 1e-6

    class Shifted(bg.NormalDistribution):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    assert _kernel_plan(bg.NormalDistribution(5), 1.0) is not None
    assert _kernel_plan(Shifted(5), 1.0) is None
    assert _kernel_plan(bg.ProductDistribution([bg.NormalDistribution(5), Shifted(5)]), 1.0) is None


def test_bench_default_batches_name_the_baseline_configs():
    """bench.py without --batch: 2^20 samples per GPU, except the cfg-3 flow on 8 GPUs = BASELINE cfg 4 (2^22 over the node, 2^19 per rank)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.default_batch(1, "cfg3") == (1 << 20, False)
    assert bench.default_batch(2, "cfg3") == (1 << 20, False) and bench.default_batch(4, "cfg3") == (1 << 20, False)
    assert bench.default_batch(8, "cfg3") == (1 << 19, True)
    assert bench.default_batch(8, "cfg2") == (1 << 20, False)


def test_bench_dump_outputs_is_a_fixed_sample_under_the_cap(tmp_path):
    """bench.py --dump-outputs: x and dlogp as f32 .npy, the same seeded rows of every array once the whole would pass DUMP_BYTES"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 1 << 20
    x = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 66)
    dlogp = -torch.arange(n, dtype=torch.float32)[:, None]
    for d in ("a", "b"):
        bench.dump_outputs((x, dlogp), str(tmp_path / d))
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("x", "dlogp")}
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES and a["x"].dtype == np.float32 and a["dlogp"].dtype == np.float32
    assert a["x"].shape == (1 << 17, 66) and a["dlogp"].shape == (1 << 17, 1)
    rows = a["x"][:, 0]
    assert (np.diff(rows) > 0).all() and np.array_equal(a["dlogp"][:, 0], -rows) and (a["x"] == rows[:, None]).all()
    assert all(np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy"))) for k in a)
    bench.dump_outputs((x[:1000], dlogp[:1000]), str(tmp_path / "small"))
    assert np.array_equal(np.load(tmp_path / "small" / "x.npy"), x[:1000].numpy())
