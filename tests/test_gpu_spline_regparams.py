"""GPU: the split-f16 inference kernel on operands in row order 2 (register-resident spline parameters, bgk_fused2.hip) -- one
coupling layer against the f64 oracle with the bars of tests/test_gpu_parity.py (log-det per sample within 1e-5, outputs within
1e-6, bin indices equal to the f32 oracle's or an ulp-tie at a knot), over every chunk shape (1..5 dims in the last chunk, both
dead-tile branches), circular / non-circular / mixed masks, periodic and plain conditioners, partial tiles, a launch in which
every resident wave's worth of tiles is exceeded twice over, and the two non-DMA staging forms."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import dense
from bgflow_amd.utils import hash_init_, synth
from test_gpu_parity import assert_bin_ties, rel_per_sample

pytestmark = pytest.mark.gpu

D_C = 6


def _mask(d, kind):
    return {"circular": [True] * d, "noncircular": [False] * d, "mixed": [j % 3 != 1 for j in range(d)]}[kind]


def _layer(d, mask, periodic, dev=None, cond_widths=(D_C,)):
    d_c = sum(cond_widths)
    circ = torch.tensor(_mask(d, mask))
    net = bg.DenseNet([2 * d_c if periodic else d_c, 128, 128, 3 * 8 * d + int((~circ).sum())], activation=torch.nn.SiLU())
    if periodic:
        net = bg.WrapPeriodic(net, indices=np.arange(d_c))
    tr = bg.ConditionalSplineTransformer(params_net=net, is_circular=circ)
    layer = hash_init_(bg.CouplingFlow(tr, transformed_indices=[0], cond_indices=list(range(1, 1 + len(cond_widths)))))
    layer.transformer.gemm_mode = "f16x2"
    return layer.to(dev) if dev is not None else layer


def _inputs(B, d, cond_widths=(D_C,), seed=0):
    return [synth(B + 7 * i + seed, B, w, uniform=True) for i, w in enumerate((d,) + tuple(cond_widths))]


def _run(layer, xs, inverse, dev):
    layer.transformer.return_bin_indices = True
    with torch.no_grad():
        out, *_, dl = layer(*[x if torch.is_tensor(x) else torch.as_tensor(x).to(dev) for x in xs], inverse=inverse)
    plan = layer.transformer._fused_cache
    assert plan.get("mode") == "f16x2" and plan.get("regp_version") == plan["version"], "the row-order-2 operands must have been used"
    return out.cpu().numpy(), dl.cpu().numpy(), layer.transformer.last_bin_indices.cpu().numpy()


def _check_vs_oracle(layer_cpu, xs, inverse, got, what):
    from oracle import flow_oracle as fo
    out, dl, idx = got
    outs64, dl64 = fo.run_block(layer_cpu, [v.astype(np.float64) for v in xs], inverse, np.float64)
    trace = []
    fo.run_block(layer_cpu, xs, inverse, np.float32, trace)
    e_out, e_dl = np.abs(out - outs64[0]).max(), rel_per_sample(dl, dl64, floor=1.0).max()
    print(f"{what}: outputs {e_out:.2e}, log-det per sample {e_dl:.2e}")
    assert e_out <= 1e-6, f"{what}: outputs {e_out:.2e} from the f64 oracle"
    assert e_dl <= 1e-5, f"{what}: log-det per sample {e_dl:.2e}"      # one layer: |dlogp| < 1 per dim, floor 1 as in test_gpu_parity
    n_ties = assert_bin_ties(idx, trace[0], xs[0], what)
    assert n_ties <= max(2, idx.size // 10000)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("mask,periodic", [("circular", True), ("noncircular", False), ("mixed", True), ("mixed", False)])
@pytest.mark.parametrize("d", [1, 2, 5, 6, 9, 17])
def test_regparams_layer_vs_oracle(hip_lib, dev, d, mask, periodic, inverse):
    """d = 1, 2, 5, 6, 9, 17: 1, 2, 5, 1, 4, 2 dims in the last chunk (two-tile and four-tile last chunks, one to four chunks);
    B = 1, 31, 33, 97 rows: partial tiles of one and of several waves -- the batches share one launch set per layer"""
    layer_cpu, layer = _layer(d, mask, periodic), _layer(d, mask, periodic, dev)
    for B in (1, 31, 33, 97):
        xs = _inputs(B, d)
        _check_vs_oracle(layer_cpu, xs, inverse, _run(layer, xs, inverse, dev), f"d={d} {mask} periodic={periodic} inverse={inverse} B={B}")


def _resident_waves(dev):
    return 2 * 4 * torch.cuda.get_device_properties(dev).multi_processor_count      # 2 workgroups of 4 waves per CU


@pytest.mark.parametrize("inverse", [False, True])
def test_regparams_many_tiles_and_tile_independence(hip_lib, dev, inverse):
    """B = 2 * 32 * W + 33 (W = resident waves of a launch): more than two tiles per resident wave, ending on a partial tile.
    Against the oracle, and rows [32 t, 32 t + 32) bit-equal to the same rows run alone as a 32-row batch for the first tile, a tile
    of the second and of the third round of W, and the last (partial) one: no tile reads another tile's buffers."""
    d, W = 17, _resident_waves(dev)
    B = 2 * 32 * W + 33
    layer_cpu, layer = _layer(d, "mixed", True), _layer(d, "mixed", True, dev)
    xs = _inputs(B, d)
    got = _run(layer, xs, inverse, dev)
    _check_vs_oracle(layer_cpu, xs, inverse, got, f"B={B} inverse={inverse}")
    n_tiles = (B + 31) // 32
    for tile in (0, 5, W + 5, 2 * W + 0, n_tiles - 1):
        rows = slice(32 * tile, min(32 * tile + 32, B))
        alone = _run(layer, [x[rows] for x in xs], inverse, dev)
        for a, b, name in zip(alone, got, ("out", "dlogp", "bin_idx")):
            assert np.array_equal(a, b[rows]), f"tile {tile}: {name} differs from the same rows run alone"


@pytest.mark.parametrize("inverse", [False, True])
def test_regparams_non_dma_staging(hip_lib, dev, inverse):
    """inputs that cannot travel by the DMA path: y as a column block of a wider tensor (row stride != d), and a conditioner made of
    two tensors (segment table); both equal, bit for bit, to the contiguous single-tensor call"""
    d, B = 9, 97
    layer_cpu, layer = _layer(d, "mixed", False), _layer(d, "mixed", False, dev)
    xs = _inputs(B, d)
    ref = _run(layer, xs, inverse, dev)
    _check_vs_oracle(layer_cpu, xs, inverse, ref, f"contiguous inverse={inverse}")
    wide = torch.zeros(B, d + 5, device=dev)
    wide[:, 2:2 + d] = torch.as_tensor(xs[0]).to(dev)
    strided = _run(layer, [wide[:, 2:2 + d], xs[1]], inverse, dev)
    for a, b in zip(strided, ref):
        assert np.array_equal(a, b), "row-strided y"
    # the same network behind two conditioning tensors of widths 2 + 4
    layer2_cpu, layer2 = _layer(d, "mixed", False, cond_widths=(2, 4)), _layer(d, "mixed", False, dev, cond_widths=(2, 4))
    xs2 = [xs[0], np.ascontiguousarray(xs[1][:, :2]), np.ascontiguousarray(xs[1][:, 2:])]
    seg = _run(layer2, xs2, inverse, dev)
    _check_vs_oracle(layer2_cpu, xs2, inverse, seg, f"two conditioning tensors inverse={inverse}")
    for a, b in zip(seg, ref):
        assert np.array_equal(a, b), "two conditioning tensors vs their concatenation"


def test_regparams_equal_order_1_bits(hip_lib, dev):
    """the order-2 operands change where a dot product is computed, not its terms: same bits as the order-1 operands"""
    d, B = 17, 1000
    layer = _layer(d, "mixed", True, dev)
    xs = _inputs(B, d)
    for inverse in (False, True):
        new = _run(layer, xs, inverse, dev)
        dense.REGISTER_PARAMS = False
        try:
            with torch.no_grad():
                out, *_, dl = layer(*[torch.as_tensor(x).to(dev) for x in xs], inverse=inverse)
        finally:
            dense.REGISTER_PARAMS = True
        assert np.array_equal(new[0], out.cpu().numpy()) and np.array_equal(new[1], dl.cpu().numpy())
        assert np.array_equal(new[2], layer.transformer.last_bin_indices.cpu().numpy())
