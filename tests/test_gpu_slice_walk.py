"""On the GPU: the slice walk of csrc/bgk_reduce.h counts every element once, shape by shape, through the C ABI -- ``bgk_bar_solve_steps``
element by element, ``bgk_mbar_solve_steps`` tile by tile.  Sizes on both sides of a piece, of a tile (1024) and of several tiles, every
16-byte phase of the first element, 1, 2 and 7 blocks (slices of 4 and empty blocks); a canary on both sides of the used range must not
reach the result.  Inputs, references and bounds: slice_walk_common.py (test_host_slice_walk.py asserts the references' own error and
that one dropped element is far outside the bounds)."""
import pytest
import torch

from bgflow_amd import _lib
from bgflow_amd import free_energy as fe
from bgflow_amd import umbrella

import slice_walk_common as sw

pytestmark = pytest.mark.gpu


def on_device(v, offset, canary, dev):
    """the view of ``v`` inside its padded buffer on the device, ``offset`` elements past a 16-byte boundary"""
    buf, _ = sw.padded(v, offset, canary)
    buf = buf.to(dev)
    view = buf[sw.PAD + offset:sw.PAD + offset + v.numel()]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (offset * v.element_size()) % 16
    return view


def bar_bounds_step(hip_lib, dev, wf, wr, nbf, nbr):
    """one step on a zeroed record: the BOUNDS phase.  The block partials start as NaN: a block that wrote none shows in the result"""
    record = torch.zeros(fe.RECORD_DOUBLES, dtype=torch.float64, device=dev)
    partial = torch.full((3 * (nbf + nbr),), float("nan"), dtype=torch.float64, device=dev)
    st = hip_lib.bgk_bar_solve_steps(_lib.ptr(wf), wf.numel(), _lib.ptr(wr), wr.numel(), fe._DTYPE_CODES[wf.dtype], nbf, nbr, _lib.ptr(partial),
                                     _lib.ptr(record), 500, 1e-12, 1, _lib.stream_ptr(dev))
    _lib.check(st, "bgk_bar_solve_steps")
    return record.cpu()


@pytest.mark.parametrize("n_blocks", sw.BLOCKS)
@pytest.mark.parametrize("dtype", sw.DTYPES)
def test_bar_bounds_count_every_element_once(hip_lib, dev, dtype, n_blocks):
    """the forward array takes every (n, offset) at ``n_blocks``; the reverse array another n, the next offset and the next block count"""
    offsets, worst = sw.OFFSETS[dtype], 0.0
    nbr = sw.BLOCKS[(sw.BLOCKS.index(n_blocks) + 1) % len(sw.BLOCKS)]
    for i, nf in enumerate(sw.BAR_NS):
        nr = sw.BAR_NS[(i + 7) % len(sw.BAR_NS)]
        upper, lower = sw.bar_upper(nf, dtype), sw.bar_lower(nr, dtype)
        for off in offsets:
            off_r = offsets[(offsets.index(off) + 1) % len(offsets)]
            got = []
            for canary in sw.CANARIES:
                wf = on_device(sw.values(nf, dtype, 0), off, canary, dev)
                wr = on_device(sw.values(nr, dtype, 1), off_r, canary, dev)
                got.append(bar_bounds_step(hip_lib, dev, wf, wr, n_blocks, nbr))
            r = got[0]
            case = f"nF {nf} at +{off} in {n_blocks} blocks, nR {nr} at +{off_r} in {nbr} blocks"
            assert got[1].equal(r), f"{case}: the result changes with the canary"
            assert int(r[0]) == 1 and float(r[fe.R_DELTA]) == float(r[fe.R_UPPER]), case      # PH_F_UPPER: the next evaluation is at the upper bound
            eu, el = abs(float(r[fe.R_UPPER]) - upper), abs(float(r[fe.R_LOWER]) - lower)
            worst = max(worst, eu / sw.bar_bound(nf, upper), el / sw.bar_bound(nr, lower))
            assert eu <= sw.bar_bound(nf, upper), f"{case}: upper {float(r[fe.R_UPPER])!r} against {upper!r}"
            assert el <= sw.bar_bound(nr, lower), f"{case}: lower {float(r[fe.R_LOWER])!r} against {lower!r}"
    print(f"BAR bounds {dtype}, {n_blocks} / {nbr} blocks: worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("n_blocks", sw.BLOCKS)
@pytest.mark.parametrize("dtype", sw.DTYPES)
def test_mbar_iteration_counts_every_sample_once(hip_lib, dev, dtype, n_blocks):
    worst = 0.0
    for n in sw.MBAR_NS:
        want, table = sw.mbar_reference(n, dtype), sw.mbar_table(n, dev)
        for off in sw.OFFSETS[dtype]:
            got = []
            for canary in sw.CANARIES:
                rc = on_device(sw.values(n, dtype, 2), off, canary, dev)
                f = torch.zeros(sw.K, dtype=torch.float64, device=dev)
                record = torch.zeros(umbrella.RECORD_DOUBLES, dtype=torch.float64, device=dev)
                partial = torch.full((n_blocks * sw.K,), float("nan"), dtype=torch.float64, device=dev)
                st = hip_lib.bgk_mbar_solve_steps(_lib.ptr(rc), n, umbrella._DTYPE_CODES[dtype], _lib.ptr(table), sw.K, n_blocks, _lib.ptr(partial),
                                                  _lib.ptr(f), _lib.ptr(record), 1, 0.0, 1, _lib.stream_ptr(dev))
                _lib.check(st, "bgk_mbar_solve_steps")
                got.append((f.cpu(), record.cpu()))
            (f, r), case = got[0], f"n {n} at +{off} in {n_blocks} blocks"
            assert got[1][0].equal(f) and got[1][1].equal(r), f"{case}: the result changes with the canary"
            assert int(r[0]) == umbrella.PHASE_DONE and int(r[1]) == umbrella.BUDGET and int(r[umbrella.R_N_ITER]) == 1, case
            assert int(r[umbrella.R_K]) == sw.K and int(r[umbrella.R_N]) == n, case
            e = float((f - want).abs().max())
            worst = max(worst, e / sw.mbar_bound(n))
            assert e <= sw.mbar_bound(n), f"{case}: f {f.tolist()} against {want.tolist()}"
    print(f"MBAR iteration {dtype}, {n_blocks} blocks: worst error {worst:.3f} of the bound")
