"""No GPU: what the bounds of test_gpu_slice_walk.py rest on (slice_walk_common.py).  The references alone, against long-double
restatements of the same sums on the same values, use a small share of the one-sided bound, and leaving one element out moves the result
by orders of magnitude more than the bound -- so a kernel that drops or double-counts a sample cannot pass."""
import numpy as np
import pytest

import slice_walk_common as sw


@pytest.mark.parametrize("dtype", sw.DTYPES)
def test_logsumexp_reference_and_the_weight_of_one_element(dtype):
    worst, least = 0.0, np.inf
    for n in sw.BAR_NS:
        for stream in (0, 1):
            v = sw.values(n, dtype, stream).double().numpy()
            ref = sw.bar_reference(n, dtype, stream)
            one_sided = sw.bar_bound(n, ref) / 2
            worst = max(worst, abs(float(np.longdouble(ref) - sw.lse_long_double(-v))) / one_sided)
            if n > 1:               # LSE without element i is LSE + log(1 - e^-w_i / sum)
                moved = np.abs(np.log1p(-np.exp(-v) / np.exp(-v).sum())).min()
                least = min(least, moved / sw.bar_bound(n, ref))
    print(f"{dtype}: torch.logsumexp uses {worst:.3f} of the one-sided bound; one element moves the result by >= {least:.2e} bounds")
    assert worst <= sw.REFERENCE_SHARE and least > sw.BAR_DROP


@pytest.mark.parametrize("dtype", sw.DTYPES)
def test_mbar_reference_and_the_weight_of_one_sample(dtype):
    worst, least = 0.0, np.inf
    for n in sw.MBAR_NS:
        rc, table = sw.values(n, dtype, 2).double().numpy(), sw.mbar_table(n).numpy()
        exact = sw.mbar_long_double(rc, table)
        worst = max(worst, float(np.abs(sw.mbar_reference(n, dtype).numpy() - exact).max()) / (sw.mbar_bound(n) / 2))
        for skip in (0, n - 1):
            least = min(least, float(np.abs(sw.mbar_long_double(rc, table, skip=skip) - exact).max()) / sw.mbar_bound(n))
    print(f"{dtype}: _mbar_torch uses {worst:.3f} of the one-sided bound; the first or last sample moves f by >= {least:.2e} bounds")
    assert worst <= sw.REFERENCE_SHARE and least > sw.MBAR_DROP


def test_the_grid_reaches_every_phase_and_an_empty_block():
    assert sw.OFFSETS[sw.DTYPES[0]] == (0, 1, 2, 3) and sw.OFFSETS[sw.DTYPES[1]] == (0, 1)      # every 16-byte phase of either element size
    per = ((5 + 7 - 1) // 7 + 3) // 4 * 4                            # the slice length of 5 elements in 7 blocks
    assert per == 4 and [max(0, min(5, (b + 1) * per) - min(5, b * per)) for b in range(7)] == [4, 1, 0, 0, 0, 0, 0]
    assert all(sum(sw.mbar_counts(n)) == n and min(sw.mbar_counts(n)) >= 1 for n in sw.MBAR_NS)
    buf, view = sw.padded(sw.values(9, sw.DTYPES[0], 0), 3, -30.0)
    assert view.equal(sw.values(9, sw.DTYPES[0], 0)) and view.data_ptr() - buf.data_ptr() == 4 * (sw.PAD + 3)
    assert float(buf[:sw.PAD + 3].max()) == -30.0 and float(buf[sw.PAD + 3 + 9:].max()) == -30.0 and buf.numel() == 9 + 2 * sw.PAD + 3
