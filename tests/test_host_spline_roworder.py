"""CPU: row order 2 of the spline layers' output operand (bgk_pack_rqs_columns_v, csrc/bgk_pack.hip) -- the order in which the
split-f16 inference kernel finds the widths / heights of a lane's element in that lane's accumulator registers -- is a permutation
of row order 1 chunk by chunk, packs to the same bytes in permuted places, and keeps the chunk and tile counts of order 1."""
import numpy as np
import pytest
import torch

from bgflow_amd import dense

K, PPD, DPC = 8, 25, 5
DIMS = [1, 2, 4, 5, 6, 9, 17]
MASKS = ["circular", "noncircular", "mixed"]


def _slots(d, mask):
    """nc_slot_host: rank of a non-circular dim among the non-circular ones, -1 for a circular dim"""
    circ = {"circular": [True] * d, "noncircular": [False] * d, "mixed": [j % 3 != 1 for j in range(d)]}[mask]
    slots, n = [], 0
    for c in circ:
        slots.append(-1 if c else n)
        n += 0 if c else 1
    return np.array(slots, dtype=np.int32)


def _tables(hip_lib, d, slots):
    out = []
    for order in (1, 2):
        ncp = hip_lib.bgk_pack_rqs_columns_v(d, K, None, order, None, None)
        src = np.empty(ncp, dtype=np.int32)
        perm = np.empty(128, dtype=np.int32)
        assert hip_lib.bgk_pack_rqs_columns_v(d, K, slots.ctypes.data, order, src.ctypes.data, perm.ctypes.data) == ncp
        out.append((src, perm))
    return out


def _live_tiles(src):
    """per chunk: 1 + the highest 32-row tile that holds a source row"""
    return [int(np.nonzero(chunk >= 0)[0].max()) // 32 + 1 for chunk in src.reshape(-1, 128)]


def _kernel_tiles(d):
    """tiles per chunk the kernels multiply: 4, and for the last chunk 2 where its nominal count is <= 2 (the dead-tile rule)"""
    n_chunks = -(-d // DPC)
    last = ((d - (n_chunks - 1) * DPC) * PPD + 31) // 32
    return [4] * (n_chunks - 1) + [2 if last <= 2 else 4]


def test_row_order_1_is_the_existing_table(hip_lib):
    d, slots = 7, _slots(7, "mixed")
    ref = np.empty(256, dtype=np.int32)
    assert hip_lib.bgk_pack_rqs_columns(d, K, slots.ctypes.data, ref.ctypes.data) == 256
    (src1, perm1), _ = _tables(hip_lib, d, slots)
    assert np.array_equal(src1, ref) and np.array_equal(perm1, np.arange(128))
    assert hip_lib.bgk_pack_rqs_columns_v(d, 4, None, 2, None, None) < 0          # order 2 exists for 8 bins only
    assert hip_lib.bgk_pack_rqs_columns_v(d, K, None, 3, None, None) < 0


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("d", DIMS)
def test_row_order_2_is_a_permutation_with_the_same_counts(hip_lib, d, mask):
    slots = _slots(d, mask)
    (src1, _), (src2, perm) = _tables(hip_lib, d, slots)
    # the permutation itself: every row of a chunk's 125 used ones exactly once, 3 positions unused
    assert sorted(perm[perm >= 0]) == list(range(DPC * PPD)) and (perm < 0).sum() == 3
    assert src1.shape == src2.shape and src1.size == 128 * (-(-d // DPC))            # chunk count unchanged
    for c1, c2 in zip(src1.reshape(-1, 128), src2.reshape(-1, 128)):
        assert np.array_equal(c2, np.where(perm >= 0, c1[np.clip(perm, 0, None)], -1))
        assert sorted(c1[c1 >= 0]) == sorted(c2[c2 >= 0])                           # same source rows in the same chunk
    # tile counts: whatever order 1 keeps inside the tiles the kernels multiply, order 2 keeps inside them too; full chunks fill all four
    kt = _kernel_tiles(d)
    assert all(a <= k for a, k in zip(_live_tiles(src1), kt)) and all(a <= k for a, k in zip(_live_tiles(src2), kt))
    assert _live_tiles(src2)[:-1] == _live_tiles(src1)[:-1] == [4] * (len(kt) - 1)
    assert sum(kt) == {17: 14, 9: 8}.get(d, sum(kt))
    # what the kernel relies on: slot IT of half-wave hh (dim 2 IT + hh of the chunk) has width r / height r at register r / 8 + r of tile 2 IT
    for q in range(min(d, 4)):
        for e in range(16):
            pos = 32 * (2 * (q >> 1)) + (e & 3) + 8 * (e >> 2) + 4 * (q & 1)
            assert perm[pos] == PPD * q + e
    for q in range(DPC):                                                           # slab rows (tiles 1, 3): slopes, then dim 4's widths / heights
        for i in range(9):
            sigma = 9 * q + i
            assert perm[32 * (1 + 2 * (sigma >> 5)) + (sigma & 31)] == PPD * q + 16 + i
    for e in range(16):
        sigma = 45 + e
        assert perm[32 * (1 + 2 * (sigma >> 5)) + (sigma & 31)] == PPD * 4 + e


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("d", DIMS)
def test_unpermuting_the_packed_operand_gives_the_order_1_operand(hip_lib, d, mask):
    slots = _slots(d, mask)
    P = 3 * K * d + int((slots >= 0).sum())
    g = torch.Generator().manual_seed(100 * d + len(mask))
    lins = [torch.nn.Linear(a, b) for a, b in ((6, 128), (128, 128), (128, P))]
    with torch.no_grad():
        for lin in lins:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.3)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.3)
    A0a, A1a, A2a, ca = dense.pack_dense_for_fused_h2(lins, slots, d, K)
    A0b, A1b, A2b, cb = dense.pack_dense_for_fused_h2(lins, slots, d, K, row_order=2)
    assert ca == cb and torch.equal(A0a, A0b) and torch.equal(A1a, A1b)
    perm = dense.rqs_row_perm(2)
    n_chunks = -(-d // DPC)
    # [chunk][block][lane][8] halves as 16-bit patterns; block (s * 4 + m) * 2 + p: row 32 m + (lane & 31); bias block 64 + m: lanes 0..31
    old = A2a.view(torch.int16).numpy().reshape(n_chunks, 68, 64, 8)
    new = A2b.view(torch.int16).numpy().reshape(n_chunks, 68, 64, 8)
    assert old.shape == new.shape
    back = np.zeros_like(old)
    for pos in range(128):
        if perm[pos] < 0:
            assert not new[:, :64].reshape(n_chunks, 8, 4, 2, 2, 32, 8)[:, :, pos // 32, :, :, pos % 32].any()
            assert not new[:, 64 + pos // 32, pos % 32].any()
            continue
        m, t, m1, t1 = pos // 32, pos % 32, perm[pos] // 32, perm[pos] % 32
        for s in range(8):
            for p in range(2):
                for kb in range(2):
                    back[:, (s * 4 + m1) * 2 + p, t1 + 32 * kb] = new[:, (s * 4 + m) * 2 + p, t + 32 * kb]
        back[:, 64 + m1, t1] = new[:, 64 + m, t]
    assert back.tobytes() == old.tobytes()
