#!/usr/bin/env python
"""Generate tests/golden/philox_edges.npz: global rows at which a kernel's Philox draw lands on a word at either end of the 32-bit
range.  Pure numpy on oracle/philox.py (no reference import, no GPU):

    python tests/golden/make_philox_edge_goldens.py

Why: u01 maps a word x to ((x >> 8) + 0.5) 2^-24 in f32.  The 256 largest words (x >= 0xFFFFFF00, "top") are the ones that would round
to 1.0 without u01's clamp; the 256 smallest (x < 0x100, "bottom") give the smallest u = 2^-25 and the largest Box-Muller radius
sqrt(50 ln 2) = 5.887.  Either kind turns up once per 2^24 words, so no test of random rows ever meets one; every drawing entry point
takes ``row0``, so a test can place such a row in a one-tile batch.

Every kernel's counter is (row low, row high, c2, offset + step), key = seed.  The layouts searched, all at SEED, OFFSET, block 0:

  name       c2        words   rows     the draws it stands for
  field0     0         0..3    all      bgk_philox_fields field 0; the proposals / momenta of bgk_*_mcmc / _hmc / _anneal; the noise w / w1
                                        of bgk_pair_langevin; the sheaf draws of bgk_colmap (its `have_cb`)
  field1     1 << 20   0..3    all      bgk_philox_fields field 1; the noise w2 of bgk_pair_langevin
  accept     1 << 20   0       all      the acceptance draw of bgk_*_mcmc / _hmc / _anneal
  exchange   2 << 20   0       even     the exchange draw of bgk_*_remc at the lower slot of a pair (0, 1) of a ladder of two

Kept per layout, the lowest rows first: at least MIN_TOP top words and MIN_BOTTOM bottom words; for field0 / field1 that many in an even
word position (the u1 of a Box-Muller pair: the radius) AND in an odd one (u2: the angle).

The file (arrays of one length, an entry each): layout (index into `layouts`), c2, row, word (0..3), x (the raw 32-bit word), top (1:
x >= 0xFFFFFF00, 0: x < 0x100); and seed, offset, layouts.  tests/philox_edges_common.py re-derives every entry with one philox4x32_10 call.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import philox  # noqa: E402

SEED, OFFSET = 20261020, 0
LAYOUTS = [("field0", 0, (0, 1, 2, 3), 1), ("field1", 1 << 20, (0, 1, 2, 3), 1), ("accept", 1 << 20, (0,), 1), ("exchange", 2 << 20, (0,), 2)]
MIN_TOP, MIN_BOTTOM = 2, 1
CHUNK, MAX_ROWS = 1 << 22, 1 << 31


def classes(words):
    """the (top, parity) classes a layout must fill: parity of the word position, or None where only word 0 is drawn"""
    return [(top, par) for top in (1, 0) for par in ((0, 1) if len(words) > 1 else (None,))]


def search(c2, words, stride):
    """entries (row, word, x, top) of one layout, rows ascending, until every class holds its minimum"""
    need = {c: (MIN_TOP if c[0] else MIN_BOTTOM) for c in classes(words)}
    found, have = [], {c: 0 for c in need}
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for start in range(0, MAX_ROWS, CHUNK * stride):
        rows = np.arange(start, start + CHUNK * stride, stride, dtype=np.uint64)
        w = philox.philox4x32_10([rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), np.full(rows.size, c2, np.uint64),
                                  np.full(rows.size, OFFSET, np.uint64)], key)
        hits = []
        for q in words:
            for top, sel in ((1, w[q] >= np.uint32(0xFFFFFF00)), (0, w[q] < np.uint32(0x100))):
                hits += [(int(rows[i]), q, int(w[q][i]), top) for i in np.nonzero(sel)[0]]
        for h in sorted(hits):
            c = (h[3], h[1] & 1 if len(words) > 1 else None)
            if have[c] < need[c]:
                have[c] += 1
                found.append(h)
        if all(have[c] >= need[c] for c in need):
            return found
    raise SystemExit(f"c2 = {c2:#x}: {have} after {MAX_ROWS} rows")


def main():
    cols = {k: [] for k in ("layout", "c2", "row", "word", "x", "top")}
    for li, (name, c2, words, stride) in enumerate(LAYOUTS):
        entries = search(c2, words, stride)
        for row, q, x, top in entries:
            for k, v in zip(cols, (li, c2, row, q, x, top)):
                cols[k].append(v)
        print(f"{name}: " + ", ".join(f"row {r} word {q} x {x:#010x}" for r, q, x, _ in entries))
    out = os.path.join(HERE, "philox_edges.npz")
    np.savez(out, seed=np.uint64(SEED), offset=np.uint32(OFFSET), layouts=np.array([l[0] for l in LAYOUTS]),
             layout=np.array(cols["layout"], np.int32), c2=np.array(cols["c2"], np.uint32), row=np.array(cols["row"], np.int64),
             word=np.array(cols["word"], np.int32), x=np.array(cols["x"], np.uint32), top=np.array(cols["top"], np.int32))
    print(f"wrote {out}: {len(cols['row'])} entries, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
