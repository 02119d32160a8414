"""Shared by test_host_philox_edges.py and test_gpu_philox_edges.py: the entries of tests/golden/philox_edges.npz (written by
tests/golden/make_philox_edge_goldens.py) -- global rows at which a kernel's Philox draw is one of the 256 largest ("top": u01 would round
to 1.0 without its clamp) or of the 256 smallest 32-bit words ("bottom": the smallest u, the largest Box-Muller radius) -- re-derived from
oracle/philox.py, and the launch arguments that place such a row on a chosen lane of a one-tile batch."""
import collections
import functools
import os

import numpy as np

from oracle import philox

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "philox_edges.npz")
TOP_FROM, BOTTOM_BELOW = 0xFFFFFF00, 0x100
U_MIN, U_MAX = np.float32(2.0 ** -25), np.float32(1.0 - 2.0 ** -24)
R_MAX = float(np.sqrt(2 * 25 * np.log(2.0)))          # the Box-Muller radius at u1 = 2^-25: 5.887
LANES = (0, 1, 37, 63)                                # where in the tile the targeted row sits: row0 = row - lane

Entry = collections.namedtuple("Entry", "layout c2 row word x top seed offset")


@functools.lru_cache(maxsize=None)
def entries():
    G = np.load(GOLDEN)
    names = [str(s) for s in G["layouts"]]
    seed, offset = int(G["seed"]), int(G["offset"])
    return tuple(Entry(names[int(l)], int(c), int(r), int(w), int(x), bool(t), seed, offset)
                 for l, c, r, w, x, t in zip(G["layout"], G["c2"], G["row"], G["word"], G["x"], G["top"]))


def select(layout, top, word_parity=None):
    """the entries of a layout at the top / bottom of the word range, optionally in an even (Box-Muller u1) or odd (u2) word position"""
    got = [e for e in entries() if e.layout == layout and e.top == top and (word_parity is None or e.word % 2 == word_parity)]
    assert got, f"no fixture entry for {layout}, top={top}, parity={word_parity}"
    return got


def words_of(e, row=None):
    """the four words of the Philox call of an entry (at another row, if given): one philox4x32_10 call"""
    row = e.row if row is None else row
    w = philox.philox4x32_10([np.array([row & 0xFFFFFFFF], np.uint64), np.array([row >> 32], np.uint64), np.array([e.c2], np.uint64),
                              np.array([e.offset], np.uint64)], (e.seed & 0xFFFFFFFF, e.seed >> 32))
    return [int(v[0]) for v in w]


def launches(e, lanes=LANES, batch=64):
    """(row0, B, lane) of launches whose tile holds the entry's row at `lane`: a tile of `batch` rows per lane, and the row alone"""
    return [(e.row - k, batch, k) for k in lanes] + [(e.row, 1, 0)]


def box_muller64(u1, u2):
    """(r cos 2 pi u2, r sin 2 pi u2), r = sqrt(-2 ln u1), in f64 from the f32 uniforms"""
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def box_muller32(u1, u2):
    """the same formula evaluated step by step in numpy f32 (numpy's log / cos / sin, not the kernels' forms)"""
    u1, u2 = np.asarray(u1, np.float32), np.asarray(u2, np.float32)
    rad, ang = np.sqrt(np.float32(-2.0) * np.log(u1)), np.float32(2.0 * np.pi) * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def probe_words():
    """the words of the device probe's test: k << 8 | j for k in [0, 4096), [2^23 - 2048, 2^23 + 2048), [2^24 - 4096, 2^24) and every
    257th k, j in {0, 255}"""
    k = np.unique(np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 2048, 2 ** 23 + 2048), np.arange(2 ** 24 - 4096, 2 ** 24),
                                  np.arange(0, 2 ** 24, 257)])).astype(np.uint32)
    return np.concatenate([(k << np.uint32(8)) | np.uint32(j) for j in (0, 255)])


def normal_bound(n64, err32_large):
    """the bound of a Box-Muller normal in f32 against f64: the suite's 4e-6 for |n| <= 1, above it 4 x the worst error of the plain
    numpy-f32 evaluation on the probe's words (never less than 4e-6)"""
    return np.where(np.abs(n64) <= 1.0, 4e-6, max(4.0 * err32_large, 4e-6))


@functools.lru_cache(maxsize=None)
def probe_reference():
    """for the probe's words w, pairs (w[i], w[i + 1]) (the last with itself): u, the f64 normals, and the measured worst error of the
    numpy-f32 evaluation at |n| > 1 -- computed once"""
    w = probe_words()
    u = philox.u01(w)
    u2 = np.concatenate([u[1:], u[-1:]])
    c64, s64 = box_muller64(u, u2)
    c32, s32 = box_muller32(u, u2)
    big_c, big_s = np.abs(c64) > 1.0, np.abs(s64) > 1.0
    err_large = max(float(np.abs(c32 - c64)[big_c].max()), float(np.abs(s32 - s64)[big_s].max()))
    err_small = max(float(np.abs(c32 - c64)[~big_c].max()), float(np.abs(s32 - s64)[~big_s].max()))
    return dict(w=w, u=u, cos64=c64, sin64=s64, err32_large=err_large, err32_small=err_small)
