#!/usr/bin/env python
"""Generate tests/golden/free_energy.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_free_energy_goldens.py

What runs: the UNMODIFIED ``bgflow.utils.free_energy`` (``bennett_acceptance_ratio``, ``_bar``, ``_bar_zero``) with the import shims of
make_goldens.py.  The fixture holds DATA only.

Work values: u1(x) = x^2 / 2 on x1 ~ N(0, 1), u2(x) = (x - shift)^2 / (2 sigma2^2) on x2 ~ N(shift, sigma2), from a seeded numpy
generator; forward work (offset + u2(x1)) - u1(x1), reverse work u1(x2) - (offset + u2(x2)) (the reference's own test,
tests/utils/test_free_energy.py, is ``pos``).  They are stored as float32 (``{case}_wf``, ``{case}_wr``); the reference is evaluated on
their f64 conversion, so f32 and f64 runs of the package see the same numbers.  Cases (nF / nR):

  pos 1000 / 2000 shift 0.2 offset +1        neg 37 / 1000 shift 0.5 offset -2          far 4096 / 4096 shift 4 offset 3
  scales 1500 / 900 shift 1 sigma2 0.3 offset 10      ragged 257 / 63      tiny 3 / 2      single 1 / 1 (wF 1.3, wR 0.4)
  expand_a, expand_b: the first two cases of a seeded search (1 - 8 samples a side) on which the reference's initial bracket fails at
      least 3 times (asserted; counted from the calls of ``_bar_zero``) and the 500-iteration value is a root to 1e-12
  nooverlap 5 / 5: means -+1e20, energies evaluated in f32: both work arrays are +inf; the reference returns the NaN pair

Per case:

  delta64, unc64   ``_bar(..., relative_tolerance=-inf)`` in f64: the reference's stop test compares with a ``delta_f_old`` that is never
                   reassigned (:149, :163), so with -inf it never fires and all 500 iterations run, whatever the sign of the estimate
  resid64          ``_bar_zero`` at delta64; asserted |resid64| <= 1e-12 on the finite cases
  delta_default, unc_default   the public function with its defaults in f64.  Asserted: ``neg`` differs from delta64 by more than 1e-8
                   (the loop leaves after one secant step when the estimate is negative)
  delta32, unc32   the reference's own f32 run (information)
  n_expand         bracket expansions of the reference
  far_it2          ``_bar(..., maximum_iterations=2, relative_tolerance=-inf)`` on ``far``

``meta``: JSON -- the public function's parameter names and defaults.
"""
import inspect
import json
import os
import sys
import warnings

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.utils import free_energy as ref  # noqa: E402

SEED = 20263
NINF = -float("inf")
CASES = {            # name: (nF, nR, shift, sigma2, offset)
    "pos": (1000, 2000, 0.2, 1.0, 1.0), "neg": (37, 1000, 0.5, 1.0, -2.0), "far": (4096, 4096, 4.0, 1.0, 3.0),
    "scales": (1500, 900, 1.0, 0.3, 10.0), "ragged": (257, 63, 0.7, 1.2, 0.5), "tiny": (3, 2, 0.3, 1.0, 0.2),
}


class TooManyCalls(Exception):
    pass


class Counted:
    """``_bar_zero`` with a call count (and a cap: the reference's bracket expansion has no end of its own)"""

    def __init__(self, cap):
        self.inner, self.calls, self.cap = ref._bar_zero, 0, cap

    def __call__(self, *args):
        self.calls += 1
        if self.calls > self.cap:
            raise TooManyCalls
        return self.inner(*args)

    def __enter__(self):
        ref._bar_zero = self
        return self

    def __exit__(self, *exc):
        ref._bar_zero = self.inner


def works(rng, nf, nr, shift, sigma2, offset):
    x1 = rng.standard_normal(nf)
    x2 = shift + sigma2 * rng.standard_normal(nr)
    u1 = lambda x: 0.5 * x * x                                      # noqa: E731
    u2 = lambda x: 0.5 * ((x - shift) / sigma2) ** 2                # noqa: E731
    return ((offset + u2(x1)) - u1(x1)).astype(np.float32), (u1(x2) - (offset + u2(x2))).astype(np.float32)


def expansions(wf, wr, cap=60):
    """bracket expansions of the reference on (wf, wr), None when it exceeds the cap: calls of _bar_zero = 2 + 2 E + 1 iteration"""
    with Counted(cap) as c:
        try:
            ref._bar(torch.from_numpy(wf).double(), torch.from_numpy(wr).double(), maximum_iterations=1, relative_tolerance=NINF)
        except TooManyCalls:
            return None
    return (c.calls - 3) // 2


def run(wf, wr, dtype, **kw):
    d, u = ref._bar(torch.from_numpy(wf).to(dtype), torch.from_numpy(wr).to(dtype), **kw)
    return d, u


def main():
    rng = np.random.default_rng(SEED)
    data = {name: works(rng, *spec) for name, spec in CASES.items()}
    data["single"] = (np.array([1.3], np.float32), np.array([0.4], np.float32))
    # seeded search for failing initial brackets
    srng = np.random.default_rng(SEED + 1)
    found, tried = [], 0
    while len(found) < 2:
        tried += 1
        assert tried <= 4000, "the search came up empty"
        nf, nr = (int(v) for v in srng.integers(1, 9, size=2))
        wf, wr = works(srng, nf, nr, srng.uniform(-3, 3), srng.uniform(0.3, 2.0), srng.uniform(-3, 3))
        e = expansions(wf, wr)
        if e is None or e < 3:
            continue
        d64, _ = run(wf, wr, torch.float64, relative_tolerance=NINF)
        if not bool(torch.isfinite(d64)) or abs(float(ref._bar_zero(torch.from_numpy(wf).double(), torch.from_numpy(wr).double(), d64))) > 1e-12:
            continue
        found.append((wf, wr))
    data["expand_a"], data["expand_b"] = found
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x1 = (np.float32(-1e20) + rng.standard_normal(5).astype(np.float32))
        x2 = (np.float32(1e20) + rng.standard_normal(5).astype(np.float32))
        e1 = lambda x: np.float32(0.5) * (x + np.float32(1e20)) ** 2       # noqa: E731
        e2 = lambda x: np.float32(0.5) * (x - np.float32(1e20)) ** 2       # noqa: E731
        data["nooverlap"] = ((np.float32(1.0) + e2(x1)) - e1(x1), e1(x2) - (np.float32(1.0) + e2(x2)))
    assert all(np.isposinf(w).all() and w.dtype == np.float32 for w in data["nooverlap"])

    out = {"seed": np.int64(SEED), "cases": np.array(json.dumps(list(data)))}
    total = 0
    for name, (wf, wr) in data.items():
        assert wf.dtype == np.float32 and wr.dtype == np.float32
        total += wf.nbytes + wr.nbytes
        wf64, wr64 = torch.from_numpy(wf).double(), torch.from_numpy(wr).double()
        finite = name != "nooverlap"
        e = expansions(wf, wr)
        with Counted(10 ** 6) as c:
            d64, u64 = run(wf, wr, torch.float64, relative_tolerance=NINF)
        if finite:
            assert c.calls == 2 + 2 * e + 500, (name, c.calls, e)
        resid = ref._bar_zero(wf64, wr64, d64)
        dd, ud = ref.bennett_acceptance_ratio(wf64, wr64)
        d32, u32 = run(wf, wr, torch.float32)
        if finite:
            assert bool(torch.isfinite(d64)) and abs(float(resid)) <= 1e-12, (name, float(d64), float(resid))
        else:
            assert bool(torch.isnan(d64)) and bool(torch.isnan(u64)) and bool(torch.isnan(dd))
        if name.startswith("expand"):
            assert e >= 3, (name, e)
        out[f"{name}_wf"], out[f"{name}_wr"] = wf, wr
        out[f"{name}_delta64"], out[f"{name}_unc64"], out[f"{name}_resid64"] = np.float64(d64), np.float64(u64), np.float64(resid)
        out[f"{name}_delta_default"], out[f"{name}_unc_default"] = np.float64(dd), np.float64(ud)
        out[f"{name}_delta32"], out[f"{name}_unc32"] = np.float32(d32), np.float32(u32)
        out[f"{name}_n_expand"] = np.int64(e if e is not None else -1)
        print(f"{name}: {len(wf)} / {len(wr)}  delta64 {float(d64):.15g}  unc64 {float(u64):.6g}  resid64 {float(resid):.2e}  "
              f"default - delta64 {float(dd) - float(d64):.2e}  f32 - delta64 {float(d32) - float(d64):.2e}  expansions {e}")
    assert total < 70000, total
    assert out["pos_delta64"] > 0 and out["neg_delta64"] < 0
    assert abs(out["neg_delta_default"] - out["neg_delta64"]) > 1e-8
    assert out["single_delta64"] == (np.float64(data["single"][0][0]) - np.float64(data["single"][1][0])) / 2 or \
        abs(out["single_delta64"] - 0.45) < 1e-7
    out["far_it2"] = np.float64(run(*data["far"], torch.float64, maximum_iterations=2, relative_tolerance=NINF)[0])
    sig = inspect.signature(ref.bennett_acceptance_ratio)
    out["meta"] = np.array(json.dumps({"bennett_acceptance_ratio": [[p.name, "<required>" if p.default is p.empty else p.default]
                                                                   for p in sig.parameters.values()]}))
    path = os.path.join(HERE, "free_energy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; work values", total, "bytes")


if __name__ == "__main__":
    main()
