#!/usr/bin/env python
"""Generate tests/golden/mixture.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_mixture_goldens.py

What runs: the UNMODIFIED reference classes ``MixtureDistribution`` (distribution/mixture.py) and ``NormalDistribution``
(distribution/normal.py), with the two import shims of make_goldens.py.  The fixture holds DATA only; the inputs are regenerated from
seeds by tests/mixture_common.py (its docstring states the recipe) and only their checksums are stored.

Per case (K, d) of mixture_common.CASES, key prefix ``k{K}_d{d}_``, B = 150 rows, trainable weights:

  from the f64 run:   u64 [150]   g64 [150, d] (gradient of sum_b a_b u_b)   neg_e64 [150, K] (``_log_assignments``)
                      gw64_bulk / gw64_far [K]: the gradient with respect to the unnormalised log-weights of sum_b a_b u_b over the
                      148 bulk rows / over the two far rows (row 3 at +1e4, row 4 at -1e3)
  from the reference's own f32 run, relative to 1 + |value64|, separately over the bulk and the far rows:
                      err_u32_{bulk,far}   err_g32_{bulk,far}   err_e32_{bulk,far}   err_w32_{bulk,far}
  check [10]:         checksums of the inputs

Asserted here: every f64 and f32 value of every case is finite (no row is left out of any comparison); the gradient of the component
of weight zero is exactly 0.  Also recorded: one reference ``sample(100)`` of the (7, 5) case in f32 under ``np.random.seed(3);
torch.manual_seed(3)`` (sample_x [100, 5], sample_counts [7]).
"""
import os
import sys
import types

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.distribution.mixture import MixtureDistribution  # noqa: E402
from bgflow.distribution.normal import NormalDistribution  # noqa: E402
import mixture_common as mc  # noqa: E402

REFERENCE = types.SimpleNamespace(MixtureDistribution=MixtureDistribution, NormalDistribution=NormalDistribution)


def run(K, d, dtype):
    inp = mc.inputs(K, d)
    mix = mc.build(REFERENCE, K, d, dtype)
    return mc.evaluate(mix, torch.from_numpy(inp["x"]).to(dtype), torch.from_numpy(inp["a"]).to(dtype))


def main():
    out = {"seed": np.int64(mc.SEED)}
    for K, d in mc.CASES:
        k = mc.key(K, d)
        r64, r32 = run(K, d, torch.float64), run(K, d, torch.float32)
        assert all(v.dtype == np.float64 for v in r64) and all(v.dtype == np.float32 for v in r32)
        assert all(np.isfinite(v).all() for v in r64 + r32), (K, d)
        if K > 2:
            assert r64[3][1] == 0.0 and r64[4][1] == 0.0 and r32[3][1] == 0.0 and r32[4][1] == 0.0
        out[k + "u64"], out[k + "g64"], out[k + "neg_e64"], out[k + "gw64_bulk"], out[k + "gw64_far"] = r64
        G = {key: np.asarray(v) for key, v in out.items()}
        errs = mc.split_errors(*r32, G, k)
        for name, (bulk, far) in errs.items():
            out[f"{k}err_{name}32_bulk"], out[f"{k}err_{name}32_far"] = np.float64(bulk), np.float64(far)
        out[k + "check"] = mc.checksum(mc.inputs(K, d))
        print(f"({K}, {d}): " + ", ".join(f"err_{n}32 {b:.3g} / {f:.3g}" for n, (b, f) in errs.items()) + "  (bulk / far)")
    K, d = mc.SAMPLE_CASE
    mix = mc.build(REFERENCE, K, d, torch.float32)
    np.random.seed(mc.SAMPLE_SEED)
    torch.manual_seed(mc.SAMPLE_SEED)
    x = mix.sample(mc.SAMPLE_N)
    np.random.seed(mc.SAMPLE_SEED)
    counts = np.random.multinomial(mc.SAMPLE_N, mix._log_weights.exp().detach().numpy(), 1)[0]
    assert x.shape == (mc.SAMPLE_N, d) and counts.sum() == mc.SAMPLE_N and counts[1] == 0
    out["sample_x"], out["sample_counts"] = x.detach().numpy(), counts.astype(np.int64)
    print("sample counts", counts)
    path = os.path.join(HERE, "mixture.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
