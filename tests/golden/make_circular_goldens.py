#!/usr/bin/env python
"""Generate tests/golden/circular.npz by IMPORTING the reference (PyTorch-CPU path, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_circular_goldens.py

What runs: the UNMODIFIED reference class ``ConditionalCircularTransformSimple`` (nn/flow/circular.py; its ``_forward`` is
``_cdf_transform`` with the log-density summed over the row) with the two import shims of make_goldens.py; its four "nets" return the
raw parameter tensors.  The fixture holds DATA only; the inputs are regenerated from seeds by tests/circular_common.py (its docstring
states the recipe and the special rows) and only their checksums are stored.

Per case (K, D) of circular_common.CASES, key prefix ``k{K}_d{D}_``, B = 100 rows, q in (out, dlogp, g_y, g_mu, g_ls, g_lw, g_le), the
gradients those of sum a out + sum c dlogp with respect to y and the four RAW parameter tensors [B, K D]:

  {q}64                     the reference's f64 run
  err_{q}32_{bulk,narrow}   its own f32 run against that: max |v - v64| / (1 + |v64|) over the BULK rows / over the NARROW row
  abserr_out32              max |out32 - out64| over BULK and NARROW (the tolerance of the inverse's bracket test)
  cd_gy [2, D], cd_gmu [2, K, D]   central differences (h = 1e-6, f64, one component at a time) of the scalar on the TIES rows
  t [100, D] (f32)          the inverse targets;   check [16]: checksums of the inputs

The case (33, 2) lies outside the kernel's envelope and is compared in values only: its gradient arrays are not stored.

and for the well-conditioned case (4, 3) (prefix ``well_k4_d3_``; no special rows, log_eps >= -2, log_sigma <= 1): the same arrays
over all rows (``err_{q}32_bulk``) and ``min_density``, the smallest f (1 - eps) + eps of its elements.

Asserted here: every f64 value is finite on every row; every f32 value is finite on BULK, NARROW and TIES; the reference's f32 run is
NaN on rows 3 and 4 (log_sigma = 40: inf / inf and 0 inf; dlogp and the gradient of y in every case, out wherever a component
saturates upwards) and wrong by more than 0.1 in ``out`` on row 5 (the seam tie).  If the reference
ever changes, the fixture says so.
"""
import os
import sys

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

from bgflow.nn.flow.circular import ConditionalCircularTransformSimple  # noqa: E402
import circular_common as cc  # noqa: E402


def reference(y, mu_raw, log_sigma, log_weight, log_eps):
    flow = ConditionalCircularTransformSimple(lambda x: mu_raw, lambda x: log_sigma, lambda x: log_weight, lambda x: log_eps)
    return flow._forward(y, y)


def record(out, k, inp, rows_bulk, rows_narrow, values_only=False):
    r64, r32 = cc.evaluate(reference, inp, torch.float64), cc.evaluate(reference, inp, torch.float32)
    assert all(v.dtype == np.float64 for v in r64) and all(v.dtype == np.float32 for v in r32)
    assert all(np.isfinite(v).all() for v in r64), k
    for name, v64, v32 in zip(cc.QUANTITIES, r64, r32):
        if not (values_only and name.startswith("g_")):
            out[f"{k}{name}64"] = v64
        out[f"{k}err_{name}32_bulk"] = np.float64(cc.rel_err(v32[rows_bulk], v64[rows_bulk]))
        if len(rows_narrow):
            out[f"{k}err_{name}32_narrow"] = np.float64(cc.rel_err(v32[rows_narrow], v64[rows_narrow]))
    both = np.concatenate([rows_bulk, rows_narrow]).astype(int)
    out[k + "abserr_out32"] = np.float64(np.abs(r32[0][both].astype(np.float64) - r64[0][both]).max())
    out[k + "t"] = inp["t"]
    out[k + "check"] = cc.checksum(inp)
    return r64, r32


def main():
    out = {"seed": np.int64(cc.SEED)}
    for K, D in cc.CASES:
        k, inp = cc.key(K, D), cc.inputs(K, D)
        r64, r32 = record(out, k, inp, cc.BULK, cc.NARROW, values_only=(K, D) not in cc.ENVELOPE)
        finite = np.concatenate([cc.BULK, cc.NARROW, cc.TIES])
        assert all(np.isfinite(v[finite]).all() for v in r32), (K, D)
        assert all(np.isnan(r32[1][r]) and np.isnan(r32[2][r]).all() for r in (3, 4)), "the reference's f32 run is no longer NaN at log_sigma = 40"
        assert (np.abs(r32[0][5] - r64[0][5]) > 0.1).all(), "the reference's f32 run is no longer wrong on the seam tie"
        cd_gy, cd_gmu = cc.central_differences(reference, inp)
        if (K, D) in cc.ENVELOPE:
            out[k + "cd_gy"], out[k + "cd_gmu"] = cd_gy, cd_gmu
        print(f"({K}, {D}): " + ", ".join(f"{n} {float(out[f'{k}err_{n}32_bulk']):.3g} / {float(out[f'{k}err_{n}32_narrow']):.3g}"
                                          for n in cc.QUANTITIES) + "  (reference f32 error, bulk / narrow)")
        ties = [cc.rel_err(r64[2][cc.TIES], cd_gy), cc.rel_err(r64[3][cc.TIES], cd_gmu.reshape(len(cc.TIES), -1))]
        print(f"    reference f64 autograd against the central differences on the TIES rows: g_y {ties[0]:.3g}, g_mu {ties[1]:.3g}")
    K, D = cc.WELL
    k, inp = cc.key(K, D, well=True), cc.inputs(K, D, well=True)
    r64, r32 = record(out, k, inp, np.arange(cc.B), np.array([], dtype=int))
    assert all(np.isfinite(v).all() for v in r32)
    mr, ls, lw, le, y, *_ = cc.tensors(inp, torch.float64)
    flow = ConditionalCircularTransformSimple(lambda x: mr, lambda x: ls, lambda x: lw, lambda x: le)
    from bgflow.nn.flow.circular import _cdf_transform
    _, logf = _cdf_transform(y, *flow._params(y, y))
    out[k + "min_density"] = np.float64(logf.exp().min())
    assert out[k + "min_density"] >= 0.1
    print(f"well ({K}, {D}): min density {float(out[k + 'min_density']):.3g}, " +
          ", ".join(f"{n} {float(out[f'{k}err_{n}32_bulk']):.3g}" for n in cc.QUANTITIES))
    path = os.path.join(HERE, "circular.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
