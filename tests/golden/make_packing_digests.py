#!/usr/bin/env python
"""Generate tests/golden/packed_operand_digests.json: SHA-256 digests of the conditioner operands the torch packers write.

    python tests/golden/make_packing_digests.py

The operand layouts (f32 blocks; split-f16 blocks of 64 lanes x 8 f16 in hi / lo parts under a power-of-two scale, bias blocks) are
the contract between the host and the coupling kernels.  The file pins them bit for bit: tests/test_host_packing.py recomputes the
digests and compares.  Regenerate it only together with a deliberate change of a layout.

Only names reachable as ``bgflow_amd.dense.<name>`` are called (the ``pack_dense_for_*`` functions and ``_pad_hidden``), on CPU tensors,
with the weights of ``hash_init_(DenseNet(units, SiLU()))`` (closed-form values: no RNG, no weight files).  A digest runs over the
dtype, shape and raw bytes of every returned tensor and over ``repr(float(c))`` of every unscale factor, in the order returned.

Cases -- the smallest shapes that reach every branch of the packers:
  spline packers: conditioner inputs n_in in {15, 16} (the bias column is the last slot of a k16-step / the first of a new one) x
      (d, circular dims, bins) in {(3, {1}, 8), (6, {}, 8), (3, {}, 4)}; d = 6 at 8 bins needs two 128-row chunks
        fused            pack_dense_for_fused (f32 layout), 8 bins only
        h2               pack_dense_for_fused_h2, row order 1
        h2_order2        pack_dense_for_fused_h2, row order 2, 8 bins only
        w256             pack_dense_for_fused_w256
        deep1, deep3     pack_dense_for_fused_deep with 1 and 3 hidden layers
        h2_padded        pack_dense_for_fused_h2 on _pad_hidden(linears of [n_in, 40, 100, P], 128)
  affine packers: n_in = 16, H in {64, 128}, d in {5, 33} (one and two output tiles)
        affine_h2, affine_h3         pack_dense_for_affine_h2 with two and three hidden layers
        affine_deep1, affine_deep4   pack_dense_for_affine_deep with 1 and 4 hidden layers
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from bgflow_amd import dense  # noqa: E402
from bgflow_amd.utils import hash_init_  # noqa: E402

PATH = os.path.join(HERE, "packed_operand_digests.json")
SPLINE_SHAPES = [(3, (1,), 8), (6, (), 8), (3, (), 4)]        # (d, circular dims, bins)


def lins(units):
    net = hash_init_(dense.DenseNet(list(units), torch.nn.SiLU()))
    return tuple(net._layers[0::2])


def slots(d, circular):
    """nc_slot_host: rank of a non-circular dim among the non-circular ones, -1 for a circular dim"""
    out, n = [], 0
    for j in range(d):
        out.append(-1 if j in circular else n)
        n += 0 if j in circular else 1
    return np.array(out, dtype=np.int32)


def feed(h, item):
    if torch.is_tensor(item):
        assert item.device.type == "cpu"
        h.update(f"T{item.dtype}{tuple(item.shape)}".encode())
        h.update(item.contiguous().view(torch.uint8).numpy().tobytes())
    elif item is None:
        h.update(b"N")
    elif isinstance(item, (tuple, list)):
        h.update(f"L{len(item)}".encode())
        for it in item:
            feed(h, it)
    else:
        h.update(("F" + repr(float(item))).encode())


def digest(packed):
    h = hashlib.sha256()
    feed(h, packed)
    return h.hexdigest()


def digests():
    out = {}
    for n_in in (15, 16):
        for d, circular, K in SPLINE_SHAPES:
            nc = slots(d, circular)
            P = 3 * K * d + int((nc >= 0).sum())
            tag = f"n_in={n_in},d={d},circular={list(circular)},bins={K}"
            l128 = lins([n_in, 128, 128, P])
            if K == 8:
                out[f"fused[{tag}]"] = digest(dense.pack_dense_for_fused(l128, nc, d, K))
            out[f"h2[{tag}]"] = digest(dense.pack_dense_for_fused_h2(l128, nc, d, K))
            if K == 8:
                out[f"h2_order2[{tag}]"] = digest(dense.pack_dense_for_fused_h2(l128, nc, d, K, row_order=2))
            out[f"w256[{tag}]"] = digest(dense.pack_dense_for_fused_w256(lins([n_in, 256, 256, P]), nc, d, K))
            for hidden in (1, 3):
                out[f"deep{hidden}[{tag}]"] = digest(dense.pack_dense_for_fused_deep(lins([n_in] + [128] * hidden + [P]), nc, d, K))
            out[f"h2_padded[{tag}]"] = digest(dense.pack_dense_for_fused_h2(dense._pad_hidden(lins([n_in, 40, 100, P]), 128), nc, d, K))
    for H in (64, 128):
        for d in (5, 33):
            tag = f"n_in=16,H={H},d={d}"
            out[f"affine_h2[{tag}]"] = digest(dense.pack_dense_for_affine_h2(lins([16, H, H, d])))
            out[f"affine_h3[{tag}]"] = digest(dense.pack_dense_for_affine_h2(lins([16, H, H, H, d])))
            for hidden in (1, 4):
                out[f"affine_deep{hidden}[{tag}]"] = digest(dense.pack_dense_for_affine_deep(lins([16] + [H] * hidden + [d])))
    return out


def main():
    table = digests()
    with open(PATH, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(PATH, len(table), "digests")


if __name__ == "__main__":
    main()
